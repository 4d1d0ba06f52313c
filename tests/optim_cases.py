"""The optimizer step of include/doda_optim.h restated in fp64 numpy (SGD, Adam, AdamW as torch.optim defines them, and the clip of
torch.nn.utils.clip_grad_norm_: norm, coef, scaled gradient), and the designed tensor and gradient sets of tests/test_optim_host.py
and tests/test_gpu_optim.py.  Reads nothing outside the repository."""
import numpy as np

TILE = 2048          # include/doda_optim.h DODA_OPTIM_TILE: elements per workgroup of both launches
NORM_BLOCKS = 512    # DODA_OPTIM_NORM_BLOCKS: grid cap of the sum-of-squares launch
MAX_NORM = 10.0      # the reference's clip (tool/train.py:100-104)

f32, f64 = np.float32, np.float64


# ---- the tensor sets: a spec per tensor -- shape, storage offset in elements (1: a view the 16-byte path cannot take), has a gradient
def edge_set():
    T = TILE
    shapes = [(1,), (3,), (T - 1,), (T,), (T + 1,), (2 * T + 5,), (27, 16, 16)]
    specs = [dict(shape=s, offset=0, grad=True) for s in shapes]
    specs.append(dict(shape=(2 * T + 1,), offset=1, grad=True))     # unaligned view: the scalar route over more than one tile
    specs.append(dict(shape=(0,), offset=0, grad=True))             # zero elements
    specs.append(dict(shape=(5,), offset=0, grad=False))            # never receives a gradient
    return specs


def many_set(n=320):
    """>= 300 small tensors: the descriptor search over more levels than any network here needs; sizes 1 .. 67, some > 1 tile."""
    specs = [dict(shape=(1 + (7 * k) % 67,), offset=0, grad=True) for k in range(n)]
    specs[n // 2] = dict(shape=(TILE + 9,), offset=0, grad=True)
    return specs


def big_set():
    """Just over NORM_BLOCKS tiles (4 MB): the first workgroups of the sum-of-squares launch take a second grid-stride trip."""
    return [dict(shape=(33,), offset=0, grad=True), dict(shape=(NORM_BLOCKS * TILE + 2 * TILE + 7,), offset=0, grad=True),
            dict(shape=(17,), offset=0, grad=True)]


def numel(spec):
    return int(np.prod(spec["shape"], dtype=np.int64))


def make_params(specs, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s["shape"]).astype(f32) for s in specs]


def make_grads(specs, kind, seed):
    """One gradient per spec (None where the spec has none).  kind: 'large' (norm well above MAX_NORM), 'small' (norm below it: coef
    is 1), 'mixed' (one tensor at 1e4 among the rest at 1e-4: an fp32 sum of squares drops the small ones), 'nan' ('large', one NaN)."""
    rng = np.random.default_rng(seed)
    with_grad = [k for k, s in enumerate(specs) if s["grad"] and numel(s) > 0]
    hot = max(with_grad, key=lambda k: (numel(specs[k]) >= 3 and numel(specs[k]) <= 64, -k))     # a short tensor carries the 1e4s
    out = []
    for k, s in enumerate(specs):
        if not s["grad"]:
            out.append(None)
            continue
        g = rng.standard_normal(s["shape"])
        if kind in ("large", "nan"):
            g *= 3.0
        elif kind == "small":
            g *= MAX_NORM / 8.0 / np.sqrt(max(1, sum(numel(specs[j]) for j in with_grad)))
        elif kind == "mixed":
            g *= 1e4 if k == hot else 1e-4
        else:
            raise ValueError(kind)
        out.append(g.astype(f32))
    if kind == "nan":
        k = with_grad[len(with_grad) // 2]
        out[k].reshape(-1)[numel(specs[k]) // 2] = np.nan
    return out


# ---- the restatement (fp64 throughout; inputs are the fp32 values, exact in fp64)
def grad_norm(grads):
    """sqrt of the sum of squares of every gradient: the squares are exact in fp64 and numpy's pairwise fp64 sum of n of them is
    within about log2(n) * 2^-53 relative of the true sum, 2^29 times finer than an fp32 ulp."""
    return float(np.sqrt(sum(np.sum(np.square(np.asarray(g, dtype=f64))) for g in grads if g is not None)))


def clip_coef(norm, max_norm=MAX_NORM):
    """clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1); a NaN norm stays NaN."""
    c = max_norm / (norm + 1e-6)
    return 1.0 if c > 1.0 else c


def sgd_update(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """torch.optim.SGD on one tensor; buf None: no buffer yet.  Returns (p, buf)."""
    if maximize:
        g = -g
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.copy() if buf is None else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adam_update(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False, decoupled=False):
    """torch.optim.Adam (decoupled: AdamW) on one tensor at step count `step` (1 for the first).  Returns (p, m, v)."""
    beta1, beta2 = betas
    if maximize:
        g = -g
    if weight_decay != 0:
        if decoupled:
            p = p - lr * weight_decay * p
        else:
            g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2_sqrt = np.sqrt(1 - beta2 ** step)
    return p - (lr / bc1) * m / (np.sqrt(v) / bc2_sqrt + eps), m, v


class Restated:
    """An optimizer over a list of tensors in fp64: kind 'sgd' | 'adam' | 'adamw', torch's hyper-parameter names in `hyper`,
    max_norm None for no clip.  step(grads) takes fp32 (or fp64) gradients, None for a tensor without one, and returns
    (norm, coef, scaled gradients) — (None, 1.0, the gradients) without the clip."""

    def __init__(self, kind, params, max_norm=None, **hyper):
        self.kind, self.max_norm, self.hyper = kind, max_norm, dict(hyper)
        self.p = [np.asarray(p, dtype=f64).copy() for p in params]
        self.s1 = [None] * len(params)      # momentum buffer | exp_avg
        self.s2 = [None] * len(params)      # exp_avg_sq
        self.steps = [0] * len(params)

    def step(self, grads):
        grads = [None if g is None else np.asarray(g, dtype=f64) for g in grads]
        norm, coef = None, 1.0
        if self.max_norm is not None:
            norm = grad_norm(grads)
            coef = clip_coef(norm, self.max_norm)
            grads = [None if g is None else g * coef for g in grads]
        h = dict(self.hyper)
        lr = h.pop("lr")
        for k, g in enumerate(grads):
            if g is None:
                continue
            self.steps[k] += 1
            if self.kind == "sgd":
                self.p[k], self.s1[k] = sgd_update(self.p[k], g, self.s1[k], lr, **h)
            else:
                if self.s1[k] is None:
                    self.s1[k], self.s2[k] = np.zeros_like(self.p[k]), np.zeros_like(self.p[k])
                self.p[k], self.s1[k], self.s2[k] = adam_update(self.p[k], g, self.s1[k], self.s2[k], self.steps[k], lr,
                                                                decoupled=self.kind == "adamw", **h)
        return norm, coef, grads


def ulp_distance(x32, ref64):
    """Largest distance of the fp32 array x32 to the fp64 array ref64 in units of the fp32 spacing at the reference (0 for two
    NaNs or equal infinities at the same place, inf where only one is finite)."""
    x = np.asarray(x32, dtype=f64).reshape(-1)
    r = np.asarray(ref64, dtype=f64).reshape(-1)
    if x.size == 0:
        return 0.0
    same = (np.isnan(x) & np.isnan(r)) | (x == r)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(x - r) / np.spacing(np.abs(r.astype(f32))).astype(f64)
    d = np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))
    return float(d.max())

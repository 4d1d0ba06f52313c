"""GPU tests of the optimizer step with the clip folded in (include/doda_optim.h, csrc/optim.hip, doda_amd.optim) on the designed
tensor and gradient sets of tests/optim_cases.py, against its fp64 restatement and against torch's own optimizers.

Bounds.  The norm: fp32 x fp32 products are exact in fp64 and the fp64 sums have fewer than 2^24 terms, so the device's fp64 sum is
within 2^-29 relative of the true one; one square root and one rounding to fp32 later it is within 1 fp32 ulp of the fp32 rounding of
the restatement.  Adam / AdamW / SGD: bit equality with torch's fused kernels (whose arithmetic the kernel follows term by term),
which is what the MI355X gives; the distances of all three routes to the fp64 restatement are printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"edge": oc.edge_set, "many": oc.many_set, "big": oc.big_set}
_HOST = {}


def dev():
    return torch.device("cuda:0")


def host_case(set_name, grad_kind, seed=0):
    """(specs, fp32 parameters, fp32 gradients) of a designed set, made once."""
    key = (set_name, grad_kind, seed)
    if key not in _HOST:
        specs = SETS[set_name]()
        _HOST[key] = (specs, oc.make_params(specs, 100 + seed), oc.make_grads(specs, grad_kind, 200 + seed))
    return _HOST[key]


def to_dev(specs, arrays):
    """Device tensors of the arrays; a spec with offset 1 becomes a view one element into its storage (not 16-byte aligned)."""
    out = []
    for s, a in zip(specs, arrays):
        if a is None:
            out.append(None)
            continue
        t = torch.from_numpy(a).to(dev())
        if s["offset"]:
            base = torch.empty(t.numel() + s["offset"], device=dev())
            view = base[s["offset"]:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 != 0
            t = view
        out.append(t)
    return out


def make_params(specs, arrays):
    return [torch.nn.Parameter(t) for t in to_dev(specs, arrays)]


def set_grads(params, specs, grads):
    for p, g in zip(params, to_dev(specs, grads)):
        p.grad = g


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def state_of(opt, p, key):
    return opt.state[p][key] if p in opt.state and key in opt.state[p] else None


# ---- the norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name,grad_kind", [("edge", "large"), ("edge", "small"), ("edge", "mixed"), ("edge", "nan"),
                                                ("many", "large"), ("many", "mixed"), ("big", "large"), ("big", "mixed")])
def test_grad_norm_is_the_fp64_norm_and_reproducible(native_lib, set_name, grad_kind):
    """last_grad_norm against the restatement's norm rounded to fp32, within 1 ulp; a second run on the same input gives the same
    bits of the norm, the parameters and the stored gradients."""
    from doda_amd.optim import FusedSGD
    specs, p0, g0 = host_case(set_name, grad_kind)
    want = np.float32(oc.grad_norm(g0))
    runs = []
    for _ in range(2):
        ps = make_params(specs, p0)
        opt = FusedSGD(ps, lr=0.01, max_grad_norm=oc.MAX_NORM)
        set_grads(ps, specs, g0)
        opt.step()
        assert opt.clips_in_step and opt.last_grad_norm.is_cuda and opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.dim() == 0
        runs.append((opt.last_grad_norm.clone(), [p.detach().clone() for p in ps], [p.grad.clone() for p in ps if p.grad is not None]))
    torch.cuda.synchronize()
    got = runs[0][0].cpu().numpy()
    print("norm %s/%s: device %r, restatement %r" % (set_name, grad_kind, got, want))
    if grad_kind == "nan":
        assert np.isnan(got) and np.isnan(want)
    else:
        assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1
    assert same_bits(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert same_bits(a, b)


# ---- Adam / AdamW ---------------------------------------------------------------------------------------------------------------
def _specs_and_inputs(seed=1):
    """The edge set and the >= 300 small tensors in one parameter list; four gradient sets (large, large, small, large)."""
    key = ("adam-inputs", seed)
    if key not in _HOST:
        specs = oc.edge_set() + oc.many_set()
        _HOST[key] = (specs, oc.make_params(specs, seed), [oc.make_grads(specs, kind, 10 * seed + it)
                                                           for it, kind in enumerate(("large", "large", "small", "large"))])
    return _HOST[key]


def _run_steps(make_opt, specs, p0, grad_steps, lrs, clip_with_torch=None, reload_at=3):
    """Four steps of an optimizer over fresh device copies: lr per step, a state-dict round trip into a fresh instance before step
    `reload_at`; clip_with_torch: clip_grad_norm_ before every step (the two-call route).  Returns (params, optimizer, the gradients
    left in p.grad after the last step, the norms, the gradients left after every step as numpy arrays)."""
    ps = make_params(specs, p0)
    opt = make_opt(ps)
    norms, left = [], []
    for it, grads in enumerate(grad_steps):
        if it == reload_at:
            sd = opt.state_dict()
            opt = make_opt(ps)
            opt.load_state_dict(sd)
        opt.param_groups[0]["lr"] = lrs[it]
        set_grads(ps, specs, grads)
        if clip_with_torch is not None:
            norms.append(torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], clip_with_torch))
        opt.step()
        if getattr(opt, "clips_in_step", False):
            norms.append(opt.last_grad_norm.clone())
        left.append([None if p.grad is None else p.grad.cpu().numpy() for p in ps])
    torch.cuda.synchronize()
    return ps, opt, [None if p.grad is None else p.grad.clone() for p in ps], norms, left


def _distances(ps, opt, rs, keys):
    """Largest ulp distance of the parameters and the state tensors to the restatement."""
    d = {"p": 0.0, keys[0]: 0.0, keys[1]: 0.0}
    for k, p in enumerate(ps):
        d["p"] = max(d["p"], oc.ulp_distance(p.detach().cpu().numpy(), rs.p[k]))
        for key, ref in zip(keys, (rs.s1[k], rs.s2[k])):
            st = state_of(opt, p, key)
            if st is not None and ref is not None:
                d[key] = max(d[key], oc.ulp_distance(st.cpu().numpy(), ref))
    return d


LRS = (1e-2, 1e-2, 2.5e-3, 2.5e-3)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("clip", [None, oc.MAX_NORM])
def test_fused_adam_is_torchs_fused_adam(native_lib, kind, wd, maximize, clip):
    """Four steps (lr changed after two, state-dict round trip into a fresh instance before the fourth, one step below the clip's
    threshold) of FusedAdam / FusedAdamW against torch.optim.Adam / AdamW(fused=True) — after clip_grad_norm_ under the clip — bit
    for bit: parameters, exp_avg, exp_avg_sq, and the step counts as torch's non-fused layout keeps them.  Under the clip the two
    routes scale by coefs that can differ in the last fp32 bit (fp64 here, fp32 in clip_grad_norm_), so there bit equality is asserted
    against torch's fused step fed with the gradients this step wrote back, and against clip_grad_norm_ + fused step the bound is:
    the distance to the fp64 restatement no greater than twice the larger of torch-fused's and torch-single-tensor's own, plus
    1 ulp (the factor 2: one differently rounded operation per element and no more)."""
    from doda_amd import optim
    specs, p0, grad_steps = _specs_and_inputs()
    mine_cls = optim.FusedAdam if kind == "adam" else optim.FusedAdamW
    ref_cls = torch.optim.Adam if kind == "adam" else torch.optim.AdamW
    kw = dict(lr=LRS[0], betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, maximize=maximize)
    mine = _run_steps(lambda ps: mine_cls(ps, max_grad_norm=clip, **kw), specs, p0, grad_steps, LRS)
    fused = _run_steps(lambda ps: ref_cls(ps, fused=True, **kw), specs, p0, grad_steps, LRS, clip_with_torch=clip)
    single = _run_steps(lambda ps: ref_cls(ps, foreach=False, **kw), specs, p0, grad_steps, LRS, clip_with_torch=clip)
    rs = oc.Restated(kind, p0, max_norm=clip, **kw)
    for it, grads in enumerate(grad_steps):
        rs.hyper["lr"] = LRS[it]
        norm, coef, scaled = rs.step(grads)
        assert clip is None or (coef == 1.0) == (it == 2)
    keys = ("exp_avg", "exp_avg_sq")
    dist = {name: _distances(run[0], run[1], rs, keys) for name, run in (("mine", mine), ("fused", fused), ("single", single))}
    equal = all(same_bits(a, b) for a, b in zip(mine[0], fused[0])) and all(
        same_bits(mine[1].state[a][key], fused[1].state[b][key]) for a, b in zip(mine[0], fused[0]) if a in mine[1].state and mine[1].state[a]
        for key in keys)
    print("%s wd=%g maximize=%s clip=%s: bit-equal to torch fused: %s; ulp distances to fp64 %s" % (kind, wd, maximize, clip, equal, dist))
    for a, b in zip(mine[0], fused[0]):       # the same tensors have state, with the same step counts, kept on the host
        sa, sb = mine[1].state.get(a, {}), fused[1].state.get(b, {})
        assert set(sa) == set(sb) and (not sa or float(sa["step"]) == float(sb["step"]) == 4.0)
        assert not sa or (sa["step"].device.type == "cpu" and sa["step"].dtype == torch.float32)
    if clip is None:
        assert equal
        for g, g0 in zip(mine[2], to_dev(specs, grad_steps[-1])):       # without the clip the gradients are only read
            assert g is None or same_bits(g, g0)
    else:
        fed = _run_steps(lambda ps: ref_cls(ps, fused=True, **kw), specs, p0, mine[4], LRS)
        for a, b in zip(mine[0], fed[0]):
            assert same_bits(a, b)
            for key in keys:
                if a in mine[1].state and mine[1].state[a]:
                    assert same_bits(mine[1].state[a][key], fed[1].state[b][key])
        for key in ("p",) + keys:
            assert dist["mine"][key] <= 2 * max(dist["fused"][key], dist["single"][key]) + 1, (key, dist)
    plain = ref_cls(mine[0], **kw)
    plain.load_state_dict(mine[1].state_dict())                 # the state loads into the plain torch optimizer


# ---- the clip -------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def _check_clipped_step(kind, mine_cls, kw, keys):
    """One step of an optimizer under max_grad_norm on the three finite gradient sets and the NaN set, from the same fp32 inputs as
    the restatement.  p.grad after step() is g * coef in fp32, exactly, for one coef within an fp32 ulp of the restatement's.
    Parameters and state: every fp32 rounding is 2^-24 relative; the scaled gradient carries one, a coef up to 1.5 ulp off three
    more, a state value one (the gradient enters exp_avg_sq squared: twice that), and the update at most six more (step size, square
    root, quotient, sum, product, quotient).  So with gmag = |g coef| (+ weight_decay |p| where the decay enters the gradient) the
    bounds are 8 x 2^-24 x the state's own scale in gmag, and for a parameter one fp32 spacing at the result per rounding of the
    parameter itself (one; two for AdamW's decay, whose result adam_math keeps in fp32) plus 16 x 2^-24 x the size of what was
    subtracted.  Below the threshold: bit-equal to the unclipped step."""
    specs, p0, _ = _specs_and_inputs()
    if kind == "sgd":       # the unclipped twin goes through doda_sgd_multi, which takes no tensor without storage
        keep = [k for k, s in enumerate(specs) if oc.numel(s)]
        specs, p0 = [specs[k] for k in keep], [p0[k] for k in keep]
    lr, wd = kw["lr"], kw.get("weight_decay", 0.0)
    for grad_kind in ("large", "small", "mixed", "nan"):
        g0 = oc.make_grads(specs, grad_kind, 77)
        ps = make_params(specs, p0)
        opt = mine_cls(ps, max_grad_norm=oc.MAX_NORM, **kw)
        set_grads(ps, specs, g0)
        opt.step()                                              # (returns: no error status under NaN either)
        ps0 = make_params(specs, p0)
        opt0 = mine_cls(ps0, **kw)
        set_grads(ps0, specs, g0)
        opt0.step()
        torch.cuda.synchronize()
        rs = oc.Restated(kind, p0, max_norm=oc.MAX_NORM, **kw)
        norm, coef, scaled = rs.step(g0)
        if grad_kind == "nan":
            assert np.isnan(norm) and bool(torch.isnan(opt.last_grad_norm))
            for k, (p, s) in enumerate(zip(ps, specs)):
                if s["grad"] and oc.numel(s):
                    assert bool(torch.isnan(p).all()) and bool(torch.isnan(p.grad).all())
                elif not s["grad"]:
                    assert same_bits(p, ps0[k])
            continue
        c32 = np.float32(coef)
        cands = [c32, np.nextafter(c32, np.float32(0)), np.nextafter(c32, np.float32(2))]
        if grad_kind == "small":
            assert coef == 1.0
            cands = [np.float32(1)]
        hit = [all(np.array_equal(p.grad.cpu().numpy(), g * c) for p, g in zip(ps, g0) if g is not None) for c in cands]
        assert any(hit), (grad_kind, coef)
        for k, (p, q) in enumerate(zip(ps, ps0)):
            if g0[k] is None:
                assert p.grad is None and same_bits(p, q)
                continue
            if grad_kind == "small":                            # coef 1: the unclipped step, bit for bit
                assert same_bits(p, q) and same_bits(p.grad, q.grad)
                for key in keys:
                    a, b = state_of(opt, p, key), state_of(opt0, q, key)
                    assert (a is None and b is None) or same_bits(a, b)
            p64 = p0[k].astype(np.float64)
            gmag = np.abs(scaled[k]) + (wd * np.abs(p64) if kind != "adamw" else 0.0)
            got = p.detach().cpu().numpy().astype(np.float64)
            moved = np.abs(rs.p[k] - p64) + 2 * lr * wd * np.abs(p64) + (lr * 2 * gmag if kind == "sgd" else 0.0)
            roundings = 2 if kind == "adamw" and wd else 1      # torch rounds the decayed parameter to fp32 before the Adam update
            tol = roundings * np.spacing(np.abs(rs.p[k]).astype(np.float32)).astype(np.float64) + 16 * EPS32 * moved
            assert np.all(np.abs(got - rs.p[k]) <= tol), (grad_kind, k, float(np.max(np.abs(got - rs.p[k]) / tol)))
            if kind == "sgd":
                scales = (gmag, gmag)                            # first step: the buffer is the gradient that entered
            else:
                b1, b2 = kw["betas"]
                scales = ((1 - b1) * gmag, 2 * (1 - b2) * gmag * gmag)
            for key, ref, scale in zip(keys, (rs.s1[k], rs.s2[k]), scales):
                st = state_of(opt, p, key)
                if st is not None and ref is not None:
                    err = np.abs(st.cpu().numpy().astype(np.float64) - ref)
                    assert np.all(err <= 8 * EPS32 * scale + 1e-45), (grad_kind, k, key)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_adam_clip_writes_back_the_clipped_gradient(native_lib, kind):
    from doda_amd import optim
    _check_clipped_step(kind, optim.FusedAdam if kind == "adam" else optim.FusedAdamW,
                        dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05), ("exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("kw", [dict(lr=0.05, momentum=0.9, weight_decay=1e-4), dict(lr=0.05), dict(lr=0.05, momentum=0.9, nesterov=True)])
def test_sgd_clip_writes_back_the_clipped_gradient(native_lib, kw):
    from doda_amd.optim import FusedSGD
    _check_clipped_step("sgd", FusedSGD, kw, ("momentum_buffer", "momentum_buffer"))


@pytest.mark.parametrize("momentum,nesterov,wd", [(0.9, False, 1e-4), (0.0, False, 0.0), (0.9, True, 1e-2)])
def test_sgd_with_clip_is_clip_grad_norm_then_fused_sgd(native_lib, momentum, nesterov, wd):
    """Four steps of FusedSGD(max_grad_norm=10) against clip_grad_norm_ + torch.optim.SGD(fused=True) and the single-tensor route,
    under the bound of the Adam test (the coefs of the two routes can differ in the last fp32 bit)."""
    from doda_amd.optim import FusedSGD
    specs, p0, grad_steps = _specs_and_inputs()
    kw = dict(lr=LRS[0], momentum=momentum, nesterov=nesterov, weight_decay=wd)
    mine = _run_steps(lambda ps: FusedSGD(ps, max_grad_norm=oc.MAX_NORM, **kw), specs, p0, grad_steps, LRS)
    fused = _run_steps(lambda ps: torch.optim.SGD(ps, fused=True, **kw), specs, p0, grad_steps, LRS, clip_with_torch=oc.MAX_NORM)
    single = _run_steps(lambda ps: torch.optim.SGD(ps, foreach=False, **kw), specs, p0, grad_steps, LRS, clip_with_torch=oc.MAX_NORM)
    rs = oc.Restated("sgd", p0, max_norm=oc.MAX_NORM, **kw)
    for it, grads in enumerate(grad_steps):
        rs.hyper["lr"] = LRS[it]
        rs.step(grads)
    keys = ("momentum_buffer", "momentum_buffer")
    dist = {name: _distances(run[0], run[1], rs, keys) for name, run in (("mine", mine), ("fused", fused), ("single", single))}
    print("sgd momentum=%g nesterov=%s wd=%g with clip: ulp distances to fp64 %s" % (momentum, nesterov, wd, dist))
    for key in ("p", "momentum_buffer"):
        assert dist["mine"][key] <= 2 * max(dist["fused"][key], dist["single"][key]) + 1, (key, dist)
    for a, b in zip(mine[3], fused[3]):                         # the norms of the two routes: fp64 here, fp32 sums there
        assert abs(float(a) - float(b)) <= 4e-6 * float(b)


# ---- unchanged results ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum,nesterov,wd", [(0.9, False, 1e-4), (0.0, False, 0.0), (0.9, True, 1e-2)])
def test_fused_sgd_without_clip_gives_the_bits_of_doda_sgd_multi(native_lib, momentum, nesterov, wd):
    """FusedSGD without max_grad_norm still goes through doda_sgd_multi: four steps bit-equal to torch's fused SGD (what
    tests/test_gpu_round2.py pins) and to direct calls of ops.sgd_multi; a clip that never bites (max_grad_norm = 1e30: coef 1)
    through doda_optim_step gives the same bits too."""
    from doda_amd import ops
    from doda_amd.optim import FusedSGD
    specs, p0, grad_steps = _specs_and_inputs()
    keep = [k for k, s in enumerate(specs) if oc.numel(s)]      # (doda_sgd_multi takes no tensor without storage)
    specs, p0, grad_steps = [specs[k] for k in keep], [p0[k] for k in keep], [[g[k] for k in keep] for g in grad_steps]
    kw = dict(lr=LRS[0], momentum=momentum, nesterov=nesterov, weight_decay=wd)
    mine = _run_steps(lambda ps: FusedSGD(ps, **kw), specs, p0, grad_steps, LRS)
    assert not mine[1].clips_in_step and mine[1].last_grad_norm is None
    fused = _run_steps(lambda ps: torch.optim.SGD(ps, fused=True, **kw), specs, p0, grad_steps, LRS)
    loose = _run_steps(lambda ps: FusedSGD(ps, max_grad_norm=1e30, **kw), specs, p0, grad_steps, LRS)
    ps = make_params(specs, p0)
    bufs = [torch.empty_like(p, memory_format=torch.contiguous_format) if momentum else None for p in ps]
    for it, grads in enumerate(grad_steps):
        gs = to_dev(specs, grads)
        sel = [k for k, g in enumerate(gs) if g is not None]
        with torch.no_grad():
            ops.sgd_multi([ps[k] for k in sel], [gs[k] for k in sel], [bufs[k] for k in sel], [it == 0] * len(sel), LRS[it], momentum,
                          0.0, wd, nesterov, False)
    torch.cuda.synchronize()
    for k, (a, b, c, d) in enumerate(zip(mine[0], fused[0], loose[0], ps)):
        assert same_bits(a, b) and same_bits(a, c) and same_bits(a, d), k
        if momentum and grad_steps[0][k] is not None:
            assert same_bits(mine[1].state[a]["momentum_buffer"], bufs[k])
            assert same_bits(mine[1].state[a]["momentum_buffer"], loose[1].state[c]["momentum_buffer"])


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import optim_cases as oc
import test_gpu_optim as t
from doda_amd import optim
from doda_amd._ext import ext
specs, p0, grad_steps = t._specs_and_inputs()
kw = dict(lr=t.LRS[0], betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
ps, opt, grads, norms, _ = t._run_steps(lambda ps: optim.FusedAdamW(ps, max_grad_norm=oc.MAX_NORM, **kw), specs, p0, grad_steps, t.LRS)
np.savez(sys.argv[2], ext=np.array(ext is not None), norms=np.array([float(n) for n in norms], dtype=np.float32),
         **{"p%d" % k: p.detach().cpu().numpy() for k, p in enumerate(ps)},
         **{"g%d" % k: g.cpu().numpy() for k, g in enumerate(grads) if g is not None},
         **{"m%d" % k: opt.state[p]["exp_avg"].cpu().numpy() for k, p in enumerate(ps) if p in opt.state and opt.state[p]},
         **{"v%d" % k: opt.state[p]["exp_avg_sq"].cpu().numpy() for k, p in enumerate(ps) if p in opt.state and opt.state[p]})
"""


def test_ctypes_route_gives_the_bits_of_the_extension_route(native_lib, tmp_path):
    """DODA_NO_EXT=1 (doda_amd.ops.optim_step over ctypes) in a fresh child process against the extension route in this one: the
    same four AdamW steps under the clip, every output bit for bit."""
    from doda_amd import optim
    from doda_amd._ext import ext
    assert ext is not None and hasattr(ext, "optim_step")
    path = str(tmp_path / "ctypes.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DODA_NO_EXT="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    child = dict(np.load(path))
    assert not bool(child.pop("ext"))
    specs, p0, grad_steps = _specs_and_inputs()
    kw = dict(lr=LRS[0], betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    ps, opt, grads, norms, _ = _run_steps(lambda ps: optim.FusedAdamW(ps, max_grad_norm=oc.MAX_NORM, **kw), specs, p0, grad_steps, LRS)
    here = {"norms": np.array([float(n) for n in norms], dtype=np.float32)}
    for k, p in enumerate(ps):
        here["p%d" % k] = p.detach().cpu().numpy()
        if grads[k] is not None:
            here["g%d" % k] = grads[k].cpu().numpy()
        if p in opt.state and opt.state[p]:
            here["m%d" % k], here["v%d" % k] = opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy()
    assert set(here) == set(child) and len(here) > 4 * 300
    for key, a in here.items():
        b = child[key]
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), key


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def test_train_entry_point_with_adamw_and_clip(native_lib, tmp_path):
    """python -m doda_amd.train under cfgs/synthetic/spconv_adamw_clip.yaml on tiny synthetic scenes: FusedAdamW with the clip inside
    its step, finite losses that move, and a checkpoint whose optimizer state loads into plain torch.optim.AdamW."""
    import re
    from doda_amd import model, st
    from doda_amd.train import build_optimizer
    argv = ["--cfg_file", "doda_amd/cfgs/synthetic/spconv_adamw_clip.yaml", "--epochs", "1", "--max_iters", "4", "--output_root", str(tmp_path),
            "--scene_cache", str(tmp_path / "scenes"), "--manual_seed", "3", "--synthetic_scenes", "4", "--synthetic_base", "4",
            "--synthetic_voxels", "5000", "--batch_size", "2", "--print_freq", "1", "--dtype", "f32"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "doda_amd.train"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    losses = [float(v) for v in re.findall(r"Loss ([0-9.naninf-]+) Accuracy", r.stdout)]
    print("adamw + clip training losses:", losses)
    assert len(losses) >= 2 and all(np.isfinite(v) and v > 0 for v in losses) and len(set(losses)) > 1
    args, cfg = st.parse_config(list(argv))
    assert cfg.OPTIMIZATION.optim == "adamw" and cfg.OPTIMIZATION.clip_grad is True
    ckpts = sorted((tmp_path / "cfgs" / "synthetic" / "spconv_adamw_clip").rglob("*.pth"))
    assert ckpts, r.stdout[-2000:]
    ckpt = torch.load(str(ckpts[-1]), map_location="cpu", weights_only=False)
    net = model.SparseConvNet(cfg).to(dev())
    opt = build_optimizer(cfg.OPTIMIZATION, net)
    assert type(opt).__name__ == "FusedAdamW" and opt.clips_in_step and opt.max_grad_norm == 10.0
    opt.load_state_dict(ckpt["optimizer"])
    plain = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=cfg.OPTIMIZATION.base_lr)
    plain.load_state_dict(ckpt["optimizer"])
    st0 = next(iter(plain.state.values()))
    assert set(st0) == {"step", "exp_avg", "exp_avg_sq"} and float(st0["step"]) >= 2.0 and bool(torch.isfinite(st0["exp_avg"]).all())

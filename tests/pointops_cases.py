"""Numpy fp32 restatements of the pointops operators (include/doda_pointops.h) and the designed inputs of their tests.

Written from the header's formulas: every product, sum and difference is one fp32 numpy operation (rounded once), every sum starts
at 0 and takes its terms in the stated order — `i` ascending in the forwards, ascending flat position inside a destination's list
in the backwards.  The loops run over the summation index and are vectorised over everything that is independent of it, which
leaves the order of every single sum as stated.  An index outside [0, n) reads as 0 in a forward and receives no gradient."""
import numpy as np

F = np.float32
WAVE_LIST = 64          # include/doda_pointops.h DODA_PO_WAVE_LIST
FPS_BLOCK = 1024        # DODA_PO_FPS_BLOCK
FPS_REG = 8             # DODA_PO_FPS_REG
EPS = 2.0 ** -24


# ---- furthest point sampling -------------------------------------------------------------------------------------------------------
def _segments(ends, total):
    lo, out = 0, []
    for e in ends:
        a, b = min(max(lo, 0), total), min(max(int(e), 0), total)
        out.append((a, max(a, b)))
        lo = int(e)
    return out


def _dist(points, centre):
    acc = np.zeros(points.shape[0], F)
    for d in range(points.shape[1]):
        diff = points[:, d] - centre[d]
        acc = acc + diff * diff
    return acc


def fps(xyz, offset, new_offset, pick=None):
    """idx int32 [new_offset[-1]]; offset / new_offset: END offsets.  pick(t): the winner among the running distances t (default:
    the first maximum, i.e. ties to the lowest index)."""
    xyz = np.asarray(xyz, F)
    m = int(new_offset[-1]) if len(new_offset) else 0
    idx = np.full(m, -2, np.int32)
    for (lo, hi), (olo, ohi) in zip(_segments(offset, xyz.shape[0]), _segments(new_offset, m)):
        if ohi == olo:
            continue
        if hi == lo:
            idx[olo:ohi] = -1
            continue
        pts = xyz[lo:hi]
        run = np.full(hi - lo, 1e10, F)
        cur = 0
        idx[olo] = lo
        for s in range(olo + 1, ohi):
            run = np.minimum(run, _dist(pts, pts[cur]))
            cur = int(np.argmax(run)) if pick is None else pick(run)
            idx[s] = lo + cur
    return idx


def block_tie_rule(block):
    """The reference's winner: thread `k % block` keeps its first maximum, and the LDS tree (strict compare, lower slot kept) lets
    the thread with the smallest bit-reversed id win among equal threads."""
    bits = block.bit_length() - 1

    def pick(run):
        ties = np.flatnonzero(run == run.max())
        rev = [int(format(int(k) % block, "0%db" % bits)[::-1], 2) if bits else 0 for k in ties]
        return int(ties[np.lexsort((ties, rev))[0]])
    return pick


class FpsCase:
    def __init__(self, name, xyz, sizes, wants):
        self.name, self.xyz = name, np.ascontiguousarray(xyz, F)
        self.sizes, self.wants = list(sizes), list(wants)
        self.offset = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)            # with the wrappers' leading 0
        self.new_offset = np.concatenate(([0], np.cumsum(wants))).astype(np.int32)
        assert self.xyz.shape[0] == self.offset[-1]


def _cloud(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(F)


def grid_cloud():
    g = np.arange(6, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def fps_cases():
    rng = np.random.default_rng(2024)
    sizes = [1, 2, 63, 64, 65, 1023, 1024, 1025]
    wants = [4, 2, 1, 0, 68, 1023, 1027, 1025]                    # 0, 1, n_b and n_b + 3 all occur
    spill = FPS_BLOCK * FPS_REG + 1
    cases = []
    for dim in (3, 6):
        cases.append(FpsCase("sizes_d%d" % dim, _cloud(rng, sum(sizes), dim), sizes, wants))
        cases.append(FpsCase("spill_d%d" % dim, _cloud(rng, spill, dim), [spill], [spill + 3 if dim == 3 else 700]))
        five = [100, 0, 300, 0, 70]
        cases.append(FpsCase("five_d%d" % dim, _cloud(rng, sum(five), dim), five, [100, 4, 303, 0, 1]))
    cases.append(FpsCase("seg2500", _cloud(rng, 2500, 3), [2500], [2500]))
    cases.append(FpsCase("grid", grid_cloud(), [216], [60]))
    half = _cloud(rng, 150, 3)
    cases.append(FpsCase("duplicates", np.concatenate((half, half))[rng.permutation(300)], [300], [300]))
    pair = np.concatenate((_cloud(rng, 40, 3), grid_cloud()))
    cases.append(FpsCase("grid_second", pair, [40, 216], [43, 216]))
    return cases


# ---- the index by destination ------------------------------------------------------------------------------------------------------
def transpose(idx, n):
    flat = np.asarray(idx, np.int64).reshape(-1)
    valid = (flat >= 0) & (flat < n)
    p = np.flatnonzero(valid)
    order = np.argsort(flat[p], kind="stable")                      # by destination, ascending position inside
    start = np.zeros(n + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(flat[p], minlength=n))
    return start, p[order].astype(np.int32)


def transpose_case(m, nsample, n=50, seed=5):
    """Lists of WAVE_LIST - 1, WAVE_LIST and WAVE_LIST + 1 entries (destinations 0, 1, 2), destination 3 never referenced, the
    invalid values -1 and n, the rest spread over the other destinations."""
    rng = np.random.default_rng(seed + nsample)
    total = m * nsample
    head = [0] * (WAVE_LIST - 1) + [1] * WAVE_LIST + [2] * (WAVE_LIST + 1) + [-1, n, -1, n + 7, -2 ** 31]
    assert total >= len(head) and total % 64
    flat = np.concatenate((head, rng.integers(4, n, total - len(head)))).astype(np.int32)
    return flat[rng.permutation(total)].reshape(m, nsample), n


# ---- the four pairs ------------------------------------------------------------------------------------------------------------------
def _rows(x, idx):
    """x[idx] with 0 for an index outside the array."""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < x.shape[0])
    out = x[np.where(ok, idx, 0)]
    out[~ok] = 0
    return out


def gather_sum(term, idx, n):
    """out[j] = the sum, in ascending position, of term[p] over j's list; term [total, c]."""
    start, pos = transpose(idx, n)
    out = np.zeros((n, term.shape[1]), F)
    length = np.diff(start)
    for t in range(int(length.max()) if n else 0):
        j = np.flatnonzero(length > t)
        out[j] = out[j] + term[pos[start[j] + t]]
    return out


def grouping_fwd(inp, idx):
    return _rows(inp, idx)


def grouping_bwd(d_out, idx, n):
    return gather_sum(d_out.reshape(-1, d_out.shape[-1]), idx, n)


def interpolation_fwd(inp, idx, w):
    out = np.zeros((idx.shape[0], inp.shape[1]), F)
    for i in range(idx.shape[1]):
        out = out + _rows(inp, idx[:, i]) * w[:, i:i + 1]
    return out


def interpolation_bwd(d_out, idx, w, n):
    k = idx.shape[1]
    return gather_sum((d_out[:, None, :] * w[:, :, None]).reshape(-1, d_out.shape[1]), idx, n) if k else np.zeros((n, d_out.shape[1]), F)


def subtraction_fwd(a, b, idx):
    return a[:, None, :] - _rows(b, idx)


def subtraction_bwd(d_out, idx, n):
    d_a = np.zeros((d_out.shape[0], d_out.shape[2]), F)
    for i in range(d_out.shape[1]):
        d_a = d_a + d_out[:, i]
    return d_a, gather_sum((-d_out).reshape(-1, d_out.shape[2]), idx, n)


def _wide(w, c):
    """w[..., ch % w_c] for ch in range(c)."""
    return w[..., np.arange(c) % w.shape[-1]]


def aggregation_fwd(inp, position, w, idx):
    c = inp.shape[1]
    out = np.zeros((idx.shape[0], c), F)
    ww = _wide(w, c)
    for i in range(idx.shape[1]):
        out = out + (_rows(inp, idx[:, i]) + position[:, i]) * ww[:, i]
    return out


def aggregation_bwd(inp, position, w, idx, g):
    c, w_c = inp.shape[1], w.shape[-1]
    ww = _wide(w, c)
    d_position = g[:, None, :] * ww
    prod = g[:, None, :] * (_rows(inp, idx) + position)
    d_w = np.zeros(w.shape, F)
    for ch in range(c):
        d_w[:, :, ch % w_c] = d_w[:, :, ch % w_c] + prod[:, :, ch]
    return gather_sum(d_position.reshape(-1, c), idx, inp.shape[0]), d_position, d_w


HOT_ROWS = 3000     # rows whose first index is destination 5


def _mixed(rng, *shape):
    """Normal values whose rows carry a factor 1e-3, 1 or 1e3, so that the order of a sum shows in its last bits."""
    x = rng.standard_normal(shape)
    scale = np.array([1e-3, 1.0, 1e3])[rng.integers(0, 3, shape[0])]
    return (x * scale.reshape((-1,) + (1,) * (len(shape) - 1))).astype(F)


class OpCase:
    """idx [m, nsample] into n rows; the first HOT_ROWS rows all point at destination 5 in column 0; a few entries are invalid."""

    def __init__(self, c, nsample, square, seed=11):
        rng = np.random.default_rng(seed + 100 * c + nsample)
        self.c, self.nsample = c, nsample
        self.m = HOT_ROWS + 37
        self.n = self.m if square else 40
        idx = rng.integers(0, self.n, (self.m, nsample)).astype(np.int32)
        idx[:HOT_ROWS, 0] = 5
        bad = rng.integers(HOT_ROWS, self.m, 6)
        idx[bad, rng.integers(0, nsample, 6)] = [-1, self.n, -7, self.n + 3, 2 ** 31 - 1, -2 ** 31]
        self.idx = idx
        self.name = "c%d_ns%d" % (c, nsample)
        self.inp = _mixed(rng, self.n, c)
        self.a = _mixed(rng, self.m, c)
        self.w1 = _mixed(rng, self.m, nsample)                     # interpolation weights
        self.position = _mixed(rng, self.m, nsample, c)
        self.g_rows = _mixed(rng, self.m, c)                       # gradient of an [m, c] output
        self.g_full = _mixed(rng, self.m, nsample, c)              # gradient of an [m, nsample, c] output
        self.w_cs = sorted({1, 4, c, 5})                           # 4 or 5 does not divide c (and may exceed it)
        self.rng = rng

    def weight(self, w_c):
        return _mixed(np.random.default_rng(7 * self.c + self.nsample + w_c), self.m, self.nsample, w_c)


CHANNELS, NSAMPLES = (1, 3, 32, 67), (1, 16, 33)


def op_cases(square):
    return [OpCase(c, ns, square) for c in CHANNELS for ns in NSAMPLES]


# ---- float64 bounds ----------------------------------------------------------------------------------------------------------------
def worst_ratio(got, exact, magnitude, terms):
    """max |got - exact| / ((terms + 2) * 2^-24 * magnitude), magnitude = the sum of the terms' absolute values (float64)."""
    bound = (np.asarray(terms, np.float64) + 2) * EPS * magnitude
    err = np.abs(got.astype(np.float64) - exact)
    ok = bound > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def gather_sum64(term, idx, n):
    start, pos = transpose(idx, n)
    out = np.zeros((n, term.shape[1]))
    np.add.at(out, np.repeat(np.arange(n), np.diff(start)), term[pos].astype(np.float64))
    return out, np.diff(start)

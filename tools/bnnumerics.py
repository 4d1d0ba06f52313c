#!/usr/bin/env python
"""Every BatchNorm kernel route of csrc/bn.hip and of the BatchNorm / statistics ops of csrc/layers.hip against an fp64 reference, at
the edges of the route selection (tests/test_gpu_bn_numerics.py, tests/test_bn_numerics_host.py).  Importable without a GPU.

  python tools/bnnumerics.py --numerics GROUP
      every probe of the group in this process (a fresh one: DODA_TRACE_BN and the grid switches are read once), one JSON line per
      traced launch and one per probe: status, traced route, per quantity [largest error, largest error / bound], sentinels, failures.
  python tools/bnnumerics.py --list
      the probe table with the launches each call must issue.
  python tools/bnnumerics.py --profile OUT.jsonl ...
      the result lines of --numerics runs as the table of profiles/r15_bn_numerics.txt.

THE PROBE TABLE (probes()).  One entry per call: entry point, dtype, m, c, statistics rows R or totals (one or two producers),
relu, add operand (none / dense / the right half of a [m, 2c] matrix), strides, environment group — and routes(p) gives the exact
launches (kernel, grid, workgroup) the call must issue, from Python copies of make_geo, n_blocks_for, apply_grid, fused_ok, plain_grid
and the op list's grids whose constants are PARSED from the sources (constants()).

THE REFERENCES are torch fp64 from the definition, never another kernel of the library.  Forward: batch mean, biased variance,
invstd = 1 / sqrt(var + eps), running statistics with momentum and the unbiased variance (m = 1: the variance as it is, bn_unbiased),
num_batches_tracked + 1.  Backward: dz = dy [yv > 0], dbeta = sum dz, dgamma = sum dz xhat, dx = gamma invstd (dz - mean(dz) - xhat
mean(dz xhat)) + add.  (torch refuses training mode at m = 1; the definition does not.)

THE BOUNDS, u = 2^-24 (one fp32 rounding):
* Sums accumulated in fp32 (standalone forms, bn_small_*, lay_stats): |S - S64| <= D u sum |addend|, D = the longest chain of fp32
  operations an addend passes through before the fp64 combine (chain() below, from the launch geometry):
      bn_small_*          ceil(m / 256) - 1 rows of a thread, 6 butterfly steps, 2 levels of the LDS fold
      bn_*_partial        ceil(m / (blocks rpb)) - 1 rows of a thread, rpb - 1 additions of the LDS column sum
      lay_stats           ceil(rows / (grid rpb)) - 1 rows of a thread, rpb - 1 additions of the LDS fold
  plus what the addend itself carries: sum (x - k): 1 (the shift); sum (x - k)^2: 3 (the shift enters squared, the product);
  sum dz: 0; sum dz xhat: 3 (xhat = (x - mean) invstd: 2, the product); sum x: 0; sum x^2: 1.  To first order
      d mean = dS1 / m + u |mean|,   d var = dS2 / m + 2 |mean - k| dS1 / m,   d invstd = invstd^3 d var / 2 + u invstd,
  and the running statistics take momentum times these (the variance times m / (m - 1)) plus their own rounding.
* Statistics handed in (rows, totals, op list): the reference finish is computed in fp64 from the very rows / totals of the call; the
  kernel adds them in fp64, so mean and invstd carry one fp32 rounding (2^-23 relative with the fp64 noise), the running statistics
  one more (3 u of |(1 - momentum) old| + |momentum new|); dgamma / dbeta one rounding; the coefficients mean(dz), mean(dz xhat) two.
* Elementwise y and dx: the reference is evaluated in fp64 from the fp32 per-channel vectors the call published (or was given); the
  bound is the count of fp32 roundings on the longest path times u times the magnitude of the terms:
      bn.hip and fp32 lay_bn (-ffp-contract=off, bn_fwd_elem / bn_bwd_elem):   y: 4 (|(x - mean) invstd gamma| + |beta|);
            dx: 7 (|a| (|dz| + |b| + |xhat d|) + |add|), a = gamma invstd, b = mean(dz), d = mean(dz xhat)
      bf16 lay_bn (pre_piece, fused multiply-adds on per-channel products):     y: 4 (|x sc| + |mean sc| + |beta|), sc = invstd gamma;
            dx: 8 (|a dz| + |a d invstd x| + |a d invstd mean| + |a b| + |add|)
      evaluation mode of lay_bn adds 3 (invstd = 1 / sqrtf(var + eps) in fp32); dx also takes |a| (db + |xhat| dd) for the error
  of the two coefficients.  A bf16 store adds half a bf16 ulp of the value: at most 2^-8 |value| (bf16 carries 8 significant bits;
  2^-9 |value| holds only for the upper half of a binade).
* ReLU mask in the backward: an element whose fp64 pre-activation lies within the forward bound of zero is undecided: skipped
  elementwise, its |dz| and |dz xhat| added as slack to the two sums.  Undecided elements are at most 1e-4 of a probe's elements
  (tests/test_bn_numerics_host.py asserts that from the reference alone).

INPUTS (make_inputs).  x with per-channel mean within 2 standard deviations of zero, non-zero, different per channel; gamma in
[0.5, 1.5], non-zero beta, running statistics that start at non-trivial values; channel 1 constant at 0.5 (every sum exact in every
form, variance exactly 0, invstd = 1 / sqrt(eps)); channel 2 with beta = -50 (mask all zero: dgamma = dbeta = 0, dx = add); rows and
totals built from the definition with all R rows / 8 slots distinct and non-zero; every output inside a sentinel-filled buffer (guard
rows on both sides, sentinel columns where the row stride exceeds c); the row after the last input row holds NaN."""
import json
import math
import os
import re
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "doda_amd", "csrc")
INSTANTIATIONS = os.path.join(ROOT, "tests", "data", "bn_instantiations.json")
STEMS = ("bn_", "lay_")      # tools/gatherroutes.py --instantiations --stem bn_ .../bn.o ; --stem lay_ .../layers.o

GROUPS = {"standalone": {}, "rows": {}, "totals": {"DODA_BN_TOT_GRID": "64"}, "layers": {"DODA_LAY_BN_GRID": "3"}}
SWITCHES = ("DODA_BN_TOT_GRID", "DODA_LAY_BN_GRID", "DODA_BN_FUSED_FINAL", "DODA_BN_FUSED_SMALL", "DODA_LAY_TUNED_ROWS", "DODA_PRE_FWD_ROWS",
            "DODA_PRE_BWD_ROWS")
U = 2.0 ** -24
EPS, MOMENTUM = 1e-4, 0.1
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -4
MAX_UNDECIDED = 1e-4
SENTINEL = 0x5A
PAD = 12345.0       # the unused doubles of a totals line


# ------------------------------------------------------------------------------------------------------ the code's own constants
def constants():
    """The thresholds of the route selection: the named constants of bn.hip, bn_totals.hpp and layers_plan.hpp, and three
    literals of bn.hip's launchers."""
    K = {}
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("bn.hip", "bn_totals.hpp", "layers_plan.hpp")}
    for text in src.values():
        for m in re.finditer(r"constexpr (?:int|long long) ((?:BN|LAY)_\w+) = ([0-9* ]+);", text):
            K[m[1]] = eval(m[2])
    one = lambda f, pat: int(re.search(pat, src[f])[1])
    K["ROWS_PER_LANE"] = one("bn.hip", r"div_up\(m, g\.rpb \* (\d+)\)")
    K["APPLY_CAP"] = one("bn.hip", r"TOT \? tot_grid_cap\(\) : (\d+), &fixed")
    K["TOT_GRID"] = one("bn.hip", r'env_ll\("DODA_BN_TOT_GRID", (\d+)\)')
    K["TUNED_ROWS"] = {4: K["LAY_TUNED_ROWS_F32"], 2: K["LAY_TUNED_ROWS_BF16"]}
    K["STATS_ROWS_PER_LANE"], K["STATS_GRID"] = K["LAY_STATS_ROWS_PER_LANE"], K["LAY_STATS_GRID"]
    return K


K = constants()
BLOCK = K["BN_BLOCK"]
TNAME = {2: "BF16", 4: "F32"}
B = lambda v: "true" if v else "false"


# ----------------------------------------------------------------------------------------- the launchers' geometry, in Python
def make_geo(c):
    nf = c // 4
    return nf, max(BLOCK // nf, 1)


def n_blocks_for(m, c):
    rpb = make_geo(c)[1]
    return min(max(-(-m // (rpb * K["ROWS_PER_LANE"])), 1), K["BN_MAX_BLOCKS"])


def plain_grid(n_frag, cap=None):
    return min(-(-n_frag // BLOCK), cap or K["APPLY_CAP"])


def apply_grid(n_frag, nf, W, aligned, cap):
    """(grid, FIXED) of an apply sweep (bn.hip apply_grid)."""
    if not aligned or nf % W or n_frag % W:
        return plain_grid(n_frag), False
    cols = nf // W
    grid = max(min(-(-(n_frag // W) // BLOCK), cap), 1)
    q = cols // math.gcd(cols, BLOCK)
    if grid < q:
        return plain_grid(n_frag), False
    return grid - grid % q, True


def fused_ok(rows, c, m):
    return m * c <= K["BN_FUSED_SMALL_ELEMS"] and c <= K["BN_FUSED_MAX_C"] and c // 4 <= BLOCK and rows * 2 * c * 4 <= K["BN_FUSED_MAX_PARTIAL_BYTES"]


def tot_cap(p):
    return min(max(int(GROUPS[p["group"]].get("DODA_BN_TOT_GRID", K["TOT_GRID"])), 64), 4096)


def lay_bn_grid(p):
    ppr = p["c"] // (16 // p["esz"])
    rpb = 256 // ppr
    return max(min(-(-p["m"] // rpb), int(GROUPS[p["group"]].get("DODA_LAY_BN_GRID", K["LAY_BN_GRID"]))), 1), rpb


def lay_stats_grid(rows, c):
    nf, rpb = make_geo(c)
    return max(min(-(-rows // (rpb * K["STATS_ROWS_PER_LANE"])), K["STATS_GRID"]), 1), rpb


def add_aligned(p):
    """Is the second gradient 16-byte aligned with a row stride of whole 16-byte accesses (launch_bwd_apply)?  Buffers are; the
    right half of a [m, 2c] matrix starts c elements in."""
    W = 2 if p["esz"] == 2 else 1
    return p["add"] != "slice" or ((p["c"] * p["esz"]) % 16 == 0 and (2 * p["c"]) % (4 * W) == 0)


def _apply(p, bwd, tot):
    nf, W = p["c"] // 4, 2 if p["esz"] == 2 else 1
    grid, fixed = apply_grid(p["m"] * nf, nf, W, add_aligned(p) if bwd else True, tot_cap(p) if tot else K["APPLY_CAP"])
    return ("%s<%s, %s, %s>" % ("bn_bwd_apply" if bwd else "bn_apply", TNAME[p["esz"]], B(fixed), B(tot)), grid, BLOCK)


def routes(p):
    """The launches (kernel, grid, workgroup) the call of probe p must issue; none where it returns an error."""
    e, m, c, T = p["entry"], p["m"], p["c"], TNAME[p["esz"]]
    if p["status"]:
        return []
    fused = min(-(-m * (c // 4) // BLOCK), K["BN_FUSED_BLOCKS"])
    if e == "fwd":
        if not p["training"]:
            return [_apply(p, 0, 0)]
        if m <= K["BN_SMALL_ROWS"]:
            return [("bn_small_fwd<%s>" % T, c // 4, BLOCK)]
        return [("bn_stats_partial<%s>" % T, n_blocks_for(m, c), BLOCK), ("bn_stats_final<%s>" % T, c, 64), _apply(p, 0, 0)]
    if e == "bwd":
        if m <= K["BN_SMALL_ROWS"]:
            return [("bn_small_bwd<%s>" % T, c // 4, BLOCK)]
        return [("bn_bwd_partial<%s>" % T, n_blocks_for(m, c), BLOCK), ("bn_bwd_final", c, 64), _apply(p, 1, 0)]
    if e == "fwd_final":
        return [("bn_fwd_final_stats", c // 4, BLOCK)]
    if e == "apply":
        return [_apply(p, 0, 0)]
    if e == "fwd_stats":
        return [("bn_fused_fwd<%s>" % T, fused, BLOCK)] if fused_ok(p["R"], c, m) else [("bn_fwd_final_stats", c // 4, BLOCK), _apply(p, 0, 0)]
    if e == "bwd_stats":
        if p["add"] != "slice" and fused_ok(p["R"], c, m):
            return [("bn_fused_bwd<%s>" % T, fused, BLOCK)]
        return [("bn_bwd_final_stats", c // 4, BLOCK), _apply(p, 1, 0)]
    if e == "fwd_totals":
        return [_apply(p, 0, 1)]
    if e == "bwd_totals":
        return [_apply(p, 1, 1)]
    if e == "lay_stats":
        return [("lay_stats<%d>" % p["esz"], lay_stats_grid(hi - lo, c)[0], 256) for lo, hi in p["ranges"]]
    tuned = m >= K["TUNED_ROWS"][p["esz"]] and not p["y_pad"] and not p["split"] and not p["accum"]
    if e == "lay_fwd":
        return [_apply(p, 0, 1)] if tuned and p["training"] else [("lay_bn<%d, 1>" % p["esz"], lay_bn_grid(p)[0], 256)]
    if e == "lay_bwd":
        return [_apply(p, 1, 1)] if tuned else [("lay_bn<%d, %d>" % (p["esz"], 3 if p["add"] else 2), lay_bn_grid(p)[0], 256)]
    raise ValueError(e)


def chain(name, grid, p):
    """fp32 additions on the longest path of an addend of the kernel's sums (the docstring's table)."""
    m, c = p["m"], p["c"]
    if name.startswith("bn_small"):
        return -(-m // BLOCK) - 1 + 6 + 2
    if name.startswith(("bn_stats_partial", "bn_bwd_partial")):
        rpb = make_geo(c)[1]
        return -(-m // (grid * rpb)) - 1 + rpb - 1
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------------------------- the probe table
def probe(group, entry, esz, m, c, **kw):
    p = dict(group=group, entry=entry, esz=esz, m=m, c=c, relu=1, training=1, add=None, R=0, c_a=0, accum=0, split=0, x_slice=0, y_pad=0,
             status=OK, ranges=None)
    p.update(kw)
    p["form"] = "fma" if entry in ("lay_fwd", "lay_bwd") and esz == 2 and not routes(dict(p, form=""))[0][0].startswith("bn_") else "seq"
    p["id"] = "%s.%s.%s.m%d.c%d" % (group, entry, TNAME[esz].lower(), m, c) + "".join(
        ".%s%s" % (k, p[k] if not isinstance(p[k], str) else "=" + p[k]) for k in ("R", "c_a", "add", "accum", "split", "x_slice", "y_pad") if p[k]) + (
        "" if p["relu"] else ".norelu") + ("" if p["training"] else ".eval") + (".ranges" if p["ranges"] and len(p["ranges"]) > 1 else "")
    return p


ADDS = (None, "dense", "slice")
REDUCTION_R = (1, 3, 4, 5, 255, 256, 257, 768, 769, 1027)
FUSED_R = {64: (1, 15, 16, 17, 63, 64, 65, 320), 16: (1, 255, 256, 257)}


def probes(group=None):
    ps = []
    small, tun = K["BN_SMALL_ROWS"], K["TUNED_ROWS"]
    fused_m = K["BN_FUSED_SMALL_ELEMS"] // 64
    fused_r = K["BN_FUSED_MAX_PARTIAL_BYTES"] // (2 * 64 * 4)
    for esz in (2, 4):
        # ---- standalone: doda_bn_relu_fwd / _bwd / _bwd_add
        shapes = [(m, c) for m in (1, 37, 255, 256, 257, small - 1, small, small + 1, 3 * small + 1) for c in (16, 48)]
        shapes += [(m, c) for c in (4, 20, 1024) for m in (37, small + 1)]
        for m, c in shapes:
            for relu in (1, 0):
                ps.append(probe("standalone", "fwd", esz, m, c, relu=relu))
                ps += [probe("standalone", "bwd", esz, m, c, relu=relu, add=a) for a in ADDS]
            if m in (37, small + 1) and c in (16, 48):
                ps.append(probe("standalone", "fwd", esz, m, c, training=0))
        # ---- statistics rows: doda_bn_fwd_final (no element type), doda_bn_relu_fwd_stats / _apply / _bwd_stats
        if esz == 2:
            ps += [probe("rows", "fwd_final", 2, 37, 16, R=R) for R in REDUCTION_R]
        for R in REDUCTION_R:       # 68 channels: above BN_FUSED_MAX_C, so the reduction is its own launch
            ps += [probe("rows", "fwd_stats", esz, 37, K["BN_FUSED_MAX_C"] + 4, R=R), probe("rows", "bwd_stats", esz, 37, K["BN_FUSED_MAX_C"] + 4, R=R)]
        for c, Rs in FUSED_R.items():
            for R in Rs:
                ps += [probe("rows", "fwd_stats", esz, 37, c, R=R), probe("rows", "bwd_stats", esz, 37, c, R=R, add="dense" if R % 2 else None)]
        ps += [probe("rows", e, esz, 37, K["BN_FUSED_MAX_C"], R=fused_r + 1) for e in ("fwd_stats", "bwd_stats")]      # (fused_r itself: FUSED_R)
        for m in (fused_m, fused_m + 1):
            ps += [probe("rows", "fwd_stats", esz, m, 64, R=5), probe("rows", "bwd_stats", esz, m, 64, R=5, add="dense")]
        ps += [probe("rows", "fwd_stats", esz, 37, 64, R=5), probe("rows", "bwd_stats", esz, 37, 64, R=5),
               probe("rows", "bwd_stats", esz, 37, 64, R=5, add="slice"), probe("rows", "bwd_stats", esz, 37, 16, R=5, add="slice"),
               probe("rows", "fwd_stats", esz, 37, 16, R=5, relu=0), probe("rows", "bwd_stats", esz, 37, 16, R=5, relu=0),
               probe("rows", "bwd_stats", esz, 37, 68, R=5, add="slice"), probe("rows", "bwd_stats", esz, 37, 68, R=5, add="dense")]
        ps += [probe("rows", e, esz, 37, 112, R=5) for e in ("fwd_stats", "bwd_stats")]       # fp32: no FIXED grid
        ps += [probe("rows", "apply", esz, m, c) for m, c in ((37, 16), (small + 1, 48), (37, 112), (37, 20))]
        # ---- fp64 totals: doda_bn_relu_fwd_totals / _bwd_totals
        tshapes = [(m, c) for c in (8, 16, 48, 20, 256) for m in (1, 37, small + 1)] + [(2 * small + 1, 16)]
        for m, c in tshapes:
            ps.append(probe("totals", "fwd_totals", esz, m, c))
            ps += [probe("totals", "bwd_totals", esz, m, c, add=a) for a in ADDS]
            if m == 37:
                ps += [probe("totals", "fwd_totals", esz, m, c, c_a=ca) for ca in sorted({4, c // 2, c - 4}) if 0 < ca < c and ca % 4 == 0]
        ps += [probe("totals", "fwd_totals", esz, 37, 16, relu=0), probe("totals", "bwd_totals", esz, 37, 16, relu=0),
               probe("totals", "fwd_totals", esz, 37, K["BN_TOT_MAX_C"] + 4, status=ERR_UNSUPPORTED),
               probe("totals", "bwd_totals", esz, 37, K["BN_TOT_MAX_C"] + 4, status=ERR_UNSUPPORTED),
               probe("totals", "fwd_totals", esz, 37, 20, c_a=10, status=ERR_INVALID)]
        # ---- the op list: doda_layers_run
        for rows in (1, 37, small + 1):
            for c in (8, 16, 48, 256, 1024):
                ps += [probe("layers", "lay_stats", esz, rows, c, x_slice=s, ranges=[(0, rows)]) for s in (0, 1)]
        ps.append(probe("layers", "lay_stats", esz, 337, 16, ranges=[(0, 37), (37, 337)]))
        for rows in (1, 37, 300):
            for c in (16, 48, 256):
                for y_pad in (0, 16):
                    ps += [probe("layers", "lay_fwd", esz, rows, c, y_pad=y_pad), probe("layers", "lay_fwd", esz, rows, c, y_pad=y_pad, c_a=c // 2),
                           probe("layers", "lay_fwd", esz, rows, c, y_pad=y_pad, training=0)]
                for add in (None, "dense"):
                    ps += [probe("layers", "lay_bwd", esz, rows, c, add=add), probe("layers", "lay_bwd", esz, rows, c, add=add, split=c // 2),
                           probe("layers", "lay_bwd", esz, rows, c, add=add, accum=1)]
        ps += [probe("layers", "lay_fwd", esz, 37, 16, relu=0), probe("layers", "lay_bwd", esz, 37, 16, relu=0),
               probe("layers", "lay_bwd", esz, 37, 16, add="slice")]
        for rows in (tun[esz] - 1, tun[esz]):       # the hand-over of a dense op to the sweeps of bn.hip
            ps += [probe("layers", "lay_fwd", esz, rows, 16), probe("layers", "lay_bwd", esz, rows, 16), probe("layers", "lay_bwd", esz, rows, 16, add="dense")]
    assert len({p["id"] for p in ps}) == len(ps)
    return [p for p in ps if group in (None, p["group"])]


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _dtype(esz):
    import torch
    return torch.float32 if esz == 4 else torch.bfloat16


def distinct_ints(R, total):
    """R distinct non-zero integers that add up to `total` (R = 1: the total itself)."""
    if R == 1:
        return [total]
    n = list(range(1, R))
    last = total - sum(n)
    if last == 0 or 1 <= last <= R - 1:
        n[0] -= R
        last += R
    return n + [last]


def spread(T, R, g, exact=None):
    """[R, c] fp64 rows that add up to T [c] (distinct positive random weights); `exact`: {channel: (total in units, unit)} — those
    channels hold distinct non-zero integer multiples of the unit instead, so that they add up EXACTLY in any order and precision."""
    import torch
    w = 0.5 + torch.rand(R, T.numel(), generator=g, dtype=torch.float64)
    out = T.cpu() * (w / w.sum(0))
    for ch, (total, unit) in (exact or {}).items():
        out[:, ch] = torch.tensor(distinct_ints(R, total), dtype=torch.float64) * unit
    return out


def totals_of(s1, s2):
    """[R = 8 slots, c] sums -> the library's totals layout [8, 2, c / 4, 16], unused doubles = PAD."""
    import torch
    c = s1.shape[1]
    t = torch.full((8, 2, c // 4, 16), PAD, dtype=torch.float64)
    t[:, 0, :, :4] = s1.view(8, c // 4, 4)
    t[:, 1, :, :4] = s2.view(8, c // 4, 4)
    return t


def padded(v, dt, ld=None, off=0):
    """(buffer, view): the [m, c] matrix v in dtype dt with row stride ld at column off of a buffer whose row m holds NaN."""
    import torch
    m, c = v.shape
    buf = torch.full((m + 1, ld or c), float("nan"), dtype=dt)
    buf[:m] = 0
    buf[:m, off:off + c] = v.to(dt)
    return buf


_drawn = {}


def _draw(m, c, esz):
    """The random operands of a shape, drawn on the CPU from a generator seeded by the shape (kept for the probes that follow with
    the same shape)."""
    import torch
    if (m, c, esz) in _drawn:
        return _drawn[(m, c, esz)]
    g = torch.Generator().manual_seed(zlib.crc32(("%d %d %d" % (m, c, esz)).encode()))
    sd = 0.5 + 1.5 * torch.rand(c, generator=g, dtype=torch.float64)
    mu = ((torch.arange(c, dtype=torch.float64) + 0.5) / c * 2 - 1) * 1.8 * sd
    x = mu + sd * torch.randn(m, c, generator=g, dtype=torch.float64)
    x[:, 1] = 0.5
    dy = torch.randn(m, c, generator=g, dtype=torch.float64)
    add = torch.randn(m, c, generator=g, dtype=torch.float64)
    gamma = (0.5 + torch.rand(c, generator=g)).float()
    beta = ((0.1 + 0.5 * torch.rand(c, generator=g)) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1)).float()
    beta[2] = -50.0
    _drawn.clear()
    _drawn[(m, c, esz)] = (x, dy, add, gamma, beta, (0.3 * torch.randn(c, generator=g)).float(), (0.5 + torch.rand(c, generator=g)).float(),
                           torch.randn(c, generator=g).float(), torch.randn(c, generator=g).float())
    return _drawn[(m, c, esz)]


def make_inputs(p, dev):
    import torch
    m, c, esz = p["m"], p["c"], p["esz"]
    dt = _dtype(esz)
    x, dy, add, gamma, beta, rm0, rv0, dg0, db0 = _draw(m, c, esz)
    g = torch.Generator().manual_seed(zlib.crc32(("%d %d %d weights" % (m, c, esz)).encode()))
    I = dict(gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, nbt0=7, dg0=dg0, db0=db0)
    xs = p["x_slice"]
    I["xbuf"] = padded(x, dt, 2 * c if xs else c, c if xs else 0)
    I["dybuf"] = padded(dy, dt)
    if p["add"]:
        sl = p["add"] == "slice"
        I["addbuf"] = padded(add, dt, 2 * c if sl else c, c if sl else 0)
    I = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in I.items()}
    I["x"] = I["xbuf"][:m, c:] if xs else I["xbuf"][:m]
    I["dy"] = I["dybuf"][:m]
    I["add"] = None if not p["add"] else I["addbuf"][:m, c:] if p["add"] == "slice" else I["addbuf"][:m]
    # the definition's statistics of the stored x (fp64) and what a backward / an apply is GIVEN: their fp32 roundings
    x64 = I["x"].double()
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    I["eps64"], I["mom64"] = eps, float(torch.tensor(MOMENTUM, dtype=torch.float32))
    if p["entry"] in ("apply",) or (p["entry"] == "fwd" and not p["training"]):       # evaluation: the running statistics
        I["mean_in"], I["invstd_in"] = I["rm0"], (1.0 / torch.sqrt(I["rv0"].double() + eps)).float()
    else:
        I["mean_in"], I["invstd_in"] = mean.float(), (1.0 / torch.sqrt(var + eps)).float()
    bwd = p["entry"] in ("bwd_stats", "bwd_totals", "lay_bwd")
    if p["entry"] in ("fwd_final", "fwd_stats", "fwd_totals", "lay_fwd") or bwd:
        R = p["R"] or 8
        if bwd:
            D = bwd_definition(p, I)
            T1, T2 = D["S1"], D["S2"]
            ex1 = {2: (0, 2.0 ** -6)} if p["relu"] else {}
            ex2 = {**ex1, 1: (0, 2.0 ** -6)}
        else:
            T1, T2 = x64.sum(0), (x64 * x64).sum(0)
            ex1, ex2 = {1: (m, 0.5)}, {1: (m, 0.25)}
        s1, s2 = spread(T1, R, g, ex1), spread(T2, R, g, ex2)
        if p["R"]:
            I["rows"] = torch.stack([s1, s2], 1).float().to(dev)        # [R, 2, c]
        elif p["c_a"] and not p["status"]:
            ca = p["c_a"]
            I["ta"], I["tb"] = totals_of(s1[:, :ca], s2[:, :ca]).to(dev), totals_of(s1[:, ca:], s2[:, ca:]).to(dev)
        else:
            I["ta"], I["tb"] = totals_of(s1, s2).to(dev), None
            if p["c_a"]:        # (an error probe: the call must refuse before it reads anything)
                I["tb"] = I["ta"]
    return I


def handed_sums(p, I):
    """[2, c] fp64: the sums of the rows / totals the call receives, or None."""
    import torch
    if "rows" in I:
        return I["rows"].double().sum(0)
    if "ta" in I:
        s = [t[:, :, :, :4].sum(0).reshape(2, -1) for t in (I["ta"], I["tb"]) if t is not None and not p["status"]]
        return torch.cat(s, 1) if s else None
    return None


# ----------------------------------------------------------------------------------------------- fp64 references and their bounds
def fwd_elem(form, x, mu, is_, ga, be, relu, extra=0):
    """(fp64 y before the store, bound of the fp32 evaluation, fp64 pre-activation)."""
    pre = (x - mu) * is_ * ga + be
    if form == "seq":
        bound = (4 + extra) * U * (((x - mu) * is_ * ga).abs() + be.abs())
    else:
        sc = is_ * ga
        bound = (4 + extra) * U * ((x * sc).abs() + (mu * sc).abs() + be.abs())
    return (pre.clamp(min=0) if relu else pre), bound, pre


def store_bound(v, e, esz):
    """e plus, for a bf16 store, half a bf16 ulp of a value as large as |v| + e."""
    import torch
    if esz == 4:
        return e
    a = v.abs() + e
    ex = torch.frexp(a)[1]
    return e + torch.where(a > 0, torch.ldexp(torch.ones_like(a), ex - 9), torch.zeros_like(a))


def bwd_definition(p, I, mean=None, invstd=None):
    """The backward's sums from the definition, over the vectors the call is given: masked dz, xhat, S1 = sum dz, S2 = sum dz xhat, the
    sums of absolute values, the undecided elements (forward bound of the form that evaluates the mask) and their slack."""
    import torch
    x, dy = I["x"].double(), I["dy"].double()
    mu, is_ = (I["mean_in"] if mean is None else mean).double(), (I["invstd_in"] if invstd is None else invstd).double()
    ga, be = I["gamma"].double(), I["beta"].double()
    xh = (x - mu) * is_
    und = torch.zeros_like(x, dtype=torch.bool)
    dz = dy
    if p["relu"]:
        _, fb, pre = fwd_elem(p["form"], x, mu, is_, ga, be, 0)
        und = pre.abs() <= fb
        dz = dy * (pre > 0)
    return dict(dz=dz, xh=xh, und=und, S1=dz.sum(0), S2=(dz * xh).sum(0), A1=dz.abs().sum(0), A2=(dz * xh).abs().sum(0),
                slack1=(dy.abs() * und).sum(0), slack2=((dy * xh).abs() * und).sum(0), undecided=float(und.double().mean()))


def bwd_elem(form, x, dz, mu, is_, ga, b, d, add, db, dd):
    a = ga * is_
    xh = (x - mu) * is_
    ref = a * (dz - b - xh * d) + add
    if form == "seq":
        bound = 7 * U * (a.abs() * (dz.abs() + b.abs() + (xh * d).abs()) + add.abs()) + a.abs() * (db + xh.abs() * dd)
    else:
        bound = 8 * U * ((a * dz).abs() + (a * d * is_ * x).abs() + (a * d * is_ * mu).abs() + (a * b).abs() + add.abs()) + \
            a.abs() * (db + ((is_ * x).abs() + (is_ * mu).abs()) * dd)
    return ref, bound


def reference(p, I, O):
    """{quantity: (fp64 reference, bound, mask of the elements that count or None)} for the outputs O of the call (the elementwise
    references are evaluated from the vectors O publishes)."""
    import torch
    e, m, c, esz = p["entry"], p["m"], p["c"], p["esz"]
    x = I["x"].double()
    ga, be, eps, mom = I["gamma"].double(), I["beta"].double(), I["eps64"], I["mom64"]
    Q = {}
    rt = routes(p)
    if e == "lay_stats":
        ref = torch.zeros(2, c, dtype=torch.float64, device=x.device)
        bound = torch.zeros_like(ref)
        for (lo, hi), (_, grid, _) in zip(p["ranges"], rt):
            rpb = make_geo(c)[1]
            D = -(-(hi - lo) // (grid * rpb)) - 1 + rpb - 1
            v = x[lo:hi]
            ref += torch.stack([v.sum(0), (v * v).sum(0)])
            bound += U * torch.stack([D * v.abs().sum(0), (D + 1) * (v * v).sum(0)])
        Q["totals"] = (ref, bound + 2.0 ** -50 * ref.abs(), None)
        return Q
    fwd = e in ("fwd", "fwd_final", "fwd_stats", "apply", "fwd_totals", "lay_fwd")
    given = e == "apply" or not p["training"]
    if fwd and not given:
        S = handed_sums(p, I)
        if S is None:       # standalone: fp32 sums of x - k, k = the first row
            name, grid, _ = rt[0]
            D = chain(name, grid, p)
            k = x[0]
            v = x - k
            dS1, dS2 = (D + 1) * U * v.abs().sum(0), (D + 3) * U * (v * v).sum(0)
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
            inv = 1.0 / torch.sqrt(var + eps)
            dvar = dS2 / m + 2 * (mean - k).abs() * dS1 / m + (dS1 / m) ** 2
            dmean, dinv = dS1 / m + U * mean.abs(), 0.5 * inv ** 3 * dvar + U * inv
            unb = var * m / (m - 1) if m > 1 else var
            rm, rv = (1 - mom) * I["rm0"].double() + mom * mean, (1 - mom) * I["rv0"].double() + mom * unb
            drm = mom * dS1 / m + U * rm.abs()
            drv = mom * (m / (m - 1) if m > 1 else 1.0) * dvar + U * rv.abs()
        else:
            mean = S[0] / m
            var = (S[1] / m - mean * mean).clamp(min=0)
            inv = 1.0 / torch.sqrt(var + eps)
            unb = var * m / (m - 1) if m > 1 else var
            rm, rv = (1 - mom) * I["rm0"].double() + mom * mean, (1 - mom) * I["rv0"].double() + mom * unb
            dmean, dinv = 2 * U * mean.abs(), 2 * U * inv
            drm = 3 * U * (((1 - mom) * I["rm0"].double()).abs() + (mom * mean).abs())
            drv = 3 * U * (((1 - mom) * I["rv0"].double()).abs() + (mom * unb).abs())
        Q.update(mean=(mean, dmean, None), invstd=(inv, dinv, None), rm=(rm, drm, None), rv=(rv, drv, None))
        Q["nbt"] = (torch.tensor([float(I["nbt0"] + 1)], dtype=torch.float64, device=x.device), torch.zeros(1, dtype=torch.float64, device=x.device), None)
    if fwd and e != "fwd_final":
        extra = 0
        if given and e == "lay_fwd":        # evaluation mode of the op list: invstd = 1 / sqrtf(running_var + eps) inside the kernel
            mu, is_, extra = I["rm0"].double(), 1.0 / torch.sqrt(I["rv0"].double() + eps), 3
        elif given:
            mu, is_ = I["mean_in"].double(), I["invstd_in"].double()
        elif "mean" in O:
            mu, is_ = O["mean"].double(), O["invstd"].double()
        else:
            mu = None       # (nothing published yet: ideal_outputs' first pass)
        if mu is not None:
            y, fb, _ = fwd_elem(p["form"], x, mu, is_, ga, be, p["relu"], extra)
            Q["y"] = (y, store_bound(y, fb, esz), None)
    if not fwd:
        D = bwd_definition(p, I)
        S = handed_sums(p, I)
        if S is None:       # standalone: fp32 sums of dz and dz xhat
            name, grid, _ = rt[0]
            n = chain(name, grid, p)
            cast = 0.0 if name.startswith("bn_small") else U
            S1, S2 = D["S1"], D["S2"]
            dS1, dS2 = n * U * D["A1"] + D["slack1"], (n + 3) * U * D["A2"] + D["slack2"]
            ddb, ddg = dS1 + cast * S1.abs(), dS2 + cast * S2.abs()
        else:               # handed in: the mask never enters the sums
            S1, S2 = S[0], S[1]
            dS1 = dS2 = torch.zeros_like(S1)
            ddb, ddg = U * S1.abs() * (1 + 2.0 ** -20), U * S2.abs() * (1 + 2.0 ** -20)
        base_b, base_g = (I["db0"].double(), I["dg0"].double()) if p["accum"] else (0.0, 0.0)
        if p["accum"]:      # one fp32 addition onto the base
            ddb, ddg = ddb + U * (base_b + S1).abs(), ddg + U * (base_g + S2).abs()
        Q["dbeta"], Q["dgamma"] = (base_b + S1, ddb, None), (base_g + S2, ddg, None)
        b, d = S1 / m, S2 / m
        add = I["add"].double() if I["add"] is not None else torch.zeros_like(x)
        dx, eb = bwd_elem(p["form"], x, D["dz"], I["mean_in"].double(), I["invstd_in"].double(), ga, b, d, add, dS1 / m + 2 * U * b.abs(),
                          dS2 / m + 2 * U * d.abs())
        Q["dx"] = (dx, store_bound(dx, eb, esz), ~D["und"])
        Q["undecided"] = D["undecided"]
    return Q


def check(p, I, O):
    """(err, fails) of the outputs O of probe p: err[quantity] = [largest error, largest error / bound]."""
    import torch
    Q = reference(p, I, O)
    err, fails = {}, []
    und = Q.pop("undecided", 0.0)
    if und > MAX_UNDECIDED:
        fails.append("undecided mask elements %.3g > %.3g" % (und, MAX_UNDECIDED))
    for name, (ref, bound, mask) in Q.items():
        got = O[name].double().reshape(ref.shape)
        diff = (got - ref).abs()
        if mask is not None:
            diff = torch.where(mask, diff, torch.zeros_like(diff))
        bad = ~(diff <= bound)          # (a NaN is bad)
        ratio = torch.where(diff > 0, diff / bound.clamp(min=1e-300), torch.zeros_like(diff))
        ratio = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), ratio)
        err[name] = [float(torch.nan_to_num(diff, nan=float("inf")).max()) if diff.numel() else 0.0, float(ratio.max()) if diff.numel() else 0.0]
        if bool(bad.any()):
            fails.append("%s: %d of %d outside their bound, worst x %.3g" % (name, int(bad.sum()), bad.numel(), err[name][1]))
    for name, ok in O.get("guards", {}).items():
        if not ok:
            fails.append("sentinel overwritten around " + name)
    return err, fails


# ----------------------------------------------------------------------------- outputs without a GPU: the rounded reference, numpy fp32
def ideal_outputs(p, I):
    """The reference's own outputs rounded once to the types the call writes (what a perfect kernel returns)."""
    import torch
    O = {}
    Q = reference(p, I, O)
    for k in ("mean", "invstd", "rm", "rv", "dbeta", "dgamma", "totals"):
        if k in Q:
            O[k] = Q[k][0].float() if k != "totals" else Q[k][0]
    if "nbt" in Q:
        O["nbt"] = Q["nbt"][0]
    Q = reference(p, I, O)      # (y from the published fp32 vectors)
    for k in ("y", "dx"):
        if k in Q:
            O[k] = Q[k][0].to(_dtype(p["esz"]))
    return O


def emu_sum(v, name, grid, c):
    """The column sums of v [rows, c] (numpy float32) in the order of kernel `name` on `grid` workgroups, as float64: bn_small_*: a
    thread's rows one after the other, then a tree over the 256 threads; the partial-sum kernels and lay_stats: a thread's rows, the
    row lanes of a workgroup one after the other, the workgroups in float64."""
    import numpy as np
    lanes = BLOCK if name.startswith("bn_small") else grid * make_geo(c)[1]
    n = -(-v.shape[0] // lanes)
    a = np.zeros((n * lanes, v.shape[1]), np.float32)
    a[:v.shape[0]] = v
    a = a.reshape(n, lanes, -1)
    acc = a[0].copy()
    for i in range(1, n):
        acc = acc + a[i]
    if name.startswith("bn_small"):
        while acc.shape[0] > 1:
            acc = acc[:acc.shape[0] // 2] + acc[acc.shape[0] // 2:]
        return acc[0].astype(np.float64)
    acc = acc.reshape(grid, lanes // grid, -1)
    col = acc[:, 0].copy()
    for r in range(1, acc.shape[1]):
        col = col + acc[:, r]
    return col.astype(np.float64).sum(0)


def emulated_outputs(p, I):
    """The kernels' expressions in numpy float32 (sums: emu_sum; a fused multiply-add: the product and sum in float64, rounded
    once), stored in the call's types: what the library computes."""
    import numpy as np
    import torch
    f = np.float32
    n32 = lambda t: t.float().cpu().numpy().astype(f)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    e, m, c = p["entry"], p["m"], p["c"]
    x, ga, be = n32(I["x"]), n32(I["gamma"]), n32(I["beta"])
    O = {}
    S = handed_sums(p, I)
    rt = routes(p)
    fwd = e in ("fwd", "fwd_final", "fwd_stats", "apply", "fwd_totals", "lay_fwd")
    if fwd:
        if e == "apply" or not p["training"]:
            mu, is_ = n32(I["mean_in"]), n32(I["invstd_in"])
            if e == "lay_fwd":
                mu, is_ = n32(I["rm0"]), f(1.0) / np.sqrt(n32(I["rv0"]) + f(I["eps64"]))
        else:
            if S is None:
                k = x[0]
                v = x - k
                s1, s2 = emu_sum(v, rt[0][0], rt[0][1], c), emu_sum(v * v, rt[0][0], rt[0][1], c)
                shift = k.astype(np.float64)
            else:
                s1, s2, shift = S[0].cpu().numpy(), S[1].cpu().numpy(), 0.0
            d = s1 / m
            var = np.maximum(s2 / m - d * d, 0.0)
            mean = shift + d
            mu, is_ = mean.astype(f), (1.0 / np.sqrt(var + I["eps64"])).astype(f)
            unb = var * m / (m - 1) if m > 1 else var
            O.update(mean=mu, invstd=is_, rm=((1.0 - I["mom64"]) * n32(I["rm0"]).astype(np.float64) + I["mom64"] * mean).astype(f),
                     rv=((1.0 - I["mom64"]) * n32(I["rv0"]).astype(np.float64) + I["mom64"] * unb).astype(f), nbt=np.array([I["nbt0"] + 1.0]))
        if e != "fwd_final":
            if p["form"] == "seq":
                y = (x - mu) * is_ * ga + be
            else:
                sc = is_ * ga
                y = fma(x, sc, be - mu * sc)
            O["y"] = np.maximum(y, f(0)) if p["relu"] else y
    elif e != "lay_stats":
        dz, mu, is_ = n32(I["dy"]), n32(I["mean_in"]), n32(I["invstd_in"])
        xh = (x - mu) * is_
        if p["form"] == "seq":
            yv = xh * ga + be
        else:
            G = is_ * ga
            yv = fma(x, G, be - mu * G)
        if p["relu"]:
            dz = np.where(yv > 0, dz, f(0))
        if S is None:
            s1, s2 = emu_sum(dz, rt[0][0], rt[0][1], c), emu_sum(dz * xh, rt[0][0], rt[0][1], c)
        else:
            s1, s2 = S[0].cpu().numpy(), S[1].cpu().numpy()
        O["dbeta"], O["dgamma"] = s1.astype(f), s2.astype(f)
        if p["accum"]:
            O["dbeta"], O["dgamma"] = n32(I["db0"]) + O["dbeta"], n32(I["dg0"]) + O["dgamma"]
        a, b, d = ga * is_, (s1 / m).astype(f), (s2 / m).astype(f)
        if p["form"] == "seq":
            dx = a * (dz - b - xh * d)
        else:
            Cc, E = a * d * is_, a * (d * is_ * mu - b)
            dx = fma(a, dz, fma(-Cc, x, E))
        if I["add"] is not None:
            dx = dx + n32(I["add"])
        O["dx"] = dx
    else:
        O["totals"] = sum(np.stack([emu_sum(x[lo:hi], r[0], r[1], c), emu_sum(x[lo:hi] * x[lo:hi], r[0], r[1], c)])
                          for (lo, hi), r in zip(p["ranges"], rt))
    out = {}
    for k, v in O.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        out[k] = t.to(_dtype(p["esz"])) if k in ("y", "dx") else t
    return out


# --------------------------------------------------------------------------------------------------------------- the device run
class Guarded:
    """An output [rows, cols] with row stride ld inside a sentinel-filled buffer: four guard rows on both sides."""
    G = 4

    def __init__(self, rows, cols, dt, dev, ld=None, init=None):
        import torch
        self.rows, self.cols, ld = rows, cols, ld or cols
        self.esz = torch.empty(0, dtype=dt).element_size()
        self.buf = torch.full(((rows + 2 * self.G) * ld * self.esz,), SENTINEL, dtype=torch.uint8, device=dev)
        self.full = self.buf.view(dt).view(rows + 2 * self.G, ld)
        self.inner = self.full[self.G:self.G + rows, :cols]
        if init is not None:
            self.inner.copy_(init.view(rows, cols))

    def ptr(self):
        return self.inner.data_ptr()

    def intact(self):
        b = self.buf.clone().view(self.rows + 2 * self.G, -1)
        b[self.G:self.G + self.rows, :self.cols * self.esz] = SENTINEL
        return bool((b == SENTINEL).all())


def run_probe(p, I, L, dev):
    """The call of probe p -> its outputs O (tensors, `status`, `guards`)."""
    import torch
    from doda_amd import ops
    e, m, c, esz = p["entry"], p["m"], p["c"], p["esz"]
    dt, f32 = _dtype(esz), torch.float32
    vec = lambda init=None: Guarded(1, c, f32, dev, c + 16, init)
    W = dict(mean=vec(), invstd=vec(), rm=vec(I["rm0"]), rv=vec(I["rv0"]), dgamma=vec(I["dg0"] if p["accum"] else None),
             dbeta=vec(I["db0"] if p["accum"] else None), y=Guarded(m, c, dt, dev, c + p["y_pad"]), coef=Guarded(3, c, f32, dev))
    nbt = torch.tensor([-77, I["nbt0"], -77], dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    x, dy, add = I["x"], I["dy"], I["add"]
    add_ld = add.stride(0) if add is not None else 0
    ga, be, relu = ptr(I["gamma"]), ptr(I["beta"]), p["relu"]
    ws = torch.empty(int(L.doda_bn_workspace_bytes(m, c)), dtype=torch.uint8, device=dev)
    out = []
    if e == "fwd":
        tr = p["training"]
        mean, inv = (W["mean"].ptr(), W["invstd"].ptr()) if tr else (ptr(I["mean_in"]), ptr(I["invstd_in"]))
        st = L.doda_bn_relu_fwd(ptr(x), m, c, esz, EPS, MOMENTUM, ga, be, W["rm"].ptr() if tr else None, W["rv"].ptr() if tr else None,
                                nbt[1:].data_ptr() if tr else None, tr, relu, W["y"].ptr(), mean, inv, ptr(ws), ws.numel(), None)
        out = ["y"] + (["mean", "invstd", "rm", "rv", "nbt"] if tr else [])
    elif e == "bwd":
        a = (ptr(x), ptr(dy), m, c, esz, ptr(I["mean_in"]), ptr(I["invstd_in"]), ga, be, relu)
        z = (W["y"].ptr(), W["dgamma"].ptr(), W["dbeta"].ptr(), ptr(ws), ws.numel(), None)
        st = L.doda_bn_relu_bwd(*a, *z) if add is None else L.doda_bn_relu_bwd_add(*a, ptr(add), add_ld, *z)
        out = ["dx", "dgamma", "dbeta"]
    elif e == "fwd_final":
        st = L.doda_bn_fwd_final(ptr(I["rows"]), p["R"], m, c, EPS, MOMENTUM, W["rm"].ptr(), W["rv"].ptr(), nbt[1:].data_ptr(), W["mean"].ptr(),
                                 W["invstd"].ptr(), None)
        out = ["mean", "invstd", "rm", "rv", "nbt"]
    elif e == "fwd_stats":
        st = L.doda_bn_relu_fwd_stats(ptr(x), m, c, esz, ptr(I["rows"]), p["R"], EPS, MOMENTUM, ga, be, W["rm"].ptr(), W["rv"].ptr(), nbt[1:].data_ptr(),
                                      relu, W["y"].ptr(), W["mean"].ptr(), W["invstd"].ptr(), None)
        out = ["y", "mean", "invstd", "rm", "rv", "nbt"]
    elif e == "apply":
        st = L.doda_bn_relu_apply(ptr(x), m, c, esz, ptr(I["mean_in"]), ptr(I["invstd_in"]), ga, be, relu, W["y"].ptr(), None)
        out = ["y"]
    elif e == "bwd_stats":
        st = L.doda_bn_relu_bwd_stats(ptr(x), ptr(dy), m, c, esz, ptr(I["rows"]), p["R"], ptr(I["mean_in"]), ptr(I["invstd_in"]), ga, be, relu, ptr(add),
                                      add_ld, W["y"].ptr(), W["dgamma"].ptr(), W["dbeta"].ptr(), W["coef"].ptr(), None)
        out = ["dx", "dgamma", "dbeta"]
    elif e == "fwd_totals":
        st = L.doda_bn_relu_fwd_totals(ptr(x), m, c, esz, ptr(I["ta"]), ptr(I["tb"]), p["c_a"], EPS, MOMENTUM, ga, be, W["rm"].ptr(), W["rv"].ptr(),
                                       nbt[1:].data_ptr(), relu, W["y"].ptr(), W["mean"].ptr(), W["invstd"].ptr(), None)
        out = ["y", "mean", "invstd", "rm", "rv", "nbt"]
    elif e == "bwd_totals":
        st = L.doda_bn_relu_bwd_totals(ptr(x), ptr(dy), m, c, esz, ptr(I["ta"]), ptr(I["mean_in"]), ptr(I["invstd_in"]), ga, be, relu, ptr(add), add_ld,
                                       W["y"].ptr(), W["dgamma"].ptr(), W["dbeta"].ptr(), None)
        out = ["dx", "dgamma", "dbeta"]
    elif e == "lay_stats":
        tot = Guarded(8 * 2 * (c // 4), 16, torch.float64, dev)
        tot.inner.fill_(PAD)
        tot.inner[:, :4] = 0
        W = dict(totals=tot)
        st = ops.layers_run([dict(kind=ops.CX_STATS, rows=hi - lo, c_in=c, x=x[lo:hi], x_ld=x.stride(0), stats=tot.inner) for lo, hi in p["ranges"]],
                            dev, esz) * 0
        out = ["totals"]
    elif e == "lay_fwd":
        tr = p["training"]
        op = dict(kind=ops.CX_BNFWD, flags=(ops.CX_F_RELU if relu else 0) | (ops.CX_F_TRAINING if tr else 0), rows=m, c_in=c, x=x, x_ld=c, y=W["y"].inner,
                  y_ld=c + p["y_pad"], gamma=I["gamma"], beta=I["beta"], eps=EPS, momentum=MOMENTUM, running_mean=W["rm"].inner, running_var=W["rv"].inner)
        if tr:
            op.update(stats=I["ta"], stats_b=I["tb"], c_split=p["c_a"], mean=W["mean"].inner, invstd=W["invstd"].inner, nbt=nbt[1:])
        st = ops.layers_run([op], dev, esz) * 0
        out = ["y"] + (["mean", "invstd", "rm", "rv", "nbt"] if tr else [])
    elif e == "lay_bwd":
        sp = p["split"]
        if sp:
            W["y"], W["y2"] = Guarded(m, sp, dt, dev), Guarded(m, c - sp, dt, dev)
        op = dict(kind=ops.CX_BNBWD, flags=(ops.CX_F_RELU if relu else 0) | (ops.CX_F_ACCUM if p["accum"] else 0), rows=m, c_in=c, x=dy, x_ld=c, aux=x,
                  aux_ld=c, y=W["y"].inner, y_ld=sp or c, stats=I["ta"], gamma=I["gamma"], beta=I["beta"], mean=I["mean_in"], invstd=I["invstd_in"],
                  dgamma=W["dgamma"].inner, dbeta=W["dbeta"].inner)
        if sp:
            op.update(c_split=sp, y2=W["y2"].inner, y2_ld=c - sp)
        if add is not None:
            op.update(res=add, res_ld=add_ld)
        st = ops.layers_run([op], dev, esz) * 0
        out = ["dx", "dgamma", "dbeta"]
    torch.cuda.synchronize()
    O = dict(status=int(st), guards={k: w.intact() for k, w in W.items() if k != "coef" or e == "bwd_stats"})
    O["guards"]["nbt"] = bool(nbt[0] == -77) and bool(nbt[2] == -77)
    if "nbt" not in out:
        O["guards"]["nbt"] = O["guards"]["nbt"] and bool(nbt[1] == I["nbt0"])
    if p["status"]:     # an error return: nothing may be written
        O["guards"]["untouched"] = all(bool((w.buf == SENTINEL).all()) for k, w in W.items() if k not in ("rm", "rv")) and bool(nbt[1] == I["nbt0"])
        return O
    for k in out:
        if k == "dx":
            O[k] = torch.cat([W["y"].inner, W["y2"].inner], 1) if p["split"] else W["y"].inner
        elif k == "nbt":
            O[k] = nbt[1:2].double()
        elif k == "totals":
            t = W["totals"].inner.view(8, 2, c // 4, 16)
            O["guards"]["totals_pad"] = bool((t[..., 4:] == PAD).all())
            O[k] = t[..., :4].sum(0).reshape(2, c)
        else:
            O[k] = W[k].inner.reshape(-1) if k not in ("y",) else W[k].inner
    return O


TRACE = re.compile(r"^bn route=(.*) grid=(\d+) block=(\d+)$", re.M)


def run_group(group):
    import torch
    import gathernumerics
    from doda_amd._lib import lib
    assert os.environ.get("DODA_TRACE_BN") == "1" and all(os.environ.get(k) == GROUPS[group].get(k) for k in SWITCHES)
    dev, L = torch.device("cuda:0"), lib()
    for p in probes(group):
        I = make_inputs(p, dev)
        O, text = gathernumerics._with_trace(lambda: run_probe(p, I, L, dev))
        traced = [[m[1], int(m[2]), int(m[3])] for m in TRACE.finditer(text)]
        for t in traced:
            print(json.dumps(dict(trace=t[0], grid=t[1], block=t[2])), flush=True)
        res = dict(id=p["id"], status=O["status"], route=traced, guards=all(O["guards"].values()), err={}, fails=[])
        if O["status"] != p["status"]:
            res["fails"].append("status %d, expected %d" % (O["status"], p["status"]))
        elif not p["status"]:
            res["err"], res["fails"] = check(p, I, O)
        else:
            res["fails"] = ["sentinel overwritten around " + k for k, ok in O["guards"].items() if not ok]
        if traced != [list(r) for r in routes(p)]:
            res["fails"].append("route %s, expected %s" % (traced, routes(p)))
        res["ratio"] = max([v[1] for v in res["err"].values()], default=0.0)
        print(json.dumps(res), flush=True)


def profile(files):
    """The table of profiles/r15_bn_numerics.txt from the result lines of --numerics runs."""
    print("# probe | traced launches (kernel grid x workgroup) | per quantity: largest error (error / bound) | largest ratio")
    for f in files:
        for l in open(f):
            if l.startswith("{") and '"id"' in l:
                r = json.loads(l)
                print("%s | %s | %s | %.3g%s" % (r["id"], "; ".join("%s %dx%d" % tuple(t) for t in r["route"]) or "status %d" % r["status"],
                                                " ".join("%s %.3g (%.3g)" % (k, v[0], v[1]) for k, v in r["err"].items()), r["ratio"],
                                                "" if not r["fails"] and r["guards"] else " FAILS " + "; ".join(r["fails"])))


if __name__ == "__main__":
    if sys.argv[1] == "--numerics":
        sys.path.insert(0, ROOT)
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(GROUPS[sys.argv[2]], DODA_TRACE_BN="1")      # (read by the library at its first BatchNorm launch)
        run_group(sys.argv[2])
    elif sys.argv[1] == "--list":
        for p in probes(sys.argv[2] if len(sys.argv) > 2 else None):
            print(p["id"], routes(p))
    elif sys.argv[1] == "--profile":
        profile(sys.argv[2:])

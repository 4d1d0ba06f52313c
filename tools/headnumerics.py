#!/usr/bin/env python
"""The head and loss kernels of csrc/head.hip (+ head_common.hpp), csrc/lovasz.hip and csrc/loss.hip against fp64 references, at
their edges (tests/test_gpu_head_numerics.py, tests/test_head_numerics_host.py).  Importable without a GPU.

  python tools/headnumerics.py --numerics [GROUP]   every probe (of the group) on the device, one JSON line per probe
  python tools/headnumerics.py --list [GROUP]       the probe table with the kernels each probe reaches
  python tools/headnumerics.py --profile OUT.jsonl  the result lines as the table of profiles/r19_head_numerics.txt

THE PROBE TABLE (probes()).  Groups A (doda_head_ce_fwd / _bwd), B (doda_head_dw_bf16), C (doda_st_voxel_confidence),
D (doda_cross_entropy_fwd / _bwd), E (doda_seg_meters), F (doda_lovasz_fwd / _bwd).  kernels(p) names the instantiations a probe
launches, from a Python restatement of the host geometry (hd_blocks, dw_blocks, bucket, ce_blocks, ce_bwd_blocks, meter_blocks,
lv_plan) whose constants are PARSED from the sources (constants()).

INPUTS (make_inputs).  Features [m, c] in the storage type, weights [n_cls, c] and bias fp32; three families: `exact` (the dyadic
grids of tests/lovasz_cases.py: every logit exact in fp32; exact ties by copied weight rows: classes (0, n_cls - 1), (1, 2) inside a
group of four, (3, 4) across a group boundary), `general` (randn x 1.5, weights x 0.4, bias x 0.2), `saturated` (the general weights
x 30).  Point lists: one point per voxel; two (1-2 points, v2p_ld = 3); ragged (0-3 points, every seventh voxel with all its points
ignored, point ids out of order); big (ragged + one voxel of 300 points); wide (ragged, v2p_ld 5 wider than any count).  Labels:
classes, the ignore index (255, -100 or 3: a real class), -1, n_cls and 2^32 + 3 among them.

THE REFERENCES are numpy fp64 from the definitions in the three file headers; bf16 probes use the weights rounded to bf16
(hd_stage_weights).  Lovasz: the weighted-item form (two items per voxel and class, descending error, J in fp64); the host test
holds it to doda_amd.lovasz.lovasz_softmax in fp64 on the gathered score matrix and its autograd.

THE BOUNDS.  u = 2^-24; every quantity has a per-element SCALE written from its definition with |.| of every addend, and a derived
count D of fp32 operations; the check is  error <= allowed x u x scale  (+ 2^-8 |value| for a bf16 store, + the Lovasz slack below),
allowed = max(4 x the ratio the reference model's own fp32 path reaches on the same probe and device, D): the accuracy of __expf,
__logf, expf and the division on gfx950 is measured, not assumed.  With C channels, NK the class bucket, S_z = sum_c |w f| + |b|,
Smax = max_k S_z:
  logit          S_z                                  C fmas + 1 add: C + 1
  p_k, conf      p (1 + 2 Smax) + 2^-100              D_p = max(2 (C + 2), NK + 4): the argument z - max carries (C + 1) u S_z twice and
                                                      its own rounding, in e_k and again in the sum; the NK - 1 additions, the division
                                                      and two exp errors only where Smax is small
  lse            Smax + |lse| + 1                     D_lse = max(3 C + 5, NK + 4): max (C + 1) + log of the sum (2 (C + 2)), or the sum
  loss           mean of cnt (lse scale) + hist S_z   D_lse + C + 1 + chain, chain = a thread's additions (the points of the workgroup's
                                                      longest voxel, or its rows in ce_fwd) + 6 butterfly steps + 3 wave sums + 2
                                                      (fp64 combine, division); per workgroup, folded into the scale
  dz (CE)        |g/n| (cnt p-scale + hist)           D_p + 3 + the element's own hist (hist subtractions of g/n, one rounding each)
  d_feats        sum_k |w| dz-scale                   D_dz + n_cls fmas
  db rows        sum over the workgroup's voxels      D_dz + 35 (32 columns in sequence, 3 shuffles)
  dW partials    sum |dz f| over the workgroup        64 T + 3: two 32-term MFMA sums per 64-voxel chunk, T chunks per wave, four waves
  dW from kernel dz: the dz bound times |f| + 2^-8 sum |dz f| (cross-entropy, bf16 dz) or 2^-16 (Lovasz, dz + dz_lo)
  dlogits        |g/n| (p-scale + onehot)             (D_lse + 1)(1 + ln c) + 6: the error of lse enters the argument of the exp
  gitem          |g|                                  2 (J in fp64, one rounding) + slack
  dz (Lovasz)    p-scale (|dp_k| + sum_j p_j |dp_j|)  D_p + n_cls + 8, + the slack through the same expression
Lovasz slack: the device orders items by ITS fp32 probabilities.  Two items of a class whose reference errors lie within their
probability bounds of each other (D_p u scale each) have no defined order; an item's gradient g = J(after) - J(before) is then
bounded by evaluating it with every such neighbour's weight moved before / after it (J is monotone in both prefix sums), and the
difference to the reference order is its slack.  The loss is the convex Lovasz extension: its error is at most sum_i (error of e_i)
x min(|g_i| + slack_i, w_i / G).  Items of non-zero weight that share their fp32 key with another item of non-zero weight in the
reference are left out of the per-item comparison (at most 1e-3 of a probe's items; an item of weight zero has g = 0 wherever it
stands).  The slack applies to the per-item and per-voxel outputs (gitem, dz, d_feats) only: the summed gradients (db rows, db, dW)
are held to their operation counts alone, since inside a run of near-tied keys the reordered g's sum to J(after) - J(before)
whatever the order.  The identical-voxel and the saturated probes (every key of a class ties; keys tie at errors 0 and 1) compare
the loss, the per-class sum of g, db, dW and the zero rows of voxels without a valid point.
pred: the exact family on every voxel; elsewhere where the fp64 top-2 gap exceeds 2 (C + 1) u Smax, one of the two top
classes where it does not (at most 1e-3 of a probe's voxels)."""
import json
import math
import os
import re
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "doda_amd", "csrc")
INSTANTIATIONS = os.path.join(ROOT, "tests", "data", "head_instantiations.json")
STEMS = ("head_", "st_voxel_conf", "lovasz_", "ce_", "seg_meters")      # tools/gatherroutes.py --instantiations --stem head_,... head.o lovasz.o loss.o
OBJECTS = ("head.o", "lovasz.o", "loss.o")
U = 2.0 ** -24
BF = 2.0 ** -8
FLOOR = 2.0 ** -100
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -4, -5
MAX_LEFT_OUT = 1e-3
SENTINEL, GUARD = 0x5A, 256
BIG_LABEL = 2 ** 32 + 3
GROUPS = ("A", "B", "C", "D", "E", "F")
HOST_ROWS = 5000       # the host test evaluates the float32 restatement up to this many rows


# ------------------------------------------------------------------------------------------------------ the code's own constants
def constants():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("head.hip", "head_common.hpp", "lovasz.hip", "loss.hip", "core.hip")}
    K = {}
    for f in ("head_common.hpp", "lovasz.hip", "loss.hip", "core.hip"):
        for m in re.finditer(r"constexpr int ([A-Z_0-9, =a-z<*/]+);", src[f]):
            for part in m[1].split(","):
                name, expr = [s.strip() for s in part.split("=")]
                try:      # integer arithmetic over literals and earlier constants; a constant of another form is not one of ours
                    K[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(K)))
                except (NameError, SyntaxError, TypeError, ValueError):
                    pass
    one = lambda f, pat: int(re.search(pat, src[f])[1])
    K["BUCKETS"] = [int(x) for x in re.findall(r"KERNEL<ESZ, C, (\d+)>", src["head_common.hpp"])]
    assert [int(x) for x in re.findall(r"nk <= (\d+)", src["head_common.hpp"])] == K["BUCKETS"][:-1]
    K["FINAL_THREADS"] = one("head.hip", r"k < nblocks; k \+= (\d+)")
    K["DW_CAP"] = one("head.hip", r"if \(nb > (\d+)\) nb = \1;")
    K["SCAN_LANES"] = one("lovasz.hip", r"t0 < stiles; t0 \+= (\d+)")
    K["CE_FWD_CAP"], K["CE_BWD_CAP"], K["METER_CAP"] = [int(x) for x in re.findall(r"if \(nb > (\d+)\) nb = \1;", src["loss.hip"])]
    K["CE_ROWS"] = one("loss.hip", r"div_up\(n, CE_BLOCK \* (\d+)\)")
    K["LOVASZ_MAX_POINTS"] = int(re.search(r"DODA_LOVASZ_MAX_POINTS_PER_VOXEL (\d+)", open(os.path.join(ROOT, "include", "doda_loss.h")).read())[1])
    return K


K = constants()
HD_BLOCK = K["HD_BLOCK"]
div_up = lambda a, b: -(-a // b)
align_up = lambda a, b: div_up(a, b) * b


# ----------------------------------------------------------------------------------------- the launchers' geometry, in Python
def hd_blocks(m):
    return max(div_up(m, HD_BLOCK), 1)


def dw_blocks(m):
    return max(min(div_up(div_up(max(m, 1), 64), 4), K["DW_CAP"]), 1)


def bucket(n_cls):
    nk = (n_cls + 3) // 4 * 4
    return next((e for e in K["BUCKETS"][:-1] if nk <= e), K["BUCKETS"][-1])


def ce_blocks(n):
    return max(min(div_up(n, K["CE_BLOCK"] * K["CE_ROWS"]), K["CE_FWD_CAP"]), 1)


def ce_bwd_blocks(n, c):
    return min(div_up(n * c, K["CE_BLOCK"] * K["CE_ROWS"]), K["CE_BWD_CAP"])


def meter_blocks(n):
    return min(div_up(n, 256 * 4), K["METER_CAP"])


def lv_plan(m, n_cls):
    """lovasz.hip lv_plan: the item, tile and workspace geometry of doda_lovasz_fwd."""
    seg = 2 * m
    total = seg * n_cls
    tiles, stiles = div_up(seg, K["LV_WTILE"]), div_up(seg, K["LV_STILE"])
    P = dict(seg=seg, total=total, tiles=tiles, n_wt=tiles * n_cls, stiles=stiles, n_st=stiles * n_cls, hist_len=tiles * n_cls * K["LV_BINS"])
    P["scan_tiles"] = div_up(P["hist_len"], K["SCAN_TILE"])
    pieces = [total * 4] * 4 + [total * 2, P["hist_len"] * 4, P["hist_len"] * 4, (P["scan_tiles"] + 8) * 4, P["n_st"] * 8, P["n_st"] * 8, 32 * 8, P["n_st"] * 8]
    P["bytes"] = sum(align_up(b, 256) for b in pieces)
    return P


def kernels(p):
    """The compiled kernels the calls of probe p launch; none where the call returns an error."""
    if p["status"]:
        return []
    g, esz, c, k = p["group"], p["esz"], p["c"], p["n_cls"]
    t = lambda stem, cc=16: "%s<%d, %d, %d>" % (stem, esz, cc, bucket(k))
    dw = ["head_dw_bf16"] if esz == 2 else []
    if g == "A":
        return [t("head_ce_fwd"), "head_ce_final", t("head_ce_bwd")] + dw
    if g == "B":
        return ["head_dw_bf16"]
    if g == "C":
        return [t("st_voxel_conf", c)] + ([t("head_ce_fwd"), "head_ce_final"] if c == 16 else [])
    if g == "D":
        return ["ce_fwd", "ce_final", "ce_bwd"]
    if g == "E":
        return ["seg_meters<%s>" % ("true" if p["p64"] else "false")]
    return [t("lovasz_items"), "lovasz_sort_hist", "lovasz_sort_scatter<true>", "lovasz_sort_scatter<false>", "lovasz_tile_sums",
            "lovasz_tile_scan", "lovasz_grad", "lovasz_final", t("lovasz_bwd")] + dw


# ------------------------------------------------------------------------------------------------------------- the probe table
DEFAULTS = dict(esz=4, c=16, n_cls=20, m=1, family="general", lists="one", labels="mixed", ignore=255, bias=1, grad=1.7, status=0, what="",
                p64=0, p2v=0, mode="items")
FAMILIES = ("exact", "general", "saturated")
LISTS = ("one", "ragged", "big", "wide")
IGNORES = (255, -100, 3)


# probes whose first seed left more than MAX_LEFT_OUT of their voxels / items out (tests/test_head_numerics_host.py asserts the cap)
RESEED = {'C-e4-c32-k32-m257-general-one-clean-i255-b0-g1.7': 1}


def probes(group=None):
    P = []

    def add(g, **kw):
        d = dict(DEFAULTS, group=g, **kw)
        d["id"] = "%s%s-e%d-c%d-k%d-m%d-%s-%s-%s-i%d-b%d-g%g%s" % (g, "-" + d["what"] if d["what"] else "", d["esz"], d["c"], d["n_cls"], d["m"], d["family"],
                                                                   d["lists"], d["labels"], d["ignore"], d["bias"], d["grad"],
                                                                   "-p64%d-p2v%d" % (d["p64"], d["p2v"]) if g == "E" else "")
        d["seed"] = (zlib.crc32(d["id"].encode()) & 0x7fffffff) + RESEED.get(d["id"], 0)
        assert d["id"] not in {q["id"] for q in P}, d["id"]
        P.append(d)

    for esz in (4, 2):
        i = 0
        # A: every bucket edge x the workgroup edge; families, lists and ignore indices in rotation
        for k in (1, 2, 12, 13, 16, 17, 20, 21, 32):
            for m in (1, 255, 256, 257):
                add("A", esz=esz, n_cls=k, m=m, family=FAMILIES[i % 3], lists=LISTS[(i + i // 4) % 4], ignore=IGNORES[(i // 3) % 3])
                i += 1
        for k in (2, 13, 17, 21):      # NULL bias, once per bucket
            add("A", esz=esz, n_cls=k, m=257, lists="ragged", bias=0, family=FAMILIES[k % 3])
        add("A", esz=esz, n_cls=13, m=257, lists="big", grad=0.0)
        add("A", esz=esz, n_cls=20, m=257, lists="ragged", labels="allign")
        add("A", esz=esz, n_cls=5, m=300, lists="ragged", family="exact", ignore=3)
        for m in (K["FINAL_THREADS"] * HD_BLOCK, K["FINAL_THREADS"] * HD_BLOCK + 1):      # 1024 and 1025 partial rows
            add("A", esz=esz, n_cls=20, m=m, lists="two")
        add("A", esz=esz, n_cls=33, m=37, what="k33", status=ERR_UNSUPPORTED)
        add("A", esz=esz, n_cls=20, m=37, c=32, what="c32", status=ERR_UNSUPPORTED)
        add("A", esz=esz, n_cls=20, m=300, what="nblocks", status=ERR_WORKSPACE)
        # C: both channel counts, every bucket from both sides
        i = 0
        for c in (16, 32):
            for k in (2, 12, 13, 16, 17, 20, 21, 32):
                for m in (1, 257):
                    add("C", esz=esz, c=c, n_cls=k, m=m, family=FAMILIES[i % 3], bias=int(i % 4 != 3), lists="one", labels="clean")
                    i += 1
        # F: the chunk, batch and tile sizes of the sort and the scan from both sides
        i = 0
        for m in (32, 33, 128, 129, 1024, 1025, 2048, 2049):
            add("F", esz=esz, n_cls=11, m=m, family=("exact", "general")[i % 2], lists=("ragged", "one", "wide")[i % 3], ignore=IGNORES[i % 3],
                labels=("mixed", "absent")[(i // 2) % 2], bias=int(i % 4 != 1))
            i += 1
        add("F", esz=esz, n_cls=2, m=K["SCAN_LANES"] * K["LV_STILE"] // 2 + 1, lists="one", family="general", labels="sparse")             # 65 scan tiles
        add("F", esz=esz, n_cls=32, m=32769, lists="one", family="general")                                           # scan_partials' second round
        for k in (13, 20):      # the two middle buckets
            add("F", esz=esz, n_cls=k, m=300, lists="big", family=("general", "exact")[k % 2])
        add("F", esz=esz, n_cls=3, m=3, lists="w16", labels="w16", family="general")
        add("F", esz=esz, n_cls=11, m=5000, lists="two", family="identical", mode="sums")
        add("F", esz=esz, n_cls=11, m=257, lists="ragged", family="saturated", mode="sums")
        add("F", esz=esz, n_cls=11, m=257, lists="ragged", labels="allign")
        add("F", esz=esz, n_cls=11, m=257, lists="ragged", grad=0.0)
        add("F", esz=esz, n_cls=2, m=1, lists="ld65537", labels="clean", what="ld", status=ERR_UNSUPPORTED)
    # B
    for m in (1, 63, 64, 65, 255, 256, 257):
        for k in (1, 2, 11, 20, 31, 32):
            add("B", esz=2, n_cls=k, m=m)
    for m in (K["DW_CAP"] * 256, K["DW_CAP"] * 256 + 1):
        for k in (11, 20):
            add("B", esz=2, n_cls=k, m=m)
    add("B", esz=2, n_cls=20, m=65, what="dzalign", status=ERR_INVALID)
    add("B", esz=2, n_cls=20, m=65, what="falign", status=ERR_INVALID)
    # D
    i = 0
    for c in (1, 2, 5, 20, 63, 64):
        for n in (1, 1023, 1025, 70001):
            add("D", c=c, n_cls=c, m=n, family=("general", "saturated")[i % 2], ignore=IGNORES[i % 3])
            i += 1
    for n in (K["CE_FWD_CAP"] * K["CE_BLOCK"] * K["CE_ROWS"], K["CE_FWD_CAP"] * K["CE_BLOCK"] * K["CE_ROWS"] + 1):
        add("D", c=5, n_cls=5, m=n)
    add("D", c=20, n_cls=20, m=1025, grad=0.0)
    add("D", c=20, n_cls=20, m=1025, labels="allign")
    add("D", c=65, n_cls=65, m=37, what="c65", status=ERR_UNSUPPORTED)
    # E
    for k in (1, 20, 255, 256):
        for n in (1, K["METER_CAP"] * 1024, K["METER_CAP"] * 1024 + 1):
            for p64 in (0, 1):
                for p2v in (0, 1):
                    add("E", c=0, n_cls=k, m=n, p64=p64, p2v=p2v)
    add("E", c=0, n_cls=257, m=37, what="k257", status=ERR_UNSUPPORTED)
    return [p for p in P if group in (None, p["group"])]


# -------------------------------------------------------------------------------------------------------------------- inputs
def r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def rbf(x):
    """Round to bf16, nearest even (the values are fp32 first, as on the device)."""
    b = np.asarray(x, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def rstore(x, esz):
    return rbf(x) if esz == 2 else r32(x)


def make_lists(p, rng):
    """-> v2p int32 [m, ld] (count, point ids, unused slots -1), pv int64 [points]: the voxel of each point."""
    m, kind = p["m"], p["lists"]
    if kind in ("one", "ld65537"):
        counts = np.ones(m, np.int64)
    elif kind == "two":
        counts = rng.randint(1, 3, m).astype(np.int64)
    elif kind == "w16":
        counts = np.array([K["LOVASZ_MAX_POINTS"], 2, 1], np.int64)
    else:
        counts = rng.randint(0, 4, m).astype(np.int64)
        counts[0] = max(counts[0], 1)
        if kind == "big":
            counts[m // 2] = 300
    n = int(counts.sum())
    ld = {"two": 3, "wide": 1 + int(counts.max()) + 5, "ld65537": K["LOVASZ_MAX_POINTS"] + 2}.get(kind, 1 + int(counts.max()))
    ids = np.arange(n) if kind == "one" else rng.permutation(n)
    vox = np.repeat(np.arange(m), counts)
    pos = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    v2p = np.full((m, ld), -1, np.int32)
    v2p[:, 0] = counts
    v2p[vox, 1 + pos] = ids
    pv = np.empty(n, np.int64)
    pv[ids] = vox
    return v2p, pv


def make_labels(p, rng, n, pv=None):
    k, kind, ign = p["n_cls"], p["labels"], p["ignore"]
    lab = rng.randint(0, k, n).astype(np.int64)
    if kind == "allign":
        return np.full(n, ign, np.int64)
    if kind == "w16":
        lab[pv == 0] = 1
        return lab
    if kind == "clean":
        return lab
    if kind == "absent":
        lab[lab == k // 2] = (k // 2 + 1) % k
    lab[rng.rand(n) < (0.75 if kind == "sparse" else 0.2)] = ign      # (sparse: fewer items of non-zero weight, fewer tied fp32 keys among 131 074)
    order = rng.permutation(n)
    cut = max(n // 50, 1)
    for j, bad in enumerate((-1, k, BIG_LABEL) if n >= 6 else ()):
        lab[order[j * cut:(j + 1) * cut]] = bad
    if pv is not None and p["lists"] in ("ragged", "big", "wide"):
        lab[pv % 7 == 3] = ign
    if kind == "absent":
        lab[lab == k // 2] = ign
    if pv is not None and p["lists"] == "two":
        lab[pv == p["m"] - 1] = 1      # (the last workgroup's only voxel counts)
    return lab


def make_inputs(p):
    """numpy inputs of probe p; float arrays are fp64 holding values exact in their storage type."""
    rng = np.random.RandomState(p["seed"])
    g, m, k, c, esz, fam = p["group"], p["m"], p["n_cls"], p["c"], p["esz"], p["family"]
    I = {}
    if g == "E":
        nv = m // 2 + 1 if p["p2v"] else m
        I["preds"] = rng.randint(-3, k + 3, nv).astype(np.int64)
        I["p2v"] = rng.randint(0, nv, m).astype(np.int32) if p["p2v"] else None
        lab = rng.randint(-2, k + 2, m).astype(np.int64)
        lab[rng.rand(m) < 0.1] = p["ignore"]
        lab[rng.rand(m) < 0.01] = BIG_LABEL
        I["labels"], I["hist0"] = lab, np.arange(3 * k, dtype=np.int64) % 7
        return I
    if g == "D":
        I["z"] = r32(rng.randn(m, c) * 2.0 * (30 if fam == "saturated" else 1))
        I["labels"] = make_labels(p, rng, m)
        return I
    if g == "B":
        F, dz = rng.randn(m, 16), rng.randn(m, k) * 0.01
        F[::37] *= 2.0 ** 10
        dz[5::41] *= 2.0 ** 10
        I["F"], I["dz"] = rbf(F), rbf(dz)
        return I
    if fam == "exact":
        F = rng.randint(-127, 128, (m, c)) / 64.0
        W = rng.randint(-48, 49, (k, c)) / 128.0
        b = rng.randint(-48, 49, k) / 128.0
        for lo, hi in ((0, k - 1), (1, 2), (3, 4)):
            if lo < hi < k:
                W[hi], b[hi] = W[lo], b[lo]
    else:
        F, W, b = rng.randn(m, c) * 1.5, rng.randn(k, c) * 0.4, rng.randn(k) * 0.2
        if fam == "saturated":
            W = W * 30
        if fam == "identical":
            F[:] = F[0]
    if not p["bias"]:
        b = np.zeros(k)
    I["F"], I["W"], I["b"] = rstore(F, esz), r32(W), r32(b)
    I["Weff"] = rbf(I["W"]) if esz == 2 else I["W"]
    I["v2p"], I["pv"] = make_lists(p, rng)
    I["labels"] = make_labels(p, rng, len(I["pv"]), I["pv"])
    return I


# ----------------------------------------------------------------------------------------------------------------- references
def valid_mask(lab, ign, k, wrong=None):
    if wrong == "label_mod":
        lab = np.where(lab >= 2 ** 32, lab - 2 ** 32, lab)
    return (lab != ign) & (lab >= 0) & (lab < k)


def counts_hist(p, I, wrong=None):
    """cnt [m], hist [m, k]: the valid points of a voxel, per class."""
    m, k = p["m"], p["n_cls"]
    ok = valid_mask(I["labels"], p["ignore"], k, wrong)
    lab = np.where(I["labels"] >= 2 ** 32, I["labels"] - 2 ** 32, I["labels"])
    flat = np.bincount(I["pv"][ok] * k + lab[ok], minlength=m * k).astype(np.float64)
    hist = flat.reshape(m, k)
    return hist.sum(1), hist


def softmax64(z):
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(1, keepdims=True)
    return e / s, (mx + np.log(s))[:, 0]


def d_counts(C, NK):
    return max(2 * (C + 2), NK + 4), max(3 * C + 5, NK + 4)


def weigh(scale, D):
    """A per-element operation count D folded into the scale: -> (scale D / max D, max D)."""
    D = np.asarray(D, np.float64)
    return scale * D / D.max(), float(D.max())


def block_sum(x, nb, block=HD_BLOCK):
    """Row sums of x [m, ...] over consecutive blocks of `block` rows -> [nb, ...]."""
    pad = nb * block - x.shape[0]
    x = np.concatenate([x, np.zeros((pad,) + x.shape[1:])]) if pad else x
    return x.reshape((nb, block) + x.shape[1:]).sum(1)


def pred_ref(z, Sz, C, exact, wrong=None):
    order = np.argsort(-z, axis=1, kind="stable")
    top1 = order[:, 0]
    top2 = order[:, 1] if z.shape[1] > 1 else top1
    if wrong == "tie_high":
        top1 = z.shape[1] - 1 - np.argmax(z[:, ::-1], axis=1)
    gap = z[np.arange(len(z)), top1] - z[np.arange(len(z)), top2] if z.shape[1] > 1 else np.full(len(z), np.inf)
    decided = np.ones(len(z), bool) if exact else gap > 2 * (C + 1) * U * Sz.max(1)
    return dict(top1=top1, top2=top2, decided=decided)


def head_logits(p, I, wrong=None):
    W = I["W"] if wrong == "no_bf16_w" else I["Weff"]
    z = I["F"] @ W.T + I["b"]
    Sz = np.abs(I["F"]) @ np.abs(W).T + np.abs(I["b"])
    return W, z, Sz


def ref_head(p, I, wrong=None):
    """Groups A and C.  -> dict(vals {name: (value, scale, D, slack, bf16 store factor)}, exact {name: array}, pred, zero {name: rows})."""
    m, k, C, esz, g = p["m"], p["n_cls"], p["c"], p["esz"], p["group"]
    NK = bucket(k)
    W, z, Sz = head_logits(p, I, wrong)
    Smax = Sz.max(1)
    zs = np.concatenate([z, np.zeros((m, NK - k))], 1) if wrong == "pad_zero" else z
    prob, lse = softmax64(zs)
    prob = prob[:, :k]
    Dp, Dl = d_counts(C, NK)
    sp = prob * (1 + 2 * Smax)[:, None] + FLOOR
    R = dict(vals={}, exact={}, zero={}, pred=pred_ref(z, Sz, C, p["family"] == "exact", wrong))
    if g == "C":
        R["vals"]["conf"] = (prob.max(1), sp.max(1), Dp, 0.0, 0.0)
        return R
    cnt, hist = counts_hist(p, I, wrong)
    n = cnt.sum()
    np_all = I["v2p"][:, 0].astype(np.float64)
    cnt_dz = np_all if wrong == "cnt_ignored" else cnt
    nv = max(len(I["pv"]) if wrong == "mean_all" else n, 1.0)
    nb = hd_blocks(m)
    term = cnt_dz * lse - (hist * z).sum(1)
    s_term = cnt * (Smax + np.abs(lse) + 1) + (hist * Sz).sum(1)
    part, s_part = block_sum(term, nb), block_sum(s_term, nb)
    # the chain of a workgroup: the points of its longest voxel, 6 butterfly steps, 3 wave sums, 2 (fp64 combine, division)
    pad = nb * HD_BLOCK - m
    chain = np.concatenate([np_all, np.zeros(pad)]).reshape(nb, HD_BLOCK).max(1) + 6 + 3 + 2
    s_part, Dloss = weigh(s_part, Dl + C + 1 + chain)
    rows = part[:K["FINAL_THREADS"]] if wrong == "drop_rows_1024" else part
    R["vals"]["out0"] = (rows.sum() / nv, s_part.sum() / nv, Dloss, 0.0, 0.0)
    R["vals"]["part_loss"] = (part, s_part, Dloss, 0.0, 0.0)
    R["exact"]["part_cnt"] = block_sum(cnt, nb)
    R["exact"]["out1"] = np.float64(R["exact"]["part_cnt"][:K["FINAL_THREADS"]].sum() if wrong == "drop_rows_1024" else n)
    sc = p["grad"] / nv
    dz = sc * (cnt_dz[:, None] * prob - hist)
    if wrong == "drop_last_odd":
        dz[:, k - 1] = 0
    s_dz, Ddz = weigh(abs(sc) * (cnt[:, None] * sp + hist), Dp + 3 + hist)      # (an element's own hist subtractions)
    bf = BF if esz == 2 else 0.0
    R["vals"]["dz"] = (dz, s_dz, Ddz, 0.0, bf)
    R["vals"]["d_feats"] = (dz @ W, s_dz @ np.abs(W), Ddz + k, 0.0, bf)
    dbp, s_dbp = block_sum(dz, nb), block_sum(s_dz, nb)
    if wrong == "drop_last_db":
        dbp[-1] = 0
    R["vals"]["dbp"] = (dbp, s_dbp, Ddz + 35, 0.0, 0.0)
    R["vals"]["db"] = (dbp.sum(0), s_dbp.sum(0), Ddz + 35, 0.0, 0.0)
    if esz == 2:      # head_dw_bf16 on the kernel's own bf16 dz
        absdzf = np.abs(dz).T @ np.abs(I["F"])
        T = div_up(div_up(m, 64), 4 * dw_blocks(m))
        R["vals"]["dW"] = (dz.T @ I["F"], s_dz.T @ np.abs(I["F"]), Ddz + 64 * T + 3, (BF + (64 * T + 3) * U) * absdzf, 0.0)
    R["zero"]["dz"] = R["zero"]["d_feats"] = cnt == 0
    R["allzero"] = ["dz", "d_feats", "dbp"] if n == 0 or p["grad"] == 0 else []
    return R


def dw_block_of(m):
    """The workgroup of each 64-voxel chunk of head_dw_bf16: chunks 4 b + wave, stepping 4 grid."""
    grid = dw_blocks(m)
    ch = np.arange(div_up(m, 64))
    return (ch % (4 * grid)) // 4, grid


def ref_dw(p, I, wrong=None):
    m, k = p["m"], p["n_cls"]
    F, dz = I["F"], I["dz"]
    n_ch = div_up(m, 64)
    pad = n_ch * 64 - m
    Fp, dzp = np.concatenate([F, np.zeros((pad, 16))]), np.concatenate([dz, np.zeros((pad, k))])
    blk, grid = dw_block_of(m)
    if wrong == "stale_lanes" and pad:      # the last chunk's tail lanes keep the rows of the wave's previous chunk
        prev = (n_ch - 1 - 4 * grid) * 64
        Fp[m:], dzp[m:] = Fp[prev + 64 - pad:prev + 64], dzp[prev + 64 - pad:prev + 64]
    per = np.einsum("nvk,nvc->nkc", dzp.reshape(n_ch, 64, k), Fp.reshape(n_ch, 64, 16))
    aper = np.einsum("nvk,nvc->nkc", np.abs(dzp).reshape(n_ch, 64, k), np.abs(Fp).reshape(n_ch, 64, 16))
    if wrong == "missing_chunk":
        per[min(1, n_ch - 1)] = 0
    part, s_part = np.zeros((grid, 32, 16)), np.zeros((grid, 32, 16))
    np.add.at(part[:, :k], blk, per)
    np.add.at(s_part[:, :k], blk, aper)
    D = 64 * div_up(n_ch, 4 * grid) + 3
    R = dict(vals={"part": (part, s_part + FLOOR, D, 0.0, 0.0), "dW": (part.sum(0)[:k], s_part.sum(0)[:k] + FLOOR, D, 0.0, 0.0)}, exact={}, zero={})
    R["padzero"] = k
    return R


def ce_block_of(n):
    grid = ce_blocks(n)
    return (np.arange(n) // K["CE_BLOCK"]) % grid, grid


def ref_ce(p, I, wrong=None):
    n, c = p["m"], p["c"]
    z = I["z"]
    Smax = np.abs(z).max(1)
    prob, lse = softmax64(z)
    if wrong == "no_max":
        with np.errstate(over="ignore"):
            lse = np.log(np.exp(z.astype(np.float32)).sum(1, dtype=np.float32)).astype(np.float64)
    Dp, Dl = d_counts(0, c)
    sp = prob * (1 + 2 * Smax)[:, None] + FLOOR
    ok = valid_mask(I["labels"], p["ignore"], c)
    y = np.where(ok, I["labels"], 0)
    zy = z[np.arange(n), y]
    nvalid = ok.sum()
    nv = max(nvalid, 1)
    blk, grid = ce_block_of(n)
    chain = div_up(n, grid * K["CE_BLOCK"]) + 6 + 3 + 2
    s_lse = Smax + np.abs(lse) + 1
    term, s_term = np.where(ok, lse - zy, 0.0), np.where(ok, s_lse + np.abs(zy), 0.0)
    part, s_part = np.bincount(blk, term, grid), np.bincount(blk, s_term, grid)
    R = dict(vals={}, exact={}, zero={})
    R["vals"]["lse"] = (lse, s_lse, Dl, 0.0, 0.0)
    R["vals"]["out0"] = (part.sum() / nv, s_part.sum() / nv, Dl + chain, 0.0, 0.0)
    R["vals"]["part_loss"] = (part, s_part, Dl + chain, 0.0, 0.0)
    R["exact"]["out1"] = np.float64(nvalid)
    R["exact"]["part_cnt"] = np.bincount(blk, ok.astype(np.float64), grid)
    sc = p["grad"] / nv
    onehot = np.zeros((n, c))
    onehot[np.arange(n), y] = 1
    R["vals"]["dlogits"] = ((prob - onehot) * sc * ok[:, None], abs(sc) * (sp + onehot), (Dl + 1) * (1 + math.log(c)) + 6, 0.0, 0.0)
    R["zero"]["dlogits"] = ~ok
    R["allzero"] = ["dlogits"] if nvalid == 0 or p["grad"] == 0 else []
    return R


def ref_meters(p, I, wrong=None):
    k = p["n_cls"]
    ok = valid_mask(I["labels"], p["ignore"], k)
    q = I["preds"][I["p2v"]] if I["p2v"] is not None else I["preds"]
    if wrong == "no_clamp":
        ok = ok & (q >= 0) & (q < k)
    q, t = np.clip(q[ok], 0, k - 1), I["labels"][ok]
    h = np.stack([np.bincount(t[q == t], minlength=k), np.bincount(q, minlength=k), np.bincount(t, minlength=k)]).reshape(-1)
    return dict(vals={}, zero={}, exact={"hist": (I["hist0"] + 2 * h).astype(np.float64)})


def _swappable(lo, hi, w):
    """For items in descending order of error with intervals [lo, hi]: the weight of the earlier items that may come after item i
    (lo_j <= hi_i) and of the later items that may come before it (hi_j >= lo_i)."""
    tot, cw = w.sum(), np.cumsum(w)
    o = np.argsort(lo)
    cl = np.concatenate([[0.0], np.cumsum(w[o])])
    before = cl[np.searchsorted(lo[o], hi, side="right")] - (tot - cw + w)
    o = np.argsort(hi)
    ch = np.concatenate([[0.0], np.cumsum(w[o])])
    after = (tot - ch[np.searchsorted(hi[o], lo, side="left")]) - cw
    return before, after


def lovasz_class(err, delta, wf, wb, want_slack=True, carry_tile=None):
    """One class over its 2 m items (2 v: bg, 2 v + 1: fg): -> (loss, g [2 m], slack [2 m], gcap [2 m])."""
    G = wf.sum()
    n = len(err)
    if G == 0:
        return 0.0, np.zeros(n), np.zeros(n), np.zeros(n)
    order = np.argsort(-err, kind="stable")
    e, f, b = err[order], wf[order], wb[order]
    cf, cb = np.cumsum(f), np.cumsum(b)
    if carry_tile is not None and n > carry_tile:      # (the mistake: the prefix of the first 64 scan tiles is lost)
        cf[carry_tile:] -= cf[carry_tile - 1]
        cb[carry_tile:] -= cb[carry_tile - 1]
    J = 1.0 - (G - cf) / (G + cb)
    gs = np.diff(J, prepend=0.0)
    slack = np.zeros(n)
    if want_slack:
        d = delta[order]
        fB, fA = _swappable(e - d, e + d, f)
        bB, bA = _swappable(e - d, e + d, b)
        a0, b0 = cf - f, cb - b
        gfun = lambda a, bb: np.where(f > 0, f / (G + bb), (G - a) * b / ((G + bb) * (G + bb + b)))
        gmax, gmin = gfun(a0 - fB, b0 - bB), gfun(np.minimum(a0 + fA, G), b0 + bA)
        slack = np.where(f + b > 0, np.maximum(gmax - gs, gs - gmin), 0.0)
    g, sl = np.empty(n), np.empty(n)
    g[order], sl[order] = gs, slack
    return float((e * gs).sum()), g, sl, np.minimum(1.0, (wf + wb) / G)


def lovasz_items(prob, delta, cnt, hist, want_slack=True, wrong=None, f32keys=False):
    """-> (loss per class, G per class, g [m, k, 2], slack [m, k, 2], gcap [m, k, 2], tied [m, k, 2]: items of non-zero weight that share
    their fp32 key with another item of non-zero weight — an item of weight zero has g = 0 wherever it stands)."""
    m, k = prob.shape
    g, sl, cap, tied = np.zeros((m, k, 2)), np.zeros((m, k, 2)), np.zeros((m, k, 2)), np.zeros((m, k, 2), bool)
    lossc = np.zeros(k)
    for c in range(k):
        err, d, wf, wb = np.empty(2 * m), np.empty(2 * m), np.zeros(2 * m), np.zeros(2 * m)
        err[0::2], err[1::2] = prob[:, c], 1.0 - prob[:, c]
        d[0::2], d[1::2] = delta[:, c], delta[:, c] + U * (1.0 - prob[:, c])
        wb[0::2], wf[1::2] = cnt - hist[:, c], hist[:, c]
        if f32keys:
            err = err.astype(np.float32).astype(np.float64)
        if wrong == "swap_one":
            v = int(np.argmax(hist[:, c] > 0))
            wb[2 * v], wf[2 * v + 1] = wf[2 * v + 1], wb[2 * v]
        if wrong == "w15":
            wf, wb = np.mod(wf, 2 ** 15), np.mod(wb, 2 ** 15)
        lossc[c], gc, sc, cc = lovasz_class(err, d, wf, wb, want_slack, K["SCAN_LANES"] * K["LV_STILE"] if wrong == "carry64" else None)
        g[:, c], sl[:, c], cap[:, c] = gc.reshape(m, 2), sc.reshape(m, 2), cc.reshape(m, 2)
        key, heavy = err.astype(np.float32), wf + wb > 0
        _, inv = np.unique(key, return_inverse=True)
        tied[:, c] = (heavy & (np.bincount(inv, heavy)[inv] > 1)).reshape(m, 2)
    return lossc, hist.sum(0), g, sl, cap, tied


def lovasz_dz(prob, g, sc):
    dp = (g[:, :, 0] - g[:, :, 1]) * sc
    return prob * (dp - (prob * dp).sum(1, keepdims=True)), dp


def ref_lovasz(p, I, wrong=None):
    m, k, C, esz = p["m"], p["n_cls"], p["c"], p["esz"]
    NK = bucket(k)
    W, z, Sz = head_logits(p, I)
    Smax = Sz.max(1)
    prob, _ = softmax64(z)
    Dp, _ = d_counts(C, NK)
    sp = prob * (1 + 2 * Smax)[:, None] + FLOOR
    delta = Dp * U * sp
    cnt, hist = counts_hist(p, I)
    # (saturated and identical-voxel probes: whole runs of keys tie, nothing is compared item by item; a run's sum of g is
    # J(after) - J(before) whatever the order inside it, so the summed gradients of identical voxels carry no slack)
    lossc, G, g, sl, cap, tied = lovasz_items(prob, delta, cnt, hist, p["mode"] == "items" and wrong != "no_slack", wrong)
    present = k if wrong == "absent_in_mean" else int((G > 0).sum())
    R = dict(vals={}, exact={}, zero={}, pred=pred_ref(z, Sz, C, p["family"] == "exact"), tied=tied)
    loss = lossc.sum() / present if present else 0.0
    derr = np.stack([delta, delta + U * (1 - prob)], 2)
    s_loss = (derr * (np.minimum(np.abs(g) + sl, cap) if p["mode"] == "items" else cap)).sum() / max(present, 1) / (Dp * U)
    R["vals"]["out0"] = (loss, s_loss + abs(loss), Dp, 0.0, 0.0)
    R["exact"]["out1"] = np.float64(int((G > 0).sum()))
    R["vals"]["gitem"] = (g, np.abs(g) + FLOOR, 2, sl, 0.0)
    gsum = g.sum((0, 2))
    R["vals"]["gsum"] = (gsum, np.ones(k), 2, 0.0, 0.0)
    R["zero"]["gitem_absent"] = G == 0
    sc = p["grad"] / present if present else 0.0
    dz, dp = lovasz_dz(prob, g, sc)
    adp = (np.abs(g[:, :, 0]) + np.abs(g[:, :, 1])) * abs(sc)
    sdp = (sl[:, :, 0] + sl[:, :, 1]) * abs(sc)
    s_dz = sp * (adp + (prob * adp).sum(1, keepdims=True))
    k_dz = prob * (sdp + (prob * sdp).sum(1, keepdims=True))
    Ddz = Dp + k + 8
    aW = np.abs(W)
    nb = hd_blocks(m)
    bf = BF if esz == 2 else 0.0
    R["vals"]["dz"] = (dz, s_dz, Ddz, k_dz, bf)
    if esz == 2:
        R["vals"]["dz_sum"] = (dz, s_dz, Ddz, k_dz, BF * BF)      # dz + dz_lo
    R["vals"]["d_feats"] = (dz @ W, s_dz @ aW, Ddz + k, k_dz @ aW, bf)
    # the sums carry no ordering slack: inside a run of near-tied keys the reordered g's sum to J(after) - J(before)
    R["vals"]["dbp"] = (block_sum(dz, nb), block_sum(s_dz, nb), Ddz + 35, 0.0, 0.0)
    R["vals"]["db"] = (dz.sum(0), s_dz.sum(0), Ddz + 35, 0.0, 0.0)
    if esz == 2:
        aF = np.abs(I["F"])
        T = div_up(div_up(m, 64), 4 * dw_blocks(m))
        R["vals"]["dW"] = (dz.T @ I["F"], s_dz.T @ aF, Ddz + 2 * (64 * T + 3), (BF * BF + 2 * (64 * T + 3) * U) * (np.abs(dz).T @ aF), 0.0)
    R["allzero"] = ["dz", "d_feats", "dbp"] if present == 0 or p["grad"] == 0 else []
    R["zero"]["dz"] = R["zero"]["d_feats"] = cnt == 0      # (its items have weight 0: g = 0, dp = 0)
    R["skip"] = () if p["mode"] == "items" else ("gitem", "dz", "dz_sum", "d_feats", "dbp")
    return R


def reference(p, I, wrong=None):
    return {"A": ref_head, "C": ref_head, "B": ref_dw, "D": ref_ce, "E": ref_meters, "F": ref_lovasz}[p["group"]](p, I, wrong)


def left_out(p, R):
    """(share of voxels whose pred is undecided, share of Lovasz items with a tied fp32 key)."""
    a = 1.0 - R["pred"]["decided"].mean() if "pred" in R else 0.0
    b = R["tied"].mean() if "tied" in R and p["mode"] == "items" else 0.0
    return float(a), float(b)


# ------------------------------------------------------------------------------------------------------------------ the checks
def round_once(p, R):
    """The reference rounded once to each output's type: what a correctly rounded device would return."""
    got = {}
    for name, (val, _, _, _, bf) in R["vals"].items():
        got[name] = rbf(val) if bf == BF else r32(val)
    for name, val in R["exact"].items():
        got[name] = np.array(val, np.float64)
    if "pred" in R:
        got["pred"] = R["pred"]["top1"].copy()
    if "dz_sum" in got:
        got["dz_sum"] = got["dz"] + rbf(R["vals"]["dz"][0] - got["dz"])
    return got


def ratios(p, R, got):
    """-> ({name: largest (error - slack - bf16 half ulp) / (u scale)}, failures of the exact checks)."""
    out, fails = {}, []
    skip = R.get("skip", ())
    for name, (val, scale, D, slack, bf) in R["vals"].items():
        if name not in got or name in skip:
            continue
        x = np.asarray(got[name], np.float64)
        if x.shape != np.shape(val):
            fails.append("%s: shape %s" % (name, x.shape))
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            err = np.abs(x - val) - slack - bf * np.abs(val)
            ratio = np.where(err > 0, err / (U * scale * (1 + bf)), 0.0)
        if name == "gitem" and p["mode"] == "items":
            ratio = np.where(R["tied"], 0.0, ratio)
        ratio = np.where(np.isfinite(x), ratio, np.inf)
        out[name] = float(np.max(ratio)) if ratio.size else 0.0
    for name, val in R["exact"].items():
        if name in got and not np.array_equal(np.asarray(got[name], np.float64), val):
            fails.append("%s differs: %s, expected %s" % (name, np.asarray(got[name]).reshape(-1)[:4], np.asarray(val).reshape(-1)[:4]))
    for name, rows in R["zero"].items():
        if name == "gitem_absent":
            if "gitem" in got and np.any(np.asarray(got["gitem"])[:, rows] != 0):
                fails.append("gitem of an absent class is not 0")
        elif name in got and np.any(np.asarray(got[name])[rows] != 0):
            fails.append("%s: the row of a voxel without a valid point is not 0" % name)
    for name in R.get("allzero", []):
        if name in got and np.any(np.asarray(got[name]) != 0):
            fails.append("%s is not 0 although every label is ignored or grad = 0" % name)
    if "padzero" in R and "part" in got and np.any(np.asarray(got["part"])[:, R["padzero"]:] != 0):
        fails.append("part: rows of the padding classes are not 0")
    if "pred" in R and "pred" in got:
        q, P = np.asarray(got["pred"]), R["pred"]
        bad = np.where(P["decided"], q != P["top1"], (q != P["top1"]) & (q != P["top2"]))
        if bad.any():
            fails.append("pred differs on %d voxels (first %d: %d, expected %d)" % (bad.sum(), np.argmax(bad), q[np.argmax(bad)], P["top1"][np.argmax(bad)]))
    return out, fails


def judge(R, kr, rr=None):
    """Per output [kernel ratio, fp32 reference path's ratio or None, allowed]; failures where the kernel's exceeds allowed =
    max(4 x the reference path's, the derived operation count)."""
    table, fails = {}, []
    for name, r in kr.items():
        ref = (rr or {}).get(name)
        allowed = max(4 * ref if ref is not None and math.isfinite(ref) else 0.0, float(R["vals"][name][2]))
        table[name] = [r, ref, allowed]
        if not r <= allowed:
            fails.append("%s: error %.4g u scale, allowed %.4g" % (name, r, allowed))
    return table, fails


def check(p, R, got, rr=None):
    kr, fails = ratios(p, R, got)
    table, f2 = judge(R, kr, rr)
    return table, fails + f2


# ------------------------------------------------------------------------------------- the kernels' expressions in numpy float32
f32 = np.float32


def _fma_rows(acc, a, b):
    """acc + a * b with one rounding (the product of two fp32 is exact in fp64)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32)


def emu_logits(F, W, b):
    z = np.zeros((F.shape[0], W.shape[0]), f32)
    for c in range(F.shape[1]):
        z = _fma_rows(z, F[:, c:c + 1].astype(f32), W[None, :, c].astype(f32))
    return z + b.astype(f32)[None]


def emu_softmax(z):
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    s = np.zeros((len(z), 1), f32)
    for k in range(z.shape[1]):
        s = s + e[:, k:k + 1]
    return e, s, mx


def emu_seq(x, nb):
    """A workgroup's sum of x [m, ...] in float32."""
    pad = nb * HD_BLOCK - x.shape[0]
    x = np.concatenate([x, np.zeros((pad,) + x.shape[1:], f32)]) if pad else x
    return x.reshape((nb, HD_BLOCK) + x.shape[1:]).sum(1, dtype=f32)


def emu_back(dz, W, esz):
    df = np.zeros((dz.shape[0], W.shape[1]), f32)
    for k in range(dz.shape[1]):
        df = _fma_rows(df, dz[:, k:k + 1], W[None, k].astype(f32))
    return df


def emulate(p, I):
    """The device's expressions in numpy float32 (accurate exp / log), in the kernels' order of operations where it matters."""
    g, m, k, esz = p["group"], p["m"], p["n_cls"], p["esz"]
    st = lambda x: rstore(x, esz)
    if g == "B":
        F, dz = I["F"].astype(f32), I["dz"].astype(f32)
        blk, grid = dw_block_of(m)
        part = np.zeros((grid, 32, 16), f32)
        for ch in range(div_up(m, 64)):
            part[blk[ch], :k] += dz[ch * 64:(ch + 1) * 64].T @ F[ch * 64:(ch + 1) * 64]
        return dict(part=part, dW=part.astype(np.float64).sum(0)[:k])
    if g == "E":
        return dict(hist=ref_meters(p, I)["exact"]["hist"])
    if g == "D":
        z = I["z"].astype(f32)
        e, s, mx = emu_softmax(z)
        lse = (mx + np.log(s))[:, 0]
        ok = valid_mask(I["labels"], p["ignore"], k)
        y = np.where(ok, I["labels"], 0)
        term = np.where(ok, lse - z[np.arange(m), y], f32(0))
        blk, grid = ce_block_of(m)
        part, cnt = np.zeros(grid, f32), np.zeros(grid, f32)
        np.add.at(part, blk, term)
        np.add.at(cnt, blk, ok.astype(f32))
        n = float(cnt.astype(np.float64).sum())
        sc = f32(p["grad"]) / f32(max(n, 1.0))
        onehot = np.zeros((m, k), f32)
        onehot[np.arange(m), y] = 1
        dl = (np.exp(z - lse[:, None]) - onehot) * sc * ok[:, None]
        return dict(lse=lse, out0=f32(part.astype(np.float64).sum() / max(n, 1.0)), out1=n, part_loss=part, part_cnt=cnt, dlogits=dl)
    z = emu_logits(I["F"], I["Weff"], I["b"])
    e, s, mx = emu_softmax(z)
    out = dict(pred=np.argmax(z, 1))
    if g == "C":
        out["conf"] = (f32(1) / s)[:, 0]
        return out
    W = I["Weff"]
    cnt, hist = counts_hist(p, I)
    nb = hd_blocks(m)
    if g == "A":
        lse = (mx + np.log(s))[:, 0]
        ok = valid_mask(I["labels"], p["ignore"], k)
        term = np.zeros(m, f32)
        np.add.at(term, I["pv"][ok], (lse[I["pv"][ok]] - z[I["pv"][ok], I["labels"][ok]]).astype(f32))
        part, pc = emu_seq(term, nb), emu_seq(cnt.astype(f32), nb)
        n = float(pc.astype(np.float64).sum())
        sc = f32(p["grad"]) / f32(max(n, 1.0))
        dz = (cnt.astype(f32) * sc / s[:, 0])[:, None] * e
        for i in range(int(hist.max())):
            dz = np.where(hist > i, dz - sc, dz)
        out.update(out0=f32(part.astype(np.float64).sum() / max(n, 1.0)), out1=n, part_loss=part, part_cnt=pc, dz=st(dz), d_feats=st(emu_back(dz, W, esz)),
                   dbp=emu_seq(dz, nb))
        out["db"] = out["dbp"].astype(np.float64).sum(0)
        if esz == 2:
            out["dW"] = (out["dz"].T @ I["F"]).astype(f32)
        return out
    # F: the items from the float32 probabilities, J in fp64 over the stable order of the float32 keys
    prob = np.minimum(e / s, f32(1))
    lossc, G, gi, _, _, _ = lovasz_items(prob.astype(np.float64), np.zeros((m, k)), cnt, hist, False, None, True)
    # (1 - p is rounded to float32 on the device: the keys; the loss multiplies the float32 errors)
    present = int((G > 0).sum())
    gi = gi.astype(f32)
    sc = f32(p["grad"]) / f32(present) if present else f32(0)
    dp = (gi[:, :, 0] - gi[:, :, 1]) * sc
    dot = (prob * dp).sum(1, dtype=f32)[:, None]
    dz = prob * (dp - dot)
    out.update(out0=f32(lossc.sum() / present if present else 0.0), out1=float(present), gitem=gi, gsum=gi.astype(np.float64).sum((0, 2)), dz=st(dz),
               d_feats=st(emu_back(dz, W, esz)), dbp=emu_seq(dz, nb))
    out["db"] = out["dbp"].astype(np.float64).sum(0)
    if esz == 2:
        out["dz_sum"] = out["dz"] + rbf(dz.astype(np.float64) - out["dz"])
        out["dW"] = (out["dz_sum"].T @ I["F"]).astype(f32)
    return out


# --------------------------------------------------------------------------------------------------------------- the device run
class Buf:
    """A device array inside a sentinel-filled allocation: GUARD bytes on both sides (`off` more in front: a misaligned base)."""

    def __init__(self, dev, data=None, nbytes=0, off=0):
        import torch
        if data is not None:
            data = data.contiguous()
            nbytes = data.numel() * data.element_size()
        self.lo, self.n = GUARD + off, nbytes
        self.raw = torch.full((self.lo + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        if data is not None and nbytes:
            self.raw[self.lo:self.lo + nbytes] = data.view(-1).view(torch.uint8).to(dev)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lo

    def get(self, dtype, shape=(-1,)):
        return self.raw[self.lo:self.lo + self.n].clone().view(dtype).reshape(shape)

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


def _t(x, esz=None, i=None):
    import torch
    if i is not None:
        return torch.from_numpy(np.ascontiguousarray(x, dtype=i))
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.bfloat16() if esz == 2 else t


def _np(t):
    return t.double().cpu().numpy()


def _twice(call, outs):
    """The call, twice into the same buffers: -> (status, the second call returned the same bits)."""
    import torch
    st = call()
    torch.cuda.synchronize()
    first = [o.raw.clone() for o in outs]
    st2 = call()
    torch.cuda.synchronize()
    return st, st2 == st and all(torch.equal(a, o.raw) for a, o in zip(first, outs))


def _torch_labels(lab, ign, k):
    import torch
    ok = valid_mask(lab, ign, k)
    return torch.from_numpy(np.where(ok, lab, -100))


def ref_path(p, I, dev):
    """The reference model's own fp32 path on the device: torch Linear on the gathered rows, F.cross_entropy / softmax /
    lovasz_softmax(compute_dtype=float32) and autograd.  -> outputs by the names of the references."""
    import torch
    import torch.nn.functional as Fn
    from doda_amd.lovasz import lovasz_softmax
    g, k = p["group"], p["n_cls"]
    if g in ("B", "E"):
        return {}
    if g == "D":
        z = _t(I["z"]).to(dev).requires_grad_()
        lab = _torch_labels(I["labels"], p["ignore"], k).to(dev)
        nv = max(int((lab >= 0).sum()), 1)
        loss = Fn.cross_entropy(z, lab, ignore_index=-100, reduction="sum") / nv
        (loss * p["grad"]).backward()
        return dict(out0=_np(loss.detach()), lse=_np(torch.logsumexp(z.detach(), 1)), dlogits=_np(z.grad))
    f = _t(I["F"]).to(dev).requires_grad_()
    w = _t(I["Weff"]).to(dev)
    b = _t(I["b"]).to(dev).requires_grad_()
    zv = Fn.linear(f, w, b)
    if g == "C":
        return dict(conf=_np(torch.softmax(zv.detach(), 1).max(1).values))
    zv.retain_grad()
    scores = zv[torch.from_numpy(I["pv"]).to(dev)]
    lab = _torch_labels(I["labels"], p["ignore"], k).to(dev)
    if g == "A":
        loss = Fn.cross_entropy(scores, lab, ignore_index=-100, reduction="sum") / max(int((lab >= 0).sum()), 1)
    else:
        loss = lovasz_softmax(scores, lab, -100, compute_dtype=torch.float32)
    if not loss.requires_grad:
        return dict(out0=_np(loss))
    (loss * p["grad"]).backward()
    return dict(out0=_np(loss.detach()), dz=_np(zv.grad), d_feats=_np(f.grad), db=_np(b.grad))


def run_probe(p, dev="cuda:0", want_ref_path=True):
    """Probe p through the C ABI into sentinel-padded buffers -> result dict(id, status, table {output: [kernel ratio, fp32 path's
    ratio, allowed]}, fails, guards, repeat)."""
    import torch
    from doda_amd._lib import lib
    L = lib()
    I = make_inputs(p)
    g, m, k, c, esz = p["group"], p["m"], p["n_cls"], p["c"], p["esz"]
    dt = torch.bfloat16 if esz == 2 else torch.float32
    s = torch.cuda.current_stream().cuda_stream
    B = {}
    fails, got, repeat = [], {}, True
    new = lambda name, nbytes: B.setdefault(name, Buf(dev, nbytes=nbytes))
    if g in ("A", "C", "F"):
        feats, w = Buf(dev, _t(I["F"], esz)), Buf(dev, _t(I["W"]))
        bias = Buf(dev, _t(I["b"])) if p["bias"] else None
        bptr = bias.ptr if bias else None
        v2p, labels = Buf(dev, _t(I["v2p"], i=np.int32)), Buf(dev, _t(I["labels"], i=np.int64))
        ld = I["v2p"].shape[1]
        nb = hd_blocks(m)
        head = (feats.ptr, m, c, esz, w.ptr, bptr, k)
        grad = Buf(dev, torch.tensor([p["grad"]], dtype=torch.float32))
        out, pred = new("out", 8), new("pred", 4 * m)
        dfe, dz, dbp = new("d_feats", m * c * esz), new("dz", m * k * esz), new("dbp", nb * k * 4)
    if g == "A":
        if int(L.doda_head_ce_blocks(m)) != nb:
            fails.append("doda_head_ce_blocks(%d) = %d, restated %d" % (m, L.doda_head_ce_blocks(m), nb))
        nba = nb + 1 if p["what"] == "nblocks" else nb
        ws = new("partial", 8 * nb)
        st, repeat = _twice(lambda: L.doda_head_ce_fwd(*head, v2p.ptr, ld, labels.ptr, p["ignore"], out.ptr, pred.ptr, ws.ptr, nba, s), [out, pred, ws])
        if st == OK:
            st, rep2 = _twice(lambda: L.doda_head_ce_bwd(*head, v2p.ptr, ld, labels.ptr, p["ignore"], out.ptr, grad.ptr, dfe.ptr, dz.ptr, dbp.ptr, nba, s),
                              [dfe, dz, dbp])
            repeat = repeat and rep2
        else:
            st2 = L.doda_head_ce_bwd(*head, v2p.ptr, ld, labels.ptr, p["ignore"], out.ptr, grad.ptr, dfe.ptr, dz.ptr, dbp.ptr, nba, s)
            if st2 != st:
                fails.append("backward status %d, forward %d" % (st2, st))
        if st == OK:
            o, part = out.get(torch.float32), ws.get(torch.float32, (nb, 2))
            got = dict(out0=_np(o[0]), out1=_np(o[1]), pred=pred.get(torch.int32).cpu().numpy(), part_loss=_np(part[:, 0]), part_cnt=_np(part[:, 1]),
                       dz=_np(dz.get(dt, (m, k))), d_feats=_np(dfe.get(dt, (m, c))), dbp=_np(dbp.get(torch.float32, (nb, k))))
            got["db"] = got["dbp"].sum(0)
    elif g == "C":
        conf = new("conf", 4 * m)
        st, repeat = _twice(lambda: L.doda_st_voxel_confidence(feats.ptr, m, c, esz, w.ptr, bptr, k, pred.ptr, conf.ptr, s), [pred, conf])
        if st == OK:
            got = dict(pred=pred.get(torch.int32).cpu().numpy(), conf=_np(conf.get(torch.float32)))
            if c == 16:      # the same bits as the cross-entropy head's argmax
                ws, pred2 = new("partial", 8 * nb), new("pred2", 4 * m)
                st = L.doda_head_ce_fwd(*head, v2p.ptr, ld, labels.ptr, p["ignore"], out.ptr, pred2.ptr, ws.ptr, nb, s)
                torch.cuda.synchronize()
                if st == OK and not torch.equal(pred2.get(torch.int32), pred.get(torch.int32)):
                    fails.append("pred differs from doda_head_ce_fwd's")
    elif g == "F":
        P = lv_plan(m, k)
        if int(L.doda_lovasz_blocks(m)) != nb:
            fails.append("doda_lovasz_blocks(%d) restated %d" % (m, nb))
        nbytes = int(L.doda_lovasz_workspace_bytes(m, k))
        if nbytes <= 0 or nbytes != P["bytes"]:
            fails.append("doda_lovasz_workspace_bytes = %d, restated %d" % (nbytes, P["bytes"]))
        ws, gitem = new("ws", max(nbytes, 256)), new("gitem", m * k * 8)
        dzlo = new("dz_lo", m * k * esz) if esz == 2 else None
        fwd_outs = [out, pred, gitem]
        st, repeat = _twice(lambda: L.doda_lovasz_fwd(*head, v2p.ptr, ld, labels.ptr, p["ignore"], out.ptr, pred.ptr, gitem.ptr, ws.ptr, nbytes, s), fwd_outs)
        if st == OK:
            st, rep2 = _twice(lambda: L.doda_lovasz_bwd(*head, gitem.ptr, out.ptr, grad.ptr, dfe.ptr, dz.ptr, dzlo.ptr if dzlo else None, dbp.ptr, nb, s),
                              [dfe, dz, dbp] + ([dzlo] if dzlo else []))
            repeat = repeat and rep2
            o = out.get(torch.float32)
            got = dict(out0=_np(o[0]), out1=_np(o[1]), pred=pred.get(torch.int32).cpu().numpy(), gitem=_np(gitem.get(torch.float32, (m, k, 2))),
                       dz=_np(dz.get(dt, (m, k))), d_feats=_np(dfe.get(dt, (m, c))), dbp=_np(dbp.get(torch.float32, (nb, k))))
            got["gsum"], got["db"] = got["gitem"].sum((0, 2)), got["dbp"].sum(0)
            if esz == 2:
                got["dz_sum"] = got["dz"] + _np(dzlo.get(dt, (m, k)))
    if g in ("A", "F") and esz == 2 and st == OK:      # dW through head_dw_bf16 on the sweep's own dz (and dz_lo)
        nbw = dw_blocks(m)
        part = new("dw_part", nbw * 512 * 4)
        got["dW"] = 0.0
        for operand in [dz] + ([dzlo] if g == "F" else []):
            st = L.doda_head_dw_bf16(feats.ptr, operand.ptr, m, 16, k, part.ptr, nbw, s)
            torch.cuda.synchronize()
            got["dW"] = got["dW"] + _np(part.get(torch.float32, (nbw, 32, 16))).sum(0)[:k]
    if g == "B":
        off_f, off_z = (8 if p["what"] == "falign" else 0), (2 if p["what"] == "dzalign" else 0)
        feats, dzb = Buf(dev, _t(I["F"], 2), off=off_f), Buf(dev, _t(I["dz"], 2), off=off_z)
        nbw = dw_blocks(m)
        if int(L.doda_head_dw_blocks(m)) != nbw:
            fails.append("doda_head_dw_blocks(%d) = %d, restated %d" % (m, L.doda_head_dw_blocks(m), nbw))
        part = new("part", nbw * 512 * 4)
        st, repeat = _twice(lambda: L.doda_head_dw_bf16(feats.ptr, dzb.ptr, m, 16, k, part.ptr, nbw, s), [part])
        if st == OK:
            got = dict(part=_np(part.get(torch.float32, (nbw, 32, 16))))
            got["dW"] = got["part"].sum(0)[:k]
    elif g == "D":
        z, labels = Buf(dev, _t(I["z"])), Buf(dev, _t(I["labels"], i=np.int64))
        nb = ce_blocks(m)
        wsb = int(L.doda_cross_entropy_workspace_bytes(m))
        if wsb != align_up(nb * 8, 256):
            fails.append("doda_cross_entropy_workspace_bytes = %d, restated %d" % (wsb, align_up(nb * 8, 256)))
        grad = Buf(dev, torch.tensor([p["grad"]], dtype=torch.float32))
        lse, out, ws, dl = new("lse", 4 * m), new("out", 8), new("ws", wsb), new("dlogits", 4 * m * c)
        st, repeat = _twice(lambda: L.doda_cross_entropy_fwd(z.ptr, labels.ptr, m, c, p["ignore"], lse.ptr, out.ptr, ws.ptr, wsb, s), [lse, out, ws])
        if st == OK:
            st, rep2 = _twice(lambda: L.doda_cross_entropy_bwd(z.ptr, labels.ptr, lse.ptr, out.ptr, grad.ptr, m, c, p["ignore"], dl.ptr, s), [dl])
            repeat = repeat and rep2
            o, part = out.get(torch.float32), ws.get(torch.float32)[:2 * nb].reshape(nb, 2)
            got = dict(out0=_np(o[0]), out1=_np(o[1]), lse=_np(lse.get(torch.float32)), part_loss=_np(part[:, 0]), part_cnt=_np(part[:, 1]),
                       dlogits=_np(dl.get(torch.float32, (m, c))))
    elif g == "E":
        preds = Buf(dev, _t(I["preds"], i=np.int64 if p["p64"] else np.int32))
        p2v = Buf(dev, _t(I["p2v"], i=np.int32)) if p["p2v"] else None
        labels = Buf(dev, _t(I["labels"], i=np.int64))
        hist = B.setdefault("hist", Buf(dev, _t(I["hist0"], i=np.int64)))
        for _ in range(2):      # two accumulating calls
            st = L.doda_seg_meters(preds.ptr, p["p64"], p2v.ptr if p2v else None, labels.ptr, m, k, p["ignore"], hist.ptr, s)
        torch.cuda.synchronize()
        if st == OK:
            got = dict(hist=_np(hist.get(torch.int64)))
    torch.cuda.synchronize()
    res = dict(id=p["id"], status=int(st), table={}, fails=fails, guards=all(b.intact() for b in B.values()), repeat=bool(repeat))
    if st != p["status"]:
        fails.append("status %d, expected %d" % (st, p["status"]))
    elif p["status"]:
        if not all(b.untouched() for n, b in B.items() if n != "hist"):
            fails.append("an error return wrote to an output")
    else:
        R = reference(p, I)
        rr = None
        if want_ref_path:
            rr, _ = ratios(p, R, ref_path(p, I, dev))
        res["table"], more = check(p, R, got, rr)
        fails += more
        missing = [n for n in list(R["vals"]) + list(R["exact"]) if n not in got]
        if missing:
            fails.append("outputs not produced: %s" % missing)
    if not res["guards"]:
        fails.append("a sentinel around an output or the workspace was overwritten")
    if not repeat:
        fails.append("a repeated call returned other bits")
    return res


def profile(files):
    """The table of profiles/r19_head_numerics.txt from the result lines of --numerics runs."""
    print("# probe | per output: kernel ratio / fp32 reference path's ratio / allowed (all in units of u x scale) | largest kernel ratio")
    worst, n = {}, 0
    for f in files:
        for l in open(f):
            if l.startswith("{") and '"id"' in l:
                r = json.loads(l)
                n += 1
                for k, v in r["table"].items():
                    if v[0] / v[2] >= worst.get((r["id"][0], k), (-1.0,))[0]:
                        worst[(r["id"][0], k)] = (v[0] / v[2], v, r["id"])
                cell = lambda v: "-" if v is None else "%.3g" % v
                print("%s | %s | %s%s" % (r["id"], " ".join("%s %s/%s/%s" % (k, cell(v[0]), cell(v[1]), cell(v[2])) for k, v in r["table"].items())
                                          or "status %d" % r["status"], cell(max([v[0] for v in r["table"].values()], default=0.0)),
                                          " FAILS " + "; ".join(r["fails"]) if r["fails"] else ""))
    print("# %d probes, %d kernels; the largest kernel ratio / allowed per group and output:" % (n, len({k for p in probes() for k in kernels(p)})))
    for (g, k), (share, v, pid) in sorted(worst.items()):
        print("#   %s %-9s %.3g of %.3g (%.3f)  fp32 path %s  %s" % (g, k, v[0], v[2], share, "-" if v[1] is None else "%.3g" % v[1], pid))


if __name__ == "__main__":
    if sys.argv[1] == "--numerics":
        sys.path.insert(0, ROOT)
        for p in probes(sys.argv[2] if len(sys.argv) > 2 else None):
            print(json.dumps(run_probe(p)), flush=True)
    elif sys.argv[1] == "--list":
        for p in probes(sys.argv[2] if len(sys.argv) > 2 else None):
            print(p["id"], kernels(p))
    elif sys.argv[1] == "--profile":
        profile(sys.argv[2:])

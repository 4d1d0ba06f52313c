"""Numerics probes of doda_spconv_gather_ex: one call per kernel instantiation that the route plan (csrc/gather_plan.hpp) can reach,
each compared with an fp64 reference (tools/gatherroutes.py --numerics GROUP; tests/test_gpu_gather_numerics.py).

The probe list is GENERATED from the plan: `space()` walks the calls, the host planner (tests/host/gather_plan_main.cpp) names the
route of each, `select()` keeps per route the call of fewest output rows and `shape()` moves it to the smallest shape at which the
kernel can still go wrong (a ragged last wave tile, a second tile, idle persistent workgroups).  tests/data/gather_numerics.json is
that list as recorded; tests/test_gather_plan_host.py regenerates it and asserts equality, and that the names it reaches, the names
the predicates of gather_plan.hpp admit and tests/data/gather_instantiations.json (what is compiled) are one set of 247.

The checkers (`reference`, `check`) are plain torch on whatever device the tensors are on: tests/test_gather_numerics_host.py feeds
them the rounded reference and corrupted copies of it on the CPU.

The second half of this file holds the probes of the LDS-staged kernels over DESIGNED tilebooks (tests/data/gather_tile_class.json;
`python tools/gathernumerics.py --tile-class PLANNER` prints that file's content)."""
import ctypes as C
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = os.path.join(ROOT, "tests", "data", "gather_numerics.json")

SWITCHES = ("tile", "wlds", "tile_pipeline", "tile_dual", "conv_up", "f32_conv_tile")
OPT = {"tile": 1, "wlds": 2, "tile_pipeline": 4, "tile_dual": 5, "conv_up": 6}     # doda_set_option; f32_conv_tile: DODA_F32_CONV_TILE
PLANE = (25, 12)            # 300 voxels: one full 256-row tile and one of 44 rows; six of eight persistent workgroups own no tile
PLANE16 = (443, 444)        # 769 tiles (196 692 rows): conv_tile16
GROUPS = ("generic", "fast.bf16.nb1", "fast.bf16.nb2", "fast.bf16.nb3", "fast.bf16.nb4", "fast.bf16.nb6", "fast.f32", "prologue",
          "tile", "tile16", "staged", "f32split")
# bounds of the existing tests: y (test_gpu_gather_routes.py, test_gpu_tile.py), statistics (test_gpu_round2.py), side and the
# parameter gradients (test_gpu_layers.py)
Y_TOL = {True: 1e-4, False: 2.0 ** -7}                      # by "y is fp32"
STATS_TOL = 1e-5
SIDE_TOL = {(1, 2): 2.0 ** -7, (1, 4): 2e-5, (2, 2): 2.0 ** -6, (2, 4): 2e-4, (3, 2): 2.0 ** -6, (3, 4): 2e-4}   # by (kind, esz)
PARAM_RTOL = 2e-3
MARGIN = 0.05               # |xhat gamma + beta| of every element of a BatchNorm-backward operand: the input decides the ReLU mask
EPS, MOMENTUM = 1e-4, 0.1


# ---------------------------------------------------------------------------------------------------------------- the probe list
def sweep_rows():
    """Row counts on both sides of every threshold of the plan (in 16-row wave tiles, divided by the channel blocks)."""
    rows = {1, 2, 16, 17, 37, 8191, 8192, 8193, 196608, 196609, 262144, 262145, 300000}
    for wf in (170, 171, 256, 341, 342, 512, 682, 683, 1024, 2048, 4096, 8192, 12288, 16384):
        rows |= {16 * (wf - 1), 16 * (wf - 1) + 1, 16 * wf, 16 * wf + 1}
    return sorted(rows)


def space(rows=None):
    """The calls of the extended sweep as dicts (the keys of plan_line below)."""
    for n in rows or sweep_rows():
        for K in (1, 8, 27):
            for kc in (3, 8, 16, 32, 48, 64):     # 8: the narrow bf16 fragments (PBF16) with enough units for split blocks
                for nc in (16, 32, 48, 64, 96):
                    for esz, out32 in ((2, 0), (2, 1), (4, 0)):
                        for stats in (0, 1):
                            base = dict(K=K, kc=kc, nc=nc, esz=esz, n_out=n, n_in=n, out32=out32, stats=stats, tilebook=0, pre=0,
                                        res_bcast=0, off=(), f32split=0)
                            var = [base, dict(base, res_bcast=1)]
                            if K == 8:
                                var += [dict(v, n_in=n // 4 + 1) for v in list(var)]
                            if K == 27 and kc in (16, 32):
                                var += [dict(v, tilebook=1) for v in list(var)]
                            if (kc == 16 and esz == 4) or kc == 32:
                                var += [dict(base, pre=kind) for kind in (1, 2, 3)]
                            for v in var:
                                yield v
                                # (a switch acts on calls with a tilebook, 48 channels or a K <= 8 table only: gather_plan.hpp)
                                if v["tilebook"] or kc == 48 or (K == 8 and kc == 32):
                                    for sw in SWITCHES:
                                        yield dict(v, off=(sw,))
                                if esz == 4:
                                    yield dict(v, f32split=1)


def plan_line(c):
    kv = dict(K=c["K"], kc=c["kc"], nc=c["nc"], esz=c["esz"], n_out=c["n_out"], n_in=c["n_in"], ld=c.get("ld", c["n_out"]),
              out32=c["out32"], stats=c["stats"], res_bcast=c["res_bcast"], pre_kind=c["pre"], tilebook=int(bool(c["tilebook"])))
    for o in c["off"]:
        kv["sw." + o] = 0
    if c["f32split"]:
        kv["sw.f32_split_rows"] = 0
    return " ".join("%s=%d" % it for it in kv.items())


def _simplest(c):
    """Order among the calls that reach one route: fewest output rows; then default switches, a dense residual, no tilebook the
    route does not need; then the larger K, kc and nc (more units per wave tile, more channel blocks per workgroup)."""
    return (c["n_out"], len(c["off"]), c["f32split"], c["res_bcast"], c["tilebook"], c["n_in"] != c["n_out"], -c["K"], -c["kc"], -c["nc"],
            c["out32"], c["stats"], c["pre"])


def select(calls, routes):
    """Per route name the simplest call that reaches it."""
    best = {}
    for c, r in zip(calls, routes):
        if r["status"] == 0 and (r["route"] not in best or _simplest(c) < _simplest(best[r["route"]])):
            best[r["route"]] = c
    return best


def group_of(route, c):
    if c["f32split"]:
        return "f32split"
    fam = re.match(r"\w+", route).group(0)
    if fam == "conv_gather":
        return "generic"
    if fam == "conv_fast":
        if c["pre"]:
            return "prologue"
        return "fast.f32" if c["esz"] == 4 else "fast.bf16.nb%d" % ((c["nc"] + 15) // 16)
    return {"conv_tile": "tile", "conv_tile16": "tile16"}.get(fam, "staged")


def shape(route, c):
    """Candidate shapes of the probe of `route`, most wanted first; the first for which the planner still names `route` is taken."""
    fam = re.match(r"\w+", route).group(0)
    out = []
    if fam == "conv_tile16":
        n = PLANE16[0] * PLANE16[1]
        out.append(dict(c, n_out=n, n_in=n + 5, ld=n + 3, tilebook="plane16"))
    elif fam == "conv_tile":
        n = PLANE[0] * PLANE[1]
        out.append(dict(c, n_out=n, n_in=n + 5, ld=n + 3, tilebook="plane"))
    elif fam == "conv_wlds48":
        out.append(dict(c, n_out=8193, n_in=8198, ld=8196))
    elif fam == "conv_up32":
        out.append(dict(c, n_out=2049, n_in=513, ld=2052))
    else:
        n = max(c["n_out"], 37)
        if c["tilebook"]:       # a tilebook the route passes by (a switch is off, or the statistics do not fit): still a real one
            for pn, (a, b) in (("plane", PLANE), ("plane16", PLANE16)):
                if a * b >= c["n_out"]:
                    out.append(dict(c, n_out=a * b, n_in=a * b + 5, ld=a * b + 3, tilebook=pn))
        else:
            n_in = n + 5 if c["n_in"] >= c["n_out"] else n // 4 + 1
            out += [dict(c, n_out=n, n_in=n_in, ld=n + 3), dict(c, n_out=c["n_out"], n_in=n_in, ld=c["n_out"] + 3)]
    return out + [dict(c, ld=c["n_out"])]


def generate(ask, produced=None):
    """The probe list; `produced` (a set) receives every route name of the sweep.  `ask` maps planner lines to dicts with status,
    route, grid, block, parts (the `planner` fixture of tests/test_gather_plan_host.py)."""
    calls = list(space())
    got = ask([plan_line(c) for c in calls])
    if produced is not None:
        produced.update(g["route"] for g in got if g["status"] == 0)
    best = select(calls, got)
    routes = sorted(best)
    cands = [shape(r, best[r]) for r in routes]
    flat = iter(ask([plan_line(c) for cs in cands for c in cs]))
    probes = []
    for route, cs in zip(routes, cands):
        got = [next(flat) for _ in cs]
        k = next(k for k, g in enumerate(got) if g["status"] == 0 and g["route"] == route)
        c = cs[k]
        # (DODA_F32_CONV_TILE is read from the environment once: a probe that needed it off would need a child of its own)
        assert c["tilebook"] in (0, "plane", "plane16") and "f32_conv_tile" not in c["off"], (route, c)
        p = dict(route=route, group=group_of(route, c), grid=got[k]["grid"], parts=got[k]["parts"])
        p.update((key, c[key]) for key in ("K", "kc", "nc", "esz", "n_out", "n_in", "ld", "out32", "stats", "tilebook", "pre", "res_bcast",
                                           "f32split"))
        p["off"] = list(c["off"])
        probes.append(p)
    return probes


def load_probes():
    return json.load(open(PROBES))


# ------------------------------------------------------------------------------------------- operands, fp64 reference and checks
G = 16                      # guard rows before and after every operand that is a slice of a larger buffer
SENTINEL = 0x5a             # the byte pattern of output guards; the guards of x hold NaN


def storage(p):
    import torch
    return torch.float32 if p["esz"] == 4 else torch.bfloat16


def y_dtype(p):
    import torch
    return torch.float32 if (p["esz"] == 4 or p["out32"]) else torch.bfloat16


def guarded(rows, cols, dtype, dev):
    """[G + rows + G, cols] filled with the sentinel byte; `inner` is the operand."""
    import torch
    buf = torch.empty((rows + 2 * G, cols), dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(SENTINEL)
    return buf


def inner(buf):
    return buf[G:buf.shape[0] - G]


def intact(buf, written=None):
    """The guard rows of `buf` (and the operand's rows from `written` on) still hold the sentinel."""
    import torch
    rows = buf.shape[0] - 2 * G if written is None else written
    b = buf.view(torch.uint8)
    return bool((b[:G] == SENTINEL).all()) and bool((b[G + rows:] == SENTINEL).all())


def scale_err(a, b):
    """Largest difference relative to the largest reference value (tests/test_gpu_layers.py _scale_err); NaN stays NaN."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def close_ratio(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|): at most 1 where torch.allclose(a, b, rtol, atol) holds."""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / (atol + rtol * b.abs())).max())


def bn_front(u, mean, invstd, gamma, beta):
    """xhat and the ReLU mask of a BatchNorm-backward operand in fp64; every |xhat gamma + beta| keeps the margin, so that the
    input decides the mask and not an fp32 rounding."""
    xh = (u.double() - mean.double()) * invstd.double()
    v = xh * gamma.double() + beta.double()
    assert float(v.abs().min()) >= MARGIN, float(v.abs().min())
    return xh, (v > 0).double()


def margin_rows(g, rows, mean, invstd, gamma, beta, dtype):
    """Rows u = mean + xhat / invstd in `dtype` with |xhat gamma + beta| >= MARGIN for every element AFTER the rounding."""
    import torch
    mean, invstd, gamma, beta = (t.double() for t in (mean, invstd, gamma, beta))
    xhat = torch.randn(rows, mean.numel(), generator=g).double()
    for _ in range(8):
        u = (mean + xhat / invstd).to(dtype)
        xhat = (u.double() - mean) * invstd
        v = xhat * gamma + beta
        near = v.abs() < 2 * MARGIN
        if not bool(near.any()):
            break
        sign = torch.where(v >= 0, 1.0, -1.0).double()
        xhat = torch.where(near, (sign * 3 * MARGIN - beta) / gamma, xhat)
    assert float(v.abs().min()) >= MARGIN
    return u


def make_inputs(p, form, dev, tbl=None):
    """The operands of probe `p` (statistics form "y": (sum y, sum y^2); "bn": the BatchNorm-backward sums) on `dev`, drawn on the
    CPU from a generator seeded by the route's name.  `tbl`: the [K, ld] table of a raster plane (tilebook routes); else a random
    table with absent neighbours and rows that have none at all."""
    import zlib
    import torch
    g = torch.Generator().manual_seed(zlib.crc32(("%s %s" % (p["route"], form)).encode()))
    K, kc, nc, n_out, n_in, ld = p["K"], p["kc"], p["nc"], p["n_out"], p["n_in"], p["ld"]
    dt, ydt = storage(p), y_dtype(p)
    rnd = lambda *s: torch.randn(*s, generator=g)
    uni = lambda *s: torch.rand(*s, generator=g)
    I = {}
    if tbl is None:
        t = torch.randint(0, n_in, (K, ld), generator=g, dtype=torch.int32)
        t[uni(K, ld) < 0.25] = -1
        t[:, uni(ld) < 0.1] = -1
        tbl = t.to(dev)
    I["tbl"] = tbl
    I["w"] = (rnd(K, kc, nc) * 0.1).bfloat16().float().to(dev)      # bf16-representable: products exact
    I["res"] = (rnd(nc) if p["res_bcast"] else rnd(n_out, nc)).to(ydt).to(dev)
    kind = p["pre"]
    if kind == 0:
        I["x"] = rnd(n_in, kc).to(dt).to(dev)
    else:
        gamma, beta = uni(kc) + 0.5, rnd(kc) * 0.3
        if kind == 1:
            x = (rnd(n_in, kc) * 1.7 + 0.3).to(dt)
            xd = x.double()
            I.update(x=x, rm0=rnd(kc) * 0.1, rv0=uni(kc) + 0.5, s1=xd.sum(0), s2=(xd * xd).sum(0))     # real totals: fp64 column sums
        else:
            mean, invstd = rnd(kc) * 0.2, uni(kc) * 0.45 + 0.8
            aux = margin_rows(g, n_in, mean, invstd, gamma, beta, dt)
            x = rnd(n_in, kc).to(dt)                                    # dz
            xh, mask = bn_front(aux, mean, invstd, gamma, beta)
            dzm = x.double() * mask
            I.update(x=x, aux=aux, mean=mean, invstd=invstd, s1=dzm.sum(0), s2=(dzm * xh).sum(0))
            if kind == 3:
                I["add"] = rnd(n_in, kc).to(dt)
        I.update(gamma=gamma, beta=beta)
    if form == "bn":
        I.update(bn_gamma=uni(nc) + 0.5, bn_beta=rnd(nc) * 0.3, bn_mean=rnd(nc) * 0.2, bn_invstd=uni(nc) * 0.45 + 0.8)
        I["bn_x"] = margin_rows(g, n_out, I["bn_mean"], I["bn_invstd"], I["bn_gamma"], I["bn_beta"], ydt)
    return {k: v.to(dev) for k, v in I.items()}


def conv64(operand, w, tbl, n_out):
    """sum_o operand[tbl[o][t]] . w[o] in fp64: per offset index_select, then matmul."""
    import torch
    ref = torch.zeros(n_out, w.shape[2], dtype=torch.float64, device=operand.device)
    for o in range(w.shape[0]):
        t = tbl[o, :n_out].long()
        ref += (operand.index_select(0, t.clamp(min=0)) * (t >= 0).unsqueeze(1)) @ w[o].double()
    return ref


def side64(p, I):
    """The folded BatchNorm in fp64 (csrc/bn_totals.hpp): the rows the gather multiplies (`side`) and the vectors the launch publishes."""
    import torch
    m = p["n_in"]
    ga, be, x = I["gamma"].double(), I["beta"].double(), I["x"].double()
    if p["pre"] == 1:
        mean = I["s1"] / m
        var = (I["s2"] / m - mean * mean).clamp(min=0)
        invstd = 1.0 / torch.sqrt(var + EPS)
        return dict(side=torch.relu((x - mean) * invstd * ga + be), mean=mean, invstd=invstd,
                    rm=(1 - MOMENTUM) * I["rm0"].double() + MOMENTUM * mean,
                    rv=(1 - MOMENTUM) * I["rv0"].double() + MOMENTUM * var * m / max(m - 1, 1))
    xh, mask = bn_front(I["aux"], I["mean"], I["invstd"], I["gamma"], I["beta"])
    du = ga * I["invstd"].double() * (x * mask - I["s1"] / m - xh * (I["s2"] / m))
    if p["pre"] == 3:
        du = du + I["add"].double()
    return dict(side=du, dgamma=I["s2"], dbeta=I["s1"])


def stats_addends(p, form, I, y):
    """The two fp64 addends of every STORED element of y: (y, y^2), or the BatchNorm-backward pair (dz, dz xhat)."""
    yd = y.double()
    if form == "bn":
        xh, mask = bn_front(I["bn_x"], I["bn_mean"], I["bn_invstd"], I["bn_gamma"], I["bn_beta"])
        dz = yd * mask
        return dz, dz * xh
    return yd, yd * yd


def stats64(p, form, I, y):
    """[2, nc] fp64 sums over the STORED y: (sum y, sum y^2), or the BatchNorm-backward pair (sum dz, sum dz xhat)."""
    import torch
    a1, a2 = stats_addends(p, form, I, y)
    return torch.stack([a1.sum(0), a2.sum(0)])


def check(p, form, I, O):
    """The measured errors of one call's outputs `O` (y, stats rows or None, side, published vectors, guards: name -> intact)
    and the list of bounds they miss (empty: the call passes)."""
    import torch
    err, fails = {}, []
    f32 = y_dtype(p) == torch.float32

    def bound(name, value, tol):
        err[name] = value
        if not value < tol:
            fails.append("%s %.3g >= %.3g" % (name, value, tol))

    operand = I["x"].double()
    if p["pre"]:
        R = side64(p, I)
        bound("side", scale_err(O["side"], R["side"]), SIDE_TOL[(p["pre"], p["esz"])])
        if p["pre"] == 1:      # ReLU: no stored value is negative
            bound("side_neg", float((-O["side"].double()).clamp(min=0).max()), 1e-30)
            for k in ("mean", "invstd", "rm", "rv"):
                bound(k, close_ratio(O[k], R[k], 1e-4, 1e-5), 1.0 + 1e-9)
            bound("nbt", abs(int(O["nbt"]) - 1), 0.5)
        else:
            for k in ("dgamma", "dbeta"):
                bound(k, close_ratio(O[k], R[k], PARAM_RTOL, PARAM_RTOL * float(R[k].abs().max())), 1.0 + 1e-9)
        operand = O["side"].double()       # y against the convolution of the STORED rows
    res = I["res"].double()
    bound("y", scale_err(O["y"], conv64(operand, I["w"], I["tbl"], p["n_out"]) + res), Y_TOL[f32])
    if p["stats"]:
        want = stats64(p, form, I, O["y"])
        got = O["stats"].double().sum(0)
        bound("stats0", scale_err(got[0], want[0]), STATS_TOL)
        bound("stats1", scale_err(got[1], want[1]), STATS_TOL)
    broken = sorted(k for k, ok in O["guards"].items() if not ok)
    err["guards"] = not broken
    if broken:
        fails.append("guards overwritten: " + ", ".join(broken))
    return err, fails


def ideal_outputs(p, form, I):
    """What a correct kernel stores: the fp64 reference rounded once to the storage types, every operand inside guards (CPU tests)."""
    import torch
    dev = I["x"].device
    O, bufs = {}, {}

    def put(name, value, dtype):
        value = value.reshape(-1, value.shape[-1]) if value.dim() > 1 else value.reshape(1, -1)
        bufs[name] = guarded(value.shape[0], value.shape[1], dtype, dev)
        inner(bufs[name]).copy_(value.to(dtype))
        return inner(bufs[name])
    operand = I["x"].double()
    if p["pre"]:
        R = side64(p, I)
        O["side"] = put("side", R["side"], storage(p))
        operand = O["side"].double()
        for k in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta"):
            if k in R:
                O[k] = put(k, R[k], torch.float32)[0]
        O["nbt"] = 1
    O["y"] = put("y", conv64(operand, I["w"], I["tbl"], p["n_out"]) + I["res"].double(), y_dtype(p))
    O["stats"] = None
    if p["stats"]:      # one row per 16 output rows
        rows = [stats64(p, form, {k: (v[r:r + 16] if k == "bn_x" else v) for k, v in I.items()}, O["y"][r:r + 16])
                for r in range(0, p["n_out"], 16)]
        O["stats"] = put("stats", torch.stack(rows).reshape(len(rows), -1), torch.float32).view(len(rows), 2, p["nc"])
    O["bufs"] = bufs
    O["guards"] = {k: intact(b) for k, b in bufs.items()}
    return O


# --------------------------------------------------------------------------------------------------------------- the device run
def _with_trace(call):
    """`call()` with the library's trace lines (file descriptor 2) captured: (result, text); the text is passed on to stderr."""
    import sys
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            result = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    sys.stderr.write(text)
    return result, text


def run_group(group):
    """Every probe of `group` once per statistics form, in this process: one JSON line per call.  Ends with status 1 at the first
    call that does not return DODA_OK (a HIP error raises at the synchronisation that follows the call)."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gatherroutes as gr
    from doda_amd import ops
    from doda_amd._lib import lib
    if group in TILE_GROUPS:
        return run_tile_group(group)
    assert group in GROUPS, group
    assert os.environ.get("DODA_TRACE_GATHER") == "1" and os.environ.get("DODA_F32_SPLIT_ROWS") == ("0" if group == "f32split" else None)
    dev = torch.device("cuda:0")
    L = lib()
    planes = {}

    def plane(name, ld):
        if name not in planes:
            a, b = PLANE if name == "plane" else PLANE16
            i, j = torch.meshgrid(torch.arange(a), torch.arange(b), indexing="ij")
            idx = torch.stack([torch.zeros(a * b, dtype=torch.long), i.reshape(-1) + 1, j.reshape(-1) + 1, torch.full((a * b,), 2)], 1)
            t = ops.rulebook_subm(idx.int().to(dev), [a + 2, b + 2, 4], 1, 3)
            tbl = torch.full((t.shape[0], ld), -1, dtype=torch.int32, device=dev)
            tbl[:, :a * b] = t[:, :a * b]
            planes[name] = (tbl, ops.tilebook_build(tbl, a * b))
        assert planes[name][0].shape[1] == ld
        return planes[name]

    for p in load_probes():
        if p["group"] != group:
            continue
        for form in (("y", "bn") if p["stats"] else ("y",)):
            K, kc, nc, esz, n_out, n_in = p["K"], p["kc"], p["nc"], p["esz"], p["n_out"], p["n_in"]
            tbl, tb = plane(p["tilebook"], p["ld"]) if p["tilebook"] else (None, None)
            I = make_inputs(p, form, dev, tbl)
            dt, ydt = storage(p), y_dtype(p)
            xbuf = torch.full((n_in + 2 * G, kc), float("nan"), dtype=dt, device=dev)
            inner(xbuf).copy_(I["x"])
            bufs = {"y": guarded(n_out, nc, ydt, dev)}
            need = int(L.doda_spconv_gather_workspace_bytes(K, kc, nc, esz))
            bufs["ws"] = guarded(need // 256, 256, torch.uint8, dev)
            ep = ops._ConvEpilogue()
            ep.residual, ep.residual_bcast = I["res"].data_ptr(), p["res_bcast"]
            rows = C.c_int32(-1)
            if p["stats"]:
                bufs["stats"] = guarded(int(L.doda_spconv_stats_capacity(n_out)), 2 * nc, torch.float32, dev)
                ep.stats, ep.stats_rows_h = inner(bufs["stats"]).data_ptr(), C.pointer(rows)
                if form == "bn":
                    ep.bn_x, ep.bn_relu = I["bn_x"].data_ptr(), 1
                    ep.bn_mean, ep.bn_invstd, ep.bn_gamma, ep.bn_beta = (I[k].data_ptr() for k in ("bn_mean", "bn_invstd", "bn_gamma", "bn_beta"))
            if tb is not None:
                ep.tilebook, ep.tilebook_rows = tb.data_ptr(), n_out
            keep = []
            if p["pre"]:
                q = gr._Prologue()
                vec = lambda name: inner(bufs.setdefault(name, guarded(1, kc, torch.float32, dev)))[0]
                tot = torch.zeros((8, 2, kc // 4, 16), dtype=torch.float64, device=dev)
                tot[0, 0, :, :4], tot[0, 1, :, :4] = I["s1"].view(-1, 4), I["s2"].view(-1, 4)       # slot 0
                bufs["side"] = guarded(n_in, kc, dt, dev)
                q.kind, q.relu, q.rows, q.totals, q.eps, q.momentum = p["pre"], 1, n_in, tot.data_ptr(), EPS, MOMENTUM
                q.gamma, q.beta = I["gamma"].data_ptr(), I["beta"].data_ptr()
                q.side, q.side_ld, q.aux_ld, q.add_ld = inner(bufs["side"]).data_ptr(), kc, kc, kc
                if p["pre"] == 1:
                    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
                    vec("rm").copy_(I["rm0"])
                    vec("rv").copy_(I["rv0"])
                    q.running_mean, q.running_var, q.num_batches_tracked = vec("rm").data_ptr(), vec("rv").data_ptr(), nbt.data_ptr()
                    q.mean, q.invstd = vec("mean").data_ptr(), vec("invstd").data_ptr()
                else:
                    q.mean, q.invstd, q.aux = I["mean"].data_ptr(), I["invstd"].data_ptr(), I["aux"].data_ptr()
                    q.dgamma, q.dbeta = vec("dgamma").data_ptr(), vec("dbeta").data_ptr()
                    if p["pre"] == 3:
                        q.add = I["add"].data_ptr()
                keep += [q, tot]
                ep.prologue = C.addressof(q)
            for o in p["off"]:
                L.doda_set_option(OPT[o], 0)
            st, text = _with_trace(lambda: L.doda_spconv_gather_ex(
                inner(xbuf).data_ptr(), n_in, kc, esz, I["w"].data_ptr(), nc, I["tbl"].data_ptr(), p["ld"], K, n_out, inner(bufs["y"]).data_ptr(),
                p["out32"], 0, inner(bufs["ws"]).data_ptr(), need, C.byref(ep), None))
            for o in p["off"]:
                L.doda_set_option(OPT[o], 1)
            torch.cuda.synchronize()
            m = re.search(r" route=(.*) grid=(\d+) block=\d+ parts=(\d+)$", text, re.M)
            out = dict(want=p["route"], route=m[1] if m else None, grid=int(m[2]) if m else -1, form=form, status=st, rows=rows.value,
                       shape={k: p[k] for k in ("K", "kc", "nc", "esz", "n_out", "n_in", "out32", "stats", "pre")})
            if st != 0:
                print(json.dumps(out), flush=True)
                sys.exit(1)
            O = dict(y=inner(bufs["y"]), stats=None, guards={k: intact(b) for k, b in bufs.items() if k != "stats"})
            if p["stats"]:
                O["stats"] = inner(bufs["stats"])[:max(rows.value, 0)].view(-1, 2, nc)
                O["guards"]["stats"] = intact(bufs["stats"], max(rows.value, 0))     # nothing past the rows the call reports
            if p["pre"]:
                O["side"] = inner(bufs["side"])
                O.update((k, inner(bufs[k])[0]) for k in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta") if k in bufs)
                if p["pre"] == 1:
                    O["nbt"] = int(nbt)
            out["err"], out["fails"] = check(p, form, I, O)
            print(json.dumps(out), flush=True)
            del keep, bufs, O, I


# ================================================================================================ the tile class: designed tilebooks
# The LDS-staged kernels over a tilebook (spconv_tile.hip: conv_tile, conv_tile16) and the persistent conv_wlds48, over SYNTHETIC
# tables whose 256-row tiles are built from named recipes and placed so that a persistent workgroup meets, one after the other,
# the tiles its tile loop can get wrong: a tile at the edge of what the kernel stages, a tile without a list, an empty one, the
# ragged last one.  Which workgroup runs which tiles is RESTATED here from the kernel text (tile_schedule) and the placement is
# asserted against it.  tests/data/gather_tile_class.json is the probe list as recorded (tests/test_gather_plan_host.py
# regenerates it); tests/test_gpu_gather_numerics.py runs it, one child per group of TILE_GROUPS.
TILE_CLASS = os.path.join(ROOT, "tests", "data", "gather_tile_class.json")
TB_T, TB_UMAX, TB_LMAX, TB_CAP64, TB_K, TB_LW = 256, 1024, 1023, 960, 27, 10      # tilebook.hpp
TB_BITMAP_BITS = 196608     # tilebook.hpp: the widest span of row numbers that the builder's bitmap form takes
# name: (tiles, rows of the last tile, launch width).  777 tiles: 768 and 512 persistent workgroups run one tile or two;
# 1031 tiles on 512 workgroups: two or three
TILE_TABLES = {"w768A": (777, 1, 768), "w768B": (777, 255, 768), "w512A": (777, 1, 512), "w512B": (777, 255, 512), "w512C": (1031, 129, 512)}
# who runs over a table: (kernel family, workgroups, distinct rows it stages)
TABLE_USERS = {"w768A": (("conv_tile", 768, TB_LMAX),), "w768B": (("conv_tile", 768, TB_LMAX),),
               "w512A": (("conv_tile", 512, TB_CAP64), ("conv_tile16", 512, TB_LMAX), ("conv_wlds48", 256, TB_CAP64)),
               "w512B": (("conv_tile", 512, TB_CAP64), ("conv_tile16", 512, TB_LMAX), ("conv_wlds48", 256, TB_CAP64)),
               "w512C": (("conv_tile", 512, TB_CAP64), ("conv_tile16", 512, TB_LMAX))}
TILE_GROUPS = ("tile.w768A", "tile.w768B", "tile.w512A.m1", "tile.w512A.etc", "tile.w512B.m1", "tile.w512B.etc", "tile.w512C")
ON_1031 = ("conv_tile16<false, false>", "conv_tile16<false, true>", "conv_tile16<true, false>", "conv_tile16<true, true>",
           "conv_tile<1, false, true, 2, true>", "conv_tile<2, true, true, 1, false>")
RECIPES = ("local", "cap64", "cap64+1", "full list", "just over", "far listed", "far over", "one row", "empty", "ragged")
EXACT = {"cap64": TB_CAP64, "cap64+1": TB_CAP64 + 1, "full list": TB_LMAX, "just over": TB_LMAX + 1, "far listed": 900, "far over": 1400}
# recipes on consecutive tiles of one workgroup; between them they hold every wanted transition for both capacities
PLACED = (("local", "far listed"), ("cap64", "cap64+1"), ("cap64", "just over"), ("just over", "local"), ("just over", "just over"),
          ("full list", "one row"), ("cap64+1", "empty"), ("empty", "cap64"), ("far over", "ragged"))
CHAINS = (("local", "just over", "cap64"), ("cap64", "full list", "one row"))      # three tiles of one workgroup (1031 tiles)
WANTED = ("staged -> staged", "staged -> unstaged with a list", "staged -> just over", "just over -> staged", "just over -> just over",
          "full list -> one row", "anything -> empty", "empty -> staged", "anything -> ragged")
CHAIN = "staged -> unstaged -> staged"


def table_rows(name):
    """(n_out, n_in, ld) of a designed table"""
    nt, last, _ = TILE_TABLES[name]
    n = (nt - 1) * TB_T + last
    return n, n + 5, n + 3


def tile_schedule(family, grid, nt):
    """Per workgroup of a launch of `grid` the tiles it runs, in order.  conv_tile and conv_tile16 (spconv_tile.hip): xcd = b & 7,
    slot = b >> 3, L = grid >> 3; XCD x owns the contiguous range [lo, lo + cnt) — the first nt & 7 XCDs one tile more — and the
    workgroup runs lo + slot, lo + slot + L, ...  conv_wlds48 (spconv_wlds.hip): b, b + grid, ..."""
    if family == "conv_wlds48":
        return [list(range(b, nt, grid)) for b in range(grid)]
    assert family in ("conv_tile", "conv_tile16") and grid % 8 == 0
    L, qn, rn = grid >> 3, nt >> 3, nt & 7
    out = []
    for b in range(grid):
        xcd, slot = b & 7, b >> 3
        lo = xcd * (qn + 1) if xcd < rn else rn * (qn + 1) + (xcd - rn) * qn
        cnt = qn + (1 if xcd < rn else 0)
        out.append([lo + tt for tt in range(slot, cnt, L)])
    return out


def stats_owner(family, grid, nt):
    """Per statistics row of a launch the tiles whose rows it sums: conv_tile and conv_tile16 keep ONE row per persistent workgroup
    (stats_flush: part = blockIdx.x), conv_wlds48 one per tile (wlds_epilogue: part = tile)."""
    return [[t] for t in range(nt)] if family == "conv_wlds48" else tile_schedule(family, grid, nt)


def stats_chain(family, n_tiles):
    """D: the longest chain of fp32 additions an addend passes through on its way into a statistics row.  conv_tile / conv_tile16
    (tile_epilogue, stats_flush): the lane adds its S = 4 rows of a tile (st1 += v), that sum joins the lane's running sum (lst +=
    st1: once per tile), row_sum16 folds the 16 lanes of a row group in 4 DPP steps, the four waves are folded as (a + b) + (c + d):
    4 + T + 4 + 2.  conv_wlds48 (wlds_epilogue): S = 2 rows, 4 DPP steps, eight waves one after the other: 2 + 4 + 7."""
    return 2 + 4 + 7 if family == "conv_wlds48" else 4 + n_tiles + 4 + 2


def arrange(name):
    """The recipe of every tile of table `name`: PLACED (and CHAINS) on consecutive tiles of one workgroup for every user of the
    table, the last tile ragged, every other tile local.  Arrangement B walks the workgroups from the other end."""
    nt = TILE_TABLES[name][0]
    recipes = {nt - 1: "ragged"}

    def windows(blocks, k):
        for tiles in blocks:
            for j in range(len(tiles) - k + 1):
                yield tiles[j:j + k]

    def fits(tiles, want, unset_ok):
        return all((recipes.get(t) == w) or (unset_ok and t not in recipes and w != "ragged") for t, w in zip(tiles, want))

    for family, grid, _ in TABLE_USERS[name]:
        blocks = tile_schedule(family, grid, nt)
        if name.endswith("B"):
            blocks = blocks[::-1]
        for want in (CHAINS if nt == 1031 else ()) + PLACED:
            if any(fits(w, want, False) for w in windows(blocks, len(want))):
                continue        # an earlier user's placement serves this one too
            w = next((w for w in windows(blocks, len(want)) if fits(w, want, True)), None)
            assert w is not None, "no workgroup of %s x %d takes %s on table %s" % (family, grid, want, name)
            recipes.update(zip(w, want))
    return [recipes.get(t, "local") for t in range(nt)]


_tables = {}


def design_tiles(name):
    """int32 [27, n_out + 3] table `name` (numpy, read-only, seeded by the name; n_in = n_out + 5) and per tile a dict with its
    recipe, distinct rows U and span (largest - smallest referenced row + 1; 0: no entry).  The recipes:
      local / ragged   entries from the 150 rows on either side of the tile, 25 % absent, 10 % of the rows without any neighbour
      cap64, cap64+1, full list, just over
                       exactly 960, 961, 1023, 1024 distinct rows out of a window of 8192 rows around the tile (bitmap form)
      far listed       exactly 900 distinct rows from the first and the last 2000 rows, row 0 and row n_in - 1 among them:
                       the span exceeds the builder's bitmap (hash + sort form)
      far over         the same with 1400 distinct rows (the hash form's overflow exit)
      one row          every present entry names the same row
      empty            every entry absent
    The columns past n_out hold valid row numbers that nothing may read."""
    import numpy as np
    if name in _tables:
        return _tables[name]
    nt, last, _ = TILE_TABLES[name]
    n, n_in, ld = table_rows(name)
    rs = np.random.RandomState(zlib_crc("tile table " + name))
    t = rs.randint(0, n_in, (TB_K, ld)).astype(np.int32)
    info = []
    for tile, recipe in enumerate(arrange(name)):
        t0 = tile * TB_T
        rows = min(TB_T, n - t0)
        assert (recipe == "ragged") == (tile == nt - 1) and rows == (last if tile == nt - 1 else TB_T)
        present = rs.rand(TB_K, rows) >= 0.25
        present[:, rs.rand(rows) < 0.1] = False
        if recipe == "ragged" and not present.any():
            present[13, 0] = True
        if recipe == "empty":
            present[:] = False
        lo, hi = max(0, t0 - 150), min(n_in, t0 + rows + 150)
        if recipe in EXACT:
            U = EXACT[recipe]
            if recipe.startswith("far"):
                pool = np.concatenate([np.arange(1, 2000), np.arange(n_in - 2000, n_in - 1)])
                used = np.concatenate([[0, n_in - 1], rs.permutation(pool)[:U - 2]])
            else:
                w0 = min(max(0, t0 - 4096), n_in - 8192)
                used = w0 + rs.permutation(8192)[:U]
            P = int(present.sum())
            assert P >= U, (name, tile, P)
            fill = np.concatenate([used, used[rs.randint(0, U, P - U)]])
            rs.shuffle(fill)
            vals = np.zeros((TB_K, rows), dtype=np.int64)
            vals[present] = fill
        elif recipe == "one row":
            vals = np.full((TB_K, rows), rs.randint(lo, hi), dtype=np.int64)
        else:
            vals = rs.randint(lo, hi, (TB_K, rows))
        blk = np.where(present, vals, -1).astype(np.int32)
        t[:, t0:t0 + rows] = blk
        ent = blk[blk >= 0]
        d = len(np.unique(ent))
        span = int(ent.max()) - int(ent.min()) + 1 if d else 0
        want = EXACT.get(recipe, {"one row": 1, "empty": 0}.get(recipe))
        assert d == want if want is not None else 0 < d <= 600, (name, tile, recipe, d)
        # the builder's form: hash + sort above the bitmap's span, the bitmap at or below it
        assert span > TB_BITMAP_BITS if recipe.startswith("far") else span <= TB_BITMAP_BITS, (name, tile, recipe, span)
        if recipe.startswith("far"):
            assert int(ent.min()) == 0 and int(ent.max()) == n_in - 1
        info.append(dict(recipe=recipe, U=d, span=span, empty_rows=int((~present.any(0)).sum())))
    assert all(0 <= int(v) < n_in for v in (t[:, n:].min(), t[:, n:].max()))
    for family, grid, cap in TABLE_USERS[name]:
        seen = transitions(family, grid, cap, info)
        need = set(WANTED) - ({"staged -> unstaged with a list"} if cap == TB_LMAX else set()) | ({CHAIN} if nt == 1031 else set())
        assert need <= seen, (name, family, grid, sorted(need - seen))
    t.setflags(write=False)
    _tables[name] = (t, info)
    return t, info


def zlib_crc(text):
    import zlib
    return zlib.crc32(text.encode())


def tile_kind(i, cap):
    """how a kernel that stages `cap` distinct rows serves a tile: staged, unstaged with a list, or without one"""
    return "staged" if i["U"] <= cap else "listed" if i["U"] <= TB_LMAX else "unlisted"


def transitions(family, grid, cap, info):
    """The wanted transitions (WANTED, CHAIN) that some workgroup of the launch meets on consecutive tiles, from the restated
    schedule.  `staged` here is a tile with entries that the kernel stages: neither the empty nor the ragged one."""
    seen = set()
    real = lambda i: tile_kind(i, cap) == "staged" and i["recipe"] not in ("empty", "ragged")
    for tiles in tile_schedule(family, grid, len(info)):
        for a, b in zip(tiles, tiles[1:]):
            a, b = info[a], info[b]
            ka, kb = tile_kind(a, cap), tile_kind(b, cap)
            if real(a) and real(b):
                seen.add("staged -> staged")
            if real(a) and kb == "listed":
                seen.add("staged -> unstaged with a list")
            if real(a) and b["recipe"] == "just over":
                seen.add("staged -> just over")
            if a["recipe"] == "just over" and real(b):
                seen.add("just over -> staged")
            if a["recipe"] == b["recipe"] == "just over":
                seen.add("just over -> just over")
            if a["recipe"] == "full list" and b["recipe"] == "one row":
                seen.add("full list -> one row")
            if b["recipe"] == "empty":
                seen.add("anything -> empty")
            if a["recipe"] == "empty" and real(b):
                seen.add("empty -> staged")
            if b["recipe"] == "ragged":
                seen.add("anything -> ragged")
        for a, b, c in zip(tiles, tiles[1:], tiles[2:]):
            if real(info[a]) and tile_kind(info[b], cap) != "staged" and real(info[c]):
                seen.add(CHAIN)
    return seen


# ---- the tilebook restated in numpy (tilebook.hpp: tb_upos, tb_lplane, tb_lshift, tb_lpos)
def _tb_maps():
    import numpy as np
    e = np.arange(TB_UMAX)
    upos = (((e >> 5) & 7) * 32 + (e & 31)) * 4 + (e >> 8)
    t = np.arange(TB_T)
    i = t & 15
    sigma = (i & 3) | ((i & 4) << 1) | ((i & 8) >> 1)
    lpos = (t & 0xC0) | (sigma << 2) | ((t >> 4) & 3)
    o = np.arange(TB_K)
    return upos, lpos, (o & 1) * 5 + (o >> 1) // 3, 10 * ((o >> 1) % 3)


def tilebook_numpy(t, n_out):
    """The tilebook of table `t` as tilebook.hip must build it: ulist [nt, 1024] int32 in storage order (entry e at tb_upos(e):
    the distinct rows ascending, -1 past the count; all -2 for a tile of more than 1023), lidx [nt, 10, 256] uint32 (zero for
    a tile without a list, whose words the builder leaves alone), ucount, span and n_over."""
    import numpy as np
    nt = -(-n_out // TB_T)
    upos, lpos, plane, shift = _tb_maps()
    ulist = np.full((nt, TB_UMAX), -1, np.int32)
    lidx = np.zeros((nt, TB_LW, TB_T), np.uint32)
    ucount, span = np.zeros(nt, np.int32), np.zeros(nt, np.int64)
    for tile in range(nt):
        ent = np.full((TB_K, TB_T), -1, np.int64)
        rows = min(TB_T, n_out - tile * TB_T)
        ent[:, :rows] = t[:, tile * TB_T:tile * TB_T + rows]
        uniq = np.unique(ent[ent >= 0])
        U = ucount[tile] = len(uniq)
        span[tile] = int(uniq[-1] - uniq[0] + 1) if U else 0
        if U > TB_LMAX:
            ulist[tile] = -2
            continue
        ulist[tile, upos[:U]] = uniq
        loc = np.where(ent >= 0, np.searchsorted(uniq, ent) + 1, 0).astype(np.uint32)
        for o in range(TB_K):
            lidx[tile, plane[o], lpos] |= loc[o] << np.uint32(shift[o])
    return dict(ulist=ulist, lidx=lidx, ucount=ucount, span=span, n_over=np.array([(ucount > TB_CAP64).sum(), (ucount > TB_LMAX).sum()], np.int32))


def tilebook_entries(tb, tile):
    """the [27, 256] table entries that tile `tile` of a tilebook encodes (-1: absent); None for a tile without a list"""
    import numpy as np
    upos, lpos, plane, shift = _tb_maps()
    if tb["ucount"][tile] > TB_LMAX:
        return None
    ul = tb["ulist"][tile][upos].astype(np.int64)       # entry e
    loc = np.stack([(tb["lidx"][tile, plane[o]][lpos] >> np.uint32(shift[o])) & np.uint32(0x3ff) for o in range(TB_K)]).astype(np.int64)
    return np.where(loc == 0, -1, ul[np.maximum(loc - 1, 0)])


def tilebook_parts(tb_bytes, n_out):
    """the four arrays of a built tilebook (a uint8 tensor; tilebook.hpp tilebook_view) as numpy"""
    import numpy as np
    nt = -(-n_out // TB_T)
    raw = tb_bytes.cpu().numpy()
    a, b = nt * TB_UMAX * 4, nt * TB_LW * TB_T * 4
    assert raw.size == a + b + 4 * nt + 8
    return dict(ulist=raw[:a].view(np.int32).reshape(nt, TB_UMAX), lidx=raw[a:a + b].view(np.uint32).reshape(nt, TB_LW, TB_T),
                ucount=raw[a + b:a + b + 4 * nt].view(np.int32), n_over=raw[a + b + 4 * nt:].view(np.int32))


def tilebook_differences(got, want):
    """What a built tilebook `got` has other than the restatement `want`, as a list of strings.  A tile of more than 1023 distinct
    rows has no local indices, and in the hash form its count is whatever the insert loop had reached when it gave up (> 1023)."""
    import numpy as np
    out = []
    listed = want["ucount"] <= TB_LMAX
    exact = listed | (want["span"] <= TB_BITMAP_BITS)
    bad = np.nonzero(np.where(exact, got["ucount"] != want["ucount"], got["ucount"] <= TB_LMAX))[0]
    out += ["ucount of tile %d: %d, not %d" % (k, got["ucount"][k], want["ucount"][k]) for k in bad[:5]]
    bad = np.nonzero((got["ulist"] != want["ulist"]).any(1))[0]
    out += ["ulist of tile %d" % k for k in bad[:5]]
    bad = np.nonzero(((got["lidx"] != want["lidx"]).any((1, 2))) & listed)[0]
    out += ["lidx of tile %d" % k for k in bad[:5]]
    if list(got["n_over"]) != list(want["n_over"]):
        out.append("n_over %s, not %s" % (list(got["n_over"]), list(want["n_over"])))
    return out


# ---- the probe list
def tile_space():
    """Candidate calls: every channel pair of the tile kernels and the 48 -> 48 layer, both output types, with and without
    statistics, default switches and the pipeline or the dual option off."""
    for kc, esz in ((16, 2), (32, 2), (16, 4), (48, 2)):
        for nc in (16, 32, 48, 64):
            for out32 in ((0, 1) if esz == 2 else (0,)):
                for stats in (0, 1):
                    for off in ((), ("tile_pipeline",), ("tile_dual",)):
                        yield dict(K=27, kc=kc, nc=nc, esz=esz, out32=out32, stats=stats, off=off, tilebook=int(kc != 48), pre=0, res_bcast=0,
                                   f32split=0)


def tile_group(route, table):
    if TILE_TABLES[table][2] == 768 or table == "w512C":
        return "tile." + table
    return "tile.%s.%s" % (table, "m1" if route.startswith("conv_tile<1") else "etc")


def generate_tile_class(ask, admitted):
    """One probe per (name, table): every conv_tile, conv_tile16 and conv_wlds48 name of `admitted` at the smallest channel pair
    and switch setting that reaches it on a 777-tile table, over both arrangements of its launch width; conv_tile16, one dual and
    one fp32 instantiation also on the 1031-tile table.  Forward and data gradient (layouts 0 and 2: the plan does not look at the
    layout, so both reach every name), a dense residual, ld = n_out + 3."""
    names = sorted(n for n in admitted if re.match(r"conv_(tile|tile16|wlds48)<", n))
    calls = list(tile_space())
    n, n_in, ld = table_rows("w768A")
    got = ask([plan_line(dict(c, n_out=n, n_in=n_in, ld=ld)) for c in calls])
    best = {}
    for c, g in zip(calls, got):
        rank = (c["kc"], c["nc"], len(c["off"]))
        if g["status"] == 0 and (g["route"] not in best or rank < best[g["route"]][0]):
            best[g["route"]] = (rank, c, g["grid"])
    probes = []
    for route in names:
        _, c, grid = best[route]
        fam = re.match(r"\w+", route).group(0)
        width = 512 if fam == "conv_wlds48" else grid
        assert (fam, grid) in {("conv_tile", 768), ("conv_tile", 512), ("conv_tile16", 512), ("conv_wlds48", 256)}, (route, grid)
        tables = [t for t, v in TILE_TABLES.items() if v[2] == width and (v[0] == 777 or route in ON_1031)]
        for table in tables:
            assert any(f == fam and g == grid for f, g, _ in TABLE_USERS[table]), (route, table)
            n, n_in, ld = table_rows(table)
            q = dict(c, n_out=n, n_in=n_in, ld=ld)
            g = ask([plan_line(q)])[0]
            assert (g["status"], g["route"], g["grid"]) == (0, route, grid), (route, table, g)
            assert g["parts"] == (TILE_TABLES[table][0] if fam == "conv_wlds48" else grid), g
            plain = None
            if fam == "conv_tile16" or (fam == "conv_tile" and route.endswith("true>")):     # the same y as the plain conv_tile (spconv_tile.hip)
                po = tuple(c["off"]) + (("tile_pipeline",) if fam == "conv_tile16" else ("tile_dual",))
                h = ask([plan_line(dict(q, stats=0, off=po))])[0]
                assert h["status"] == 0 and re.match(r"conv_tile<[01], (true|false), false, 1, false>$", h["route"]), (route, h)
                plain = dict(route=h["route"], grid=h["grid"], off=list(po))
            p = dict(route=route, group=tile_group(route, table), table=table, grid=grid, parts=g["parts"], layouts=[0, 2])
            p.update((k, q[k]) for k in ("K", "kc", "nc", "esz", "n_out", "n_in", "ld", "out32", "stats", "tilebook", "pre", "res_bcast", "f32split"))
            p.update(off=list(c["off"]), plain=plain)
            probes.append(p)
    assert {p["group"] for p in probes} == set(TILE_GROUPS)
    return probes


def dump_tile_class(probes):
    return "[" + ",\n".join(json.dumps(p) for p in probes) + "]\n"


def load_tile_class():
    return json.load(open(TILE_CLASS))


# ---- operands, reference and checks
def tile_inputs(p, layout, dev, tbl):
    """make_inputs over the designed table, seeded by name, table and layout; one draw serves both statistics forms.  `w_call` is
    what the call gets (layout 2: [K][nc][kc]), `w` what the reference multiplies under offset o (layout 2: w_call[K - 1 - o]^T)."""
    q = dict(p, route="%s %s layout %d" % (p["route"], p["table"], layout))
    I = make_inputs(q, "bn" if p["stats"] else "y", dev, tbl)
    I["w_call"] = I["w"]
    if layout == 2:
        I["w_call"] = I["w"].transpose(1, 2).contiguous()
        I["w"] = I["w"].flip(0).contiguous()
    else:
        assert layout == 0
    return I


def tile_reference(p, I):
    return conv64(I["x"].double(), I["w"], I["tbl"], p["n_out"]) + I["res"].double()


def per_part(a, owner, n_parts):
    """[n_parts, nc] sums of the rows of `a` [n_out, nc] over the tiles each statistics row owns (owner: tile -> row, long)"""
    import torch
    nt = owner.numel()
    pad = torch.zeros(nt * TB_T, a.shape[1], dtype=a.dtype, device=a.device)
    pad[:a.shape[0]] = a
    return torch.zeros(n_parts, a.shape[1], dtype=a.dtype, device=a.device).index_add_(0, owner, pad.view(nt, TB_T, -1).sum(1))


def tile_check(p, form, I, O, ref):
    """The measured errors of one call over a designed table and the bounds they miss (empty: the call passes).
      y        every row against fp64: fp32 rows within Y_TOL[True] of the largest value; bf16 rows ELEMENTWISE within
               2^-7 |ref| + 1e-5 max |ref| (tests/test_gpu_round4.py), as the largest ratio error / bound
      bare     elements of rows without any neighbour — every row of an empty tile is one — that are not bit-equal to the residual
      stats0/1 the totals against fp64 sums of the stored y, STATS_TOL
      part0/1  every statistics row against the fp64 sums over exactly the tiles its workgroup runs (stats_owner), as the largest
               ratio error / (D 2^-24 sum |addend|).  D = stats_chain(); the second sum's addend is a product of rounded
               factors: v v (one more rounding), or v xhat with xhat = (x - mean) invstd in fp32 (three more)."""
    import torch
    err, fails = {}, []
    f32 = y_dtype(p) == torch.float32
    fam = re.match(r"\w+", p["route"]).group(0)

    def bound(name, value, tol, strict=True):
        err[name] = value
        if not (value < tol if strict else value <= tol):
            fails.append("%s %.3g %s %.3g" % (name, value, ">=" if strict else ">", tol))

    diff = (O["y"].double() - ref).abs()
    scale = ref.abs().max()
    if f32:
        bound("y", float(diff.max() / scale.clamp(min=1e-30)), Y_TOL[True])
    else:
        bound("y", float((diff / (2.0 ** -7 * ref.abs() + 1e-5 * scale)).max()), 1.0, strict=False)
    bare = ~(I["tbl"][:, :p["n_out"]] >= 0).any(0)
    bound("bare", float((O["y"][bare] != I["res"][bare]).sum()), 0.0, strict=False)
    if p["stats"]:
        a = stats_addends(p, form, I, O["y"])
        got = O["stats"].double()
        nt = -(-p["n_out"] // TB_T)
        owned = stats_owner(fam, p["grid"], nt)
        assert got.shape[0] == len(owned) == p["parts"], (got.shape, len(owned))
        owner = torch.empty(nt, dtype=torch.long)
        for k, tiles in enumerate(owned):
            owner[torch.tensor(tiles, dtype=torch.long)] = k
        owner = owner.to(ref.device)
        D = torch.tensor([stats_chain(fam, len(tiles)) for tiles in owned], dtype=torch.float64, device=ref.device).view(-1, 1)
        for k in (0, 1):
            bound("stats%d" % k, scale_err(got[:, k].sum(0), a[k].sum(0)), STATS_TOL)
            more = 0 if k == 0 else 3 if form == "bn" else 1
            d = (got[:, k] - per_part(a[k], owner, len(owned))).abs()
            lim = (D + more) * 2.0 ** -24 * per_part(a[k].abs(), owner, len(owned))
            ratio = torch.where(d > 0, d / lim.clamp(min=1e-300), torch.zeros_like(d))
            bound("part%d" % k, float(ratio.max()), 1.0, strict=False)
    broken = sorted(k for k, ok in O["guards"].items() if not ok)
    err["guards"] = not broken
    if broken:
        fails.append("guards overwritten: " + ", ".join(broken))
    return err, fails


def tile_ideal(p, form, I, ref):
    """What a correct kernel stores over a designed table: the fp64 reference rounded once, the statistics rows the fp64 sums over
    the tiles of their workgroups rounded once (CPU tests)."""
    import torch
    fam = re.match(r"\w+", p["route"]).group(0)
    O = dict(y=ref.to(y_dtype(p)), stats=None, guards={"y": True})
    if p["stats"]:
        a = stats_addends(p, form, I, O["y"])
        owned = stats_owner(fam, p["grid"], -(-p["n_out"] // TB_T))
        owner = torch.empty(-(-p["n_out"] // TB_T), dtype=torch.long)
        for k, tiles in enumerate(owned):
            owner[torch.tensor(tiles, dtype=torch.long)] = k
        O["stats"] = torch.stack([per_part(a[0], owner, len(owned)), per_part(a[1], owner, len(owned))], 1).float()
    return O


# ---- the device run
def run_tile_group(group):
    """The group's designed table: its tilebook against the numpy restatement (one JSON line), then every probe of the group per
    layout and statistics form (one JSON line each): the call, a repeated identical call (bit-equal) and, for the pipelined and
    the dual kernels, the plain conv_tile over the same table (bit-equal y)."""
    import sys
    import torch
    from doda_amd import ops
    from doda_amd._lib import lib
    assert group in TILE_GROUPS and os.environ.get("DODA_TRACE_GATHER") == "1" and "DODA_F32_SPLIT_ROWS" not in os.environ
    dev = torch.device("cuda:0")
    L = lib()
    probes = [p for p in load_tile_class() if p["group"] == group]
    table = probes[0]["table"]
    t, info = design_tiles(table)
    n_out, n_in, ld = table_rows(table)
    tbl = torch.from_numpy(t.copy()).to(dev)
    tb = ops.tilebook_build(tbl, n_out)
    torch.cuda.synchronize()
    want = tilebook_numpy(t, n_out)
    print(json.dumps(dict(tilebook=table, tiles=len(info), n_over=[int(v) for v in want["n_over"]],
                          differences=tilebook_differences(tilebook_parts(tb, n_out), want))), flush=True)

    def call(p, layout, form, I, off, stats):
        kc, nc, esz = p["kc"], p["nc"], p["esz"]
        dt, ydt = storage(p), y_dtype(p)
        xbuf = torch.full((n_in + 2 * G, kc), float("nan"), dtype=dt, device=dev)
        inner(xbuf).copy_(I["x"])
        rbuf = torch.full((n_out + 2 * G, nc), float("nan"), dtype=ydt, device=dev)
        inner(rbuf).copy_(I["res"])
        bufs = {"y": guarded(n_out, nc, ydt, dev)}
        need = int(L.doda_spconv_gather_workspace_bytes(27, kc, nc, esz))
        bufs["ws"] = guarded(need // 256, 256, torch.uint8, dev)
        ep = ops._ConvEpilogue()
        ep.residual, ep.residual_bcast = inner(rbuf).data_ptr(), 0
        rows = C.c_int32(-1)
        if stats:
            bufs["stats"] = guarded(int(L.doda_spconv_stats_capacity(n_out)), 2 * nc, torch.float32, dev)
            ep.stats, ep.stats_rows_h = inner(bufs["stats"]).data_ptr(), C.pointer(rows)
            if form == "bn":
                ep.bn_x, ep.bn_relu = I["bn_x"].data_ptr(), 1
                ep.bn_mean, ep.bn_invstd, ep.bn_gamma, ep.bn_beta = (I[k].data_ptr() for k in ("bn_mean", "bn_invstd", "bn_gamma", "bn_beta"))
        if p["tilebook"]:
            ep.tilebook, ep.tilebook_rows = tb.data_ptr(), n_out
        for o in off:
            L.doda_set_option(OPT[o], 0)
        st, text = _with_trace(lambda: L.doda_spconv_gather_ex(
            inner(xbuf).data_ptr(), n_in, kc, esz, I["w_call"].data_ptr(), nc, tbl.data_ptr(), ld, 27, n_out, inner(bufs["y"]).data_ptr(),
            p["out32"], layout, inner(bufs["ws"]).data_ptr(), need, C.byref(ep), None))
        for o in off:
            L.doda_set_option(OPT[o], 1)
        torch.cuda.synchronize()
        m = re.search(r" route=(.*) grid=(\d+) block=\d+ parts=(\d+)$", text, re.M)
        out = dict(status=st, route=m[1] if m else None, grid=int(m[2]) if m else -1, rows=rows.value)
        if st != 0:
            print(json.dumps(dict(out, want=p["route"], table=table, layout=layout, form=form)), flush=True)
            sys.exit(1)
        O = dict(y=inner(bufs["y"]), stats=None, guards={k: intact(b) for k, b in bufs.items() if k != "stats"})
        if stats:
            O["stats"] = inner(bufs["stats"])[:max(rows.value, 0)].view(-1, 2, nc)
            O["guards"]["stats"] = intact(bufs["stats"], max(rows.value, 0))
        return out, O

    for p in probes:
        assert p["table"] == table and (p["n_out"], p["n_in"], p["ld"]) == (n_out, n_in, ld)
        for layout in p["layouts"]:
            I = tile_inputs(p, layout, dev, tbl)
            ref = tile_reference(p, I)
            for k, form in enumerate(("y", "bn") if p["stats"] else ("y",)):
                out, O = call(p, layout, form, I, p["off"], p["stats"])
                err, fails = tile_check(p, form, I, O, ref)
                _, O2 = call(p, layout, form, I, p["off"], p["stats"])
                err["repeat"] = bool(torch.equal(O["y"], O2["y"])) and (not p["stats"] or bool(torch.equal(O["stats"], O2["stats"])))
                if not err["repeat"]:
                    fails.append("a repeated identical call differs")
                if p["plain"] and k == 0:
                    po, O3 = call(p, layout, "y", I, p["plain"]["off"], 0)
                    err["plain"] = bool(torch.equal(O["y"], O3["y"])) and (po["route"], po["grid"]) == (p["plain"]["route"], p["plain"]["grid"])
                    if not err["plain"]:
                        fails.append("differs from %s (traced %s, grid %d)" % (p["plain"]["route"], po["route"], po["grid"]))
                print(json.dumps(dict(out, want=p["route"], table=table, layout=layout, form=form, err=err, fails=fails)), flush=True)
                del O, O2
            del I, ref


if __name__ == "__main__":
    import subprocess
    import sys
    if sys.argv[1] == "--tile-class":       # PLANNER: the built tests/host/gather_plan_main.cpp; prints the content of TILE_CLASS
        exe = sys.argv[2]

        def ask(lines):
            r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
            out = [re.match(r"status=(-?\d+) route=(.*) grid=(\d+) block=(\d+) parts=(\d+) ", l) for l in r.stdout.splitlines()]
            assert len(out) == len(lines) and all(out)
            return [dict(status=int(m[1]), route=m[2], grid=int(m[3]), block=int(m[4]), parts=int(m[5])) for m in out]
        admitted = subprocess.run([exe, "--compiled"], capture_output=True, text=True, check=True).stdout.splitlines()
        sys.stdout.write(dump_tile_class(generate_tile_class(ask, admitted)))

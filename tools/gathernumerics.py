"""Numerics probes of doda_spconv_gather_ex: one call per kernel instantiation that the route plan (csrc/gather_plan.hpp) can reach,
each compared with an fp64 reference (tools/gatherroutes.py --numerics GROUP; tests/test_gpu_gather_numerics.py).

The probe list is GENERATED from the plan: `space()` walks the calls, the host planner (tests/host/gather_plan_main.cpp) names the
route of each, `select()` keeps per route the call of fewest output rows and `shape()` moves it to the smallest shape at which the
kernel can still go wrong (a ragged last wave tile, a second tile, idle persistent workgroups).  tests/data/gather_numerics.json is
that list as recorded; tests/test_gather_plan_host.py regenerates it and asserts equality, and that the names it reaches, the names
the predicates of gather_plan.hpp admit and tests/data/gather_instantiations.json (what is compiled) are one set of 247.

The checkers (`reference`, `check`) are plain torch on whatever device the tensors are on: tests/test_gather_numerics_host.py feeds
them the rounded reference and corrupted copies of it on the CPU."""
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


def stats64(p, form, I, y):
    """[2, nc] fp64 sums over the STORED y: (sum y, sum y^2), or the BatchNorm-backward pair (sum dz, sum dz xhat)."""
    import torch
    yd = y.double()
    if form == "bn":
        xh, mask = bn_front(I["bn_x"], I["bn_mean"], I["bn_invstd"], I["bn_gamma"], I["bn_beta"])
        dz = yd * mask
        return torch.stack([dz.sum(0), (dz * xh).sum(0)])
    return torch.stack([yd.sum(0), (yd * yd).sum(0)])


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

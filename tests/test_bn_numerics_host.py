"""tools/bnnumerics.py on the CPU: the probe table of tests/test_gpu_bn_numerics.py reaches every compiled BatchNorm kernel
(tests/data/bn_instantiations.json, regenerated from the built objects when they are there) and nothing else, has a probe on each
side of every threshold of the route selection (the constants are parsed from bn.hip / layers_plan.hpp), keeps the undecided ReLU
masks of every backward probe below 1e-4 of its elements — and its bounds do their work: the fp64 reference rounded once and the
kernels' expressions in numpy float32 pass them, twelve subtly wrong results (applied to the reference's own outputs) do not."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bn = _load("bnnumerics")
K = bn.K
CPU = torch.device("cpu")
PROBES = bn.probes()
BY_ID = {p["id"]: p for p in PROBES}
FWD = ("fwd", "fwd_final", "fwd_stats", "fwd_totals", "lay_fwd", "apply")
BWD = ("bwd", "bwd_stats", "bwd_totals", "lay_bwd")


def names(p):
    return [r[0] for r in bn.routes(p)]


def find(**kw):
    """The probes whose fields equal kw (relu, training and the add operand default to the plain call's)."""
    want = dict(dict(relu=1, training=1, add=None, accum=0, split=0, c_a=0, y_pad=0, x_slice=0, status=0), **kw)
    got = [p for p in PROBES if all(p[k] == v for k, v in want.items())]
    assert got, kw
    return got


def test_one_set_of_names():
    """Probed = compiled: 41 kernels (33 of bn.hip, 8 of layers.hip)."""
    compiled = json.load(open(bn.INSTANTIATIONS))
    objs = [os.path.join(ROOT, "doda_amd", "csrc", "_obj", f) for f in ("bn.o", "layers.o")]
    gr = _load("gatherroutes")
    if all(os.path.exists(o) for o in objs) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        assert gr.instantiations(objs, bn.STEMS) == compiled       # regenerate: tools/gatherroutes.py --instantiations --stem bn_,lay_ ...
    probed = {n for p in PROBES for n in names(p)}
    assert probed == set(compiled) and len(compiled) == 41, sorted(probed ^ set(compiled))
    assert sum(n.startswith("bn_") for n in compiled) == 33 and sum(n.startswith("lay_") for n in compiled) == 8
    for g, env in bn.GROUPS.items():
        assert set(env) <= set(bn.SWITCHES) and bn.probes(g)


def test_every_threshold_has_a_probe_on_each_side():
    small, tuned = K["BN_SMALL_ROWS"], K["TUNED_ROWS"]
    assert (small, tuned[4], tuned[2], K["BN_FUSED_MAX_C"], K["BN_TOT_MAX_C"]) == (4096, 4096, 32768, 64, 256)      # (what the issue's shapes assume)
    for esz, T in bn.TNAME.items():
        for c in (16, 48):      # one launch up to BN_SMALL_ROWS rows, three above
            for e, k in (("fwd", "bn_small_fwd"), ("bwd", "bn_small_bwd")):
                assert names(find(group="standalone", entry=e, esz=esz, m=small, c=c)[0]) == ["%s<%s>" % (k, T)]
                assert len(names(find(group="standalone", entry=e, esz=esz, m=small + 1, c=c)[0])) == 3
        for m in (1, 37, 255, 256, 257, small - 1, 3 * small + 1):
            assert find(group="standalone", entry="bwd", esz=esz, m=m, c=48, add="slice")
        # one row lane per workgroup, and 256 of them, in the partial-sum kernels
        assert bn.make_geo(1024)[1] == 1 and bn.make_geo(4)[1] == 256
        for c in (4, 20, 1024):
            assert names(find(group="standalone", entry="fwd", esz=esz, m=small + 1, c=c)[0])[0].startswith("bn_stats_partial")
        # fused_ok: channels, bytes of the statistics rows, elements
        cmax, rmax, mmax = K["BN_FUSED_MAX_C"], K["BN_FUSED_MAX_PARTIAL_BYTES"] // (2 * 64 * 4), K["BN_FUSED_SMALL_ELEMS"] // 64
        for e, k in (("fwd_stats", "bn_fused_fwd"), ("bwd_stats", "bn_fused_bwd")):
            one = ["%s<%s>" % (k, T)]
            assert names(find(entry=e, esz=esz, m=37, c=cmax, R=5)[0]) == one and len(names(find(entry=e, esz=esz, m=37, c=cmax + 4, R=5)[0])) == 2
            assert names(find(entry=e, esz=esz, m=37, c=64, R=rmax, add=None if e == "fwd_stats" else None)[0]) == one
            assert len(names(find(entry=e, esz=esz, m=37, c=64, R=rmax + 1)[0])) == 2
            add = None if e == "fwd_stats" else "dense"
            assert names(find(entry=e, esz=esz, m=mmax, c=64, R=5, add=add)[0]) == one and len(names(find(entry=e, esz=esz, m=mmax + 1, c=64, R=5, add=add)[0])) == 2
        assert bn.fused_ok(5, 64, 37) and names(find(entry="bwd_stats", esz=esz, m=37, c=64, R=5, add="slice")[0])[0] == "bn_bwd_final_stats"
        # sum_rows, four rows in flight: a thread enters the unrolled trip from 3 * step + its first row on
        for R in (3 * 256, 3 * 256 + 1, 4 * 256 + 3):
            assert find(entry="fwd_final", m=37, c=16, R=R) and find(entry="fwd_stats", esz=esz, c=68, R=R) and find(entry="bwd_stats", esz=esz, c=68, R=R)
        for c in (64, 16):
            rpb = bn.make_geo(c)[1]
            # (the last row lane's first unrolled trip; at 64 channels also a row lane without a row)
            for R in (4 * rpb - 1, 4 * rpb, 4 * rpb + 1) + ((rpb - 1, rpb, rpb + 1) if c == 64 else ()):
                assert names(find(entry="fwd_stats", esz=esz, m=37, c=c, R=R)[0])[0].startswith("bn_fused_fwd")
        # no FIXED grid: 112 channels in fp32 at 37 rows, an odd fragment count in bf16
        assert names(find(entry="fwd_stats", esz=4, m=37, c=112)[0])[1] == "bn_apply<F32, false, false>"
        assert names(find(group="standalone", entry="fwd", esz=2, m=small + 1, c=20)[0])[2] == "bn_apply<BF16, false, false>"
        # totals: BN_TOT_MAX_C, the second trip of the FIXED sweeps under DODA_BN_TOT_GRID=64
        assert find(entry="fwd_totals", esz=esz, c=K["BN_TOT_MAX_C"]) and find(entry="fwd_totals", esz=esz, c=K["BN_TOT_MAX_C"] + 4, status=bn.ERR_UNSUPPORTED)
        assert find(entry="fwd_totals", esz=esz, c=20, c_a=10, status=bn.ERR_INVALID)
        for e in ("fwd_totals", "bwd_totals"):
            p = find(entry=e, esz=esz, m=2 * small + 1, c=16)[0]
            (name, grid, block), = bn.routes(p)
            assert name.endswith("true, true>") and grid == 64 and p["m"] * 4 // (2 if esz == 2 else 1) > grid * block
        # the op list: lay_bn's tail of four rows in flight, the hand-over to bn.hip
        p = find(entry="lay_fwd", esz=esz, m=300, c=256)[0]
        grid, rpb = bn.lay_bn_grid(p)
        trips = -(-300 // (grid * rpb))
        assert grid == 3 and trips > 4 and trips % 4
        for e, k in (("lay_fwd", "bn_apply"), ("lay_bwd", "bn_bwd_apply")):
            assert names(find(entry=e, esz=esz, m=tuned[esz] - 1, c=16)[0]) == ["lay_bn<%d, %d>" % (esz, 1 if e == "lay_fwd" else 2)]
            assert names(find(entry=e, esz=esz, m=tuned[esz], c=16)[0]) == ["%s<%s, true, true>" % (k, T)]
        assert names(find(entry="lay_bwd", esz=esz, m=tuned[esz] - 1, c=16, add="dense")[0]) == ["lay_bn<%d, 3>" % esz]


def test_undecided_masks_are_rare_in_every_backward_probe():
    """From the reference alone: at most 1e-4 of a backward probe's elements lie within the forward bound of zero."""
    seen = {}
    for p in PROBES:
        if p["entry"] in BWD and p["relu"] and not p["status"]:
            seen.setdefault((p["m"], p["c"], p["esz"], p["form"]), p)
    assert len(seen) > 60
    for p in seen.values():
        I = bn.make_inputs(dict(p, entry="bwd", add=None), CPU)
        D = bn.bwd_definition(p, I)
        assert D["undecided"] <= bn.MAX_UNDECIDED, (p["id"], D["undecided"])
        assert float(D["S1"][2]) == 0.0 and float(D["S2"][2]) == 0.0 and float(D["S2"][1]) == 0.0       # the dead and the constant channel


SMALL = [p for p in PROBES if not p["status"] and p["m"] <= 37 and p["c"] <= 48 and p["R"] in (0, 5)] + \
    [BY_ID[i] for i in ("rows.fwd_final.bf16.m37.c16.R1027", "standalone.fwd.f32.m4097.c16", "standalone.bwd.bf16.m4097.c20.add=slice",
                        "layers.lay_stats.f32.m337.c16.ranges", "layers.lay_stats.bf16.m4097.c8.x_slice1")]


@pytest.mark.parametrize("kind", ["rounded_reference", "numpy_float32"])
def test_unmutated_results_pass(kind):
    assert len(SMALL) > 150
    for p in SMALL:
        I = bn.make_inputs(p, CPU)
        O = bn.ideal_outputs(p, I) if kind == "rounded_reference" else bn.emulated_outputs(p, I)
        err, fails = bn.check(p, I, O)
        assert fails == [] and err and all(v[1] <= 1.0 for v in err.values()), (p["id"], err, fails)


def _fwd_family(esz):
    return [find(group="standalone", entry="fwd", esz=esz, m=37, c=16)[0], find(entry="fwd_stats", esz=esz, m=37, c=16, R=255)[0],
            find(entry="fwd_totals", esz=esz, m=37, c=16)[0], find(entry="lay_fwd", esz=esz, m=37, c=16)[0]]


def _bwd_family(esz, add="dense"):
    return [find(group="standalone", entry="bwd", esz=esz, m=37, c=16, add=add)[0], find(entry="bwd_stats", esz=esz, m=37, c=16, R=255, add=add)[0],
            find(entry="bwd_totals", esz=esz, m=37, c=16, add=add)[0], find(entry="lay_bwd", esz=esz, m=37, c=16, add=add)[0]]


def _rejected(p, I, O, quantity):
    err, fails = bn.check(p, I, O)
    assert any(f.startswith(quantity + ":") for f in fails), (p["id"], quantity, err, fails)


def _stats(p, I):
    """(mean, biased variance) in fp64 of what the call's statistics say."""
    S = bn.handed_sums(p, I)
    if S is None:
        x = I["x"].double()
        return x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
    mean = S[0] / p["m"]
    return mean, (S[1] / p["m"] - mean * mean).clamp(min=0)


@pytest.mark.parametrize("esz", [2, 4])
def test_wrong_forward_statistics_are_rejected(esz):
    mom = float(torch.tensor(bn.MOMENTUM, dtype=torch.float32))
    for p in _fwd_family(esz):
        I = bn.make_inputs(p, CPU)
        O = bn.ideal_outputs(p, I)
        m = p["m"]
        mean, var = _stats(p, I)
        _rejected(p, I, dict(O, mean=(mean * m / (m + 1)).float()), "mean")                                           # m + 1 in place of m
        _rejected(p, I, dict(O, rv=((1 - mom) * I["rv0"].double() + mom * var).float()), "rv")                       # biased variance in running_var
        _rejected(p, I, dict(O, invstd=(1 / torch.sqrt(var.clamp(min=1e-30))).float()), "invstd")                    # eps omitted
        _rejected(p, I, dict(O, rm=(mom * I["rm0"].double() + (1 - mom) * mean).float()), "rm")                      # momentum on the wrong operand
        _rejected(p, I, dict(O, nbt=O["nbt"] - 1), "nbt")
        if p["entry"] == "fwd":                                                                                       # one input row dropped from a sum
            _rejected(p, I, dict(O, mean=((I["x"].double().sum(0) - I["x"][m - 1].double()) / m).float()), "mean")
        y = O["y"].clone()
        y[m - 1, 5] = 0.0 if float(y[m - 1, 5]) else 1.0
        _rejected(p, I, dict(O, y=y), "y")


def test_dropped_statistics_are_rejected():
    p = BY_ID["rows.fwd_final.bf16.m37.c16.R1027"]                  # one statistics row of the largest R
    I = bn.make_inputs(p, CPU)
    O = bn.ideal_outputs(dict(p, R=1026), dict(I, rows=I["rows"][:-1]))
    for q in ("mean", "invstd", "rm", "rv"):
        _rejected(p, I, O, q)
    p = find(entry="bwd_stats", esz=4, m=37, c=68, R=1027)[0]
    I = bn.make_inputs(p, CPU)
    O = bn.ideal_outputs(p, dict(I, rows=I["rows"][1:]))
    for q in ("dgamma", "dbeta", "dx"):
        _rejected(p, I, O, q)
    for p in (find(entry="fwd_totals", esz=2, m=37, c=8)[0], find(entry="lay_fwd", esz=4, m=37, c=16)[0]):      # one totals slot
        I = bn.make_inputs(p, CPU)
        ta = I["ta"].clone()
        ta[3, :, :, :4] = 0
        O = bn.ideal_outputs(p, dict(I, ta=ta))
        for q in ("mean", "invstd", "rm", "rv"):
            _rejected(p, I, O, q)
    for e in ("fwd_totals", "lay_fwd"):                             # the second producer's columns read from the first
        p = find(entry=e, esz=4, m=37, c=16, c_a=8)[0]
        I = bn.make_inputs(p, CPU)
        O = bn.ideal_outputs(p, I)
        _rejected(p, I, dict(O, mean=torch.cat([O["mean"][:8], O["mean"][:8]])), "mean")
        _rejected(p, I, dict(O, invstd=torch.cat([O["invstd"][:8], O["invstd"][:8]])), "invstd")
    p = find(entry="lay_stats", esz=2, m=37, c=16, ranges=[(0, 37)])[0]       # one input row dropped from lay_stats' sums
    I = bn.make_inputs(p, CPU)
    O = bn.ideal_outputs(p, I)
    x = I["x"][36].double()
    _rejected(p, I, dict(O, totals=O["totals"] - torch.stack([x, x * x])), "totals")


@pytest.mark.parametrize("esz", [2, 4])
def test_wrong_backward_results_are_rejected(esz):
    for p in _bwd_family(esz):
        I = bn.make_inputs(p, CPU)
        O = bn.ideal_outputs(p, I)
        D = bn.bwd_definition(p, I)
        Q = bn.reference(p, I, O)
        a = I["gamma"].double() * I["invstd_in"].double()
        dy = I["dy"].double()
        # one ReLU mask bit flipped on a decided element (the largest |dy| of a live channel)
        ch = 5
        r = int((dy[:, ch].abs() * ~D["und"][:, ch]).argmax())
        on = bool(D["dz"][r, ch] != 0)
        dx = Q["dx"][0].clone()
        dx[r, ch] += a[ch] * dy[r, ch] * (-1 if on else 1)
        _rejected(p, I, dict(O, dx=dx.to(O["dx"].dtype)), "dx")
        dx = Q["dx"][0].clone()                                                                                       # add dropped on one row
        dx[36] -= I["add"][36].double()
        _rejected(p, I, dict(O, dx=dx.to(O["dx"].dtype)), "dx")
        _rejected(p, I, dict(O, dx=(Q["dx"][0] + a * Q["dbeta"][0] / p["m"]).to(O["dx"].dtype)), "dx")              # mean(dz) omitted
        if p["entry"] == "bwd":                                                                                       # one input row dropped from the sums
            _rejected(p, I, dict(O, dbeta=(D["S1"] - D["dz"][0]).float()), "dbeta")
            _rejected(p, I, dict(O, dgamma=(D["S2"] - (D["dz"] * D["xh"])[0]).float()), "dgamma")
    p = find(entry="lay_bwd", esz=esz, m=37, c=16, accum=1)[0]                                                       # CX_F_ACCUM ignored
    I = bn.make_inputs(p, CPU)
    O = bn.ideal_outputs(p, I)
    S = bn.handed_sums(p, I)
    _rejected(p, I, dict(O, dbeta=S[0].float()), "dbeta")
    _rejected(p, I, dict(O, dgamma=S[1].float()), "dgamma")


def test_a_touched_sentinel_and_a_nan_are_rejected():
    p = find(group="standalone", entry="fwd", esz=4, m=37, c=16)[0]
    I = bn.make_inputs(p, CPU)
    O = bn.ideal_outputs(p, I)
    assert bn.check(p, I, dict(O, guards={"y": False}))[1] == ["sentinel overwritten around y"]
    y = O["y"].clone()
    y[3, 3] = float("nan")
    _rejected(p, I, dict(O, y=y), "y")
    assert torch.isnan(I["xbuf"][37]).all() and not torch.isnan(I["x"]).any()

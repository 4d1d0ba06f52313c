"""The checkers of the gather numerics probes (tools/gathernumerics.py: make_inputs, check) on CPU tensors: the fp64 reference
rounded once to the storage types passes every bound of tests/test_gpu_gather_numerics.py, and the outputs of a subtly wrong
kernel — one offset dropped in the last, ragged row; the last row missing from the statistics; one channel block of a multi-block
tile zeroed; one guard element overwritten; one flipped ReLU mask in the prologue's side output — are rejected, each by the bound
that is there for it.  So the GPU test would fail for such a kernel."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("gathernumerics", os.path.join(ROOT, "tools", "gathernumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gn = _load()
# 37 rows: three wave tiles, the last with 5 rows; 48 output channels: three channel blocks
BASE = dict(route="host", K=27, kc=32, nc=48, n_out=37, n_in=42, ld=40, out32=0, stats=1, tilebook=0, pre=0, res_bcast=0, f32split=0, off=[])
CASES = [dict(BASE, esz=esz, kc=kc, out32=out32, pre=pre, route="host.%d.%d.%d.%d" % (esz, kc, out32, pre))
         for esz, kc, out32, pre in ((2, 32, 0, 0), (2, 32, 1, 0), (4, 16, 0, 0), (2, 32, 0, 1), (4, 16, 0, 1), (2, 32, 0, 2), (4, 16, 0, 2),
                                     (2, 32, 0, 3), (4, 16, 0, 3))]
IDS = [c["route"] for c in CASES]


def _case(p, form):
    I = gn.make_inputs(p, form, torch.device("cpu"))
    last = p["n_out"] - 1
    if int((I["tbl"][:, last] >= 0).sum()) == 0:
        I["tbl"][0, last] = 3
    return I, gn.ideal_outputs(p, form, I)


def _operand(p, I, O):
    return O["side"].double() if p["pre"] else I["x"].double()


@pytest.mark.parametrize("form", ["y", "bn"])
@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_rounded_reference_passes(p, form):
    I, O = _case(p, form)
    err, fails = gn.check(p, form, I, O)
    assert fails == [] and err["guards"], (err, fails)
    assert err["y"] < gn.Y_TOL[gn.y_dtype(p) == torch.float32] and err["stats0"] < gn.STATS_TOL and err["stats1"] < gn.STATS_TOL


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_offset_dropped_in_the_last_ragged_row_is_rejected(p):
    I, O = _case(p, "y")
    last, operand = p["n_out"] - 1, _operand(p, I, O)
    contrib = torch.stack([operand[int(t)] @ I["w"][o].double() if int(t) >= 0 else torch.zeros(p["nc"], dtype=torch.float64)
                           for o, t in enumerate(I["tbl"][:, last])])
    o = int(contrib.abs().amax(1).argmax())
    full = gn.conv64(operand, I["w"], I["tbl"], p["n_out"]) + I["res"].double()
    O["y"][last] = (full[last] - contrib[o]).to(O["y"].dtype)
    err, fails = gn.check(p, "y", I, O)
    assert any(f.startswith("y ") for f in fails), (err, fails)


@pytest.mark.parametrize("form", ["y", "bn"])
@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_last_row_missing_from_the_statistics_is_rejected(p, form):
    I, O = _case(p, form)
    lo, last = p["n_out"] // 16 * 16, p["n_out"] - 1
    part = {k: (v[lo:last] if k == "bn_x" else v) for k, v in I.items()}
    O["stats"][-1] = gn.stats64(p, form, part, O["y"][lo:last]).float()
    err, fails = gn.check(p, form, I, O)
    assert any(f.startswith("stats") for f in fails), (err, fails)


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_zeroed_channel_block_is_rejected(p):
    I, O = _case(p, "y")
    O["y"][16:32, 16:32] = 0          # the second of three channel blocks, in the second wave tile
    O["stats"][1] = gn.stats64(p, "y", I, O["y"][16:32]).float()      # (statistics of the stored rows stay consistent)
    err, fails = gn.check(p, "y", I, O)
    assert [f for f in fails if f.startswith("y ")] and not [f for f in fails if f.startswith("stats")], (err, fails)


@pytest.mark.parametrize("where", ["before", "after"])
@pytest.mark.parametrize("name", ["y", "stats", "side"])
def test_overwritten_guard_element_is_rejected(name, where):
    p = CASES[5]
    I, O = _case(p, "y")
    buf = O["bufs"][name]
    row = gn.G - 1 if where == "before" else buf.shape[0] - gn.G
    buf[row, -1 if where == "before" else 0] = 1.0
    O["guards"] = {k: gn.intact(b) for k, b in O["bufs"].items()}
    err, fails = gn.check(p, "y", I, O)
    assert not err["guards"] and fails == ["guards overwritten: " + name], (err, fails)


def test_statistics_row_past_the_reported_count_is_rejected():
    buf = gn.guarded(4, 8, torch.float32, torch.device("cpu"))
    assert gn.intact(buf) and gn.intact(buf, 2)
    gn.inner(buf)[1, 0] = 2.0
    assert gn.intact(buf, 2) and not gn.intact(buf, 1)


@pytest.mark.parametrize("p", [c for c in CASES if c["pre"]], ids=[c["route"] for c in CASES if c["pre"]])
def test_one_relu_mask_flip_in_side_is_rejected(p):
    I, O = _case(p, "y")
    ga, be, x = I["gamma"].double(), I["beta"].double(), I["x"].double()
    if p["pre"] == 1:     # a negative pre-activation stored as it is
        R = gn.side64(p, I)
        v = (x - R["mean"]) * R["invstd"] * ga + be
        r, c = divmod(int(v.argmin()), p["kc"])
        assert float(v[r, c]) < 0
        O["side"][r, c] = v[r, c].to(O["side"].dtype)
    else:                 # a masked gradient let through
        xh, mask = gn.bn_front(I["aux"], I["mean"], I["invstd"], I["gamma"], I["beta"])
        leak = (ga * I["invstd"].double() * x * (1 - mask)).abs()
        r, c = divmod(int(leak.argmax()), p["kc"])
        O["side"][r, c] = (O["side"][r, c].double() + ga[c] * I["invstd"][c].double() * x[r, c]).to(O["side"].dtype)
    err, fails = gn.check(p, "y", I, O)
    assert any(f.startswith("side") for f in fails), (err, fails)

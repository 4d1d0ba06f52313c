"""What the kernels behind doda_spconv_gather_ex COMPUTE, for every instantiation the route plan (csrc/gather_plan.hpp) can reach:
tests/test_gpu_gather_routes.py pins which kernel a call reaches, this file compares one call per reachable instantiation
(tests/data/gather_numerics.json, generated from the plan: tools/gathernumerics.py; all 247 compiled names — the plan's predicates
decide what is compiled, and tests/test_gather_plan_host.py holds admitted, compiled and probed names to one set) with an fp64
reference on the device: per offset index_select, then matmul.

Each probe is the smallest shape at which its kernel can still go wrong: a ragged last wave tile (37 rows, or a threshold
16 (W - 1) + 1), a 300-voxel plane for the tile kernels (a full and a 44-row tile, six idle persistent workgroups), tables with
absent neighbours and empty rows, ld = n_out + 3, n_in != n_out, a dense residual, every sliced operand between guard rows.
Prologue routes get real totals (kind 1) or BatchNorm-backward operands whose ReLU mask the input decides (kinds 2 and 3);
statistics routes run in both epilogue forms.  Bounds, all from existing tests: y 1e-4 (fp32 rows) or 2^-7 (bf16 rows) of the
largest value, each statistics sum 1e-5, side 2^-7 / 2e-5 (kind 1) and 2^-6 / 2e-4 (kinds 2, 3), dgamma / dbeta rtol 2e-3.

The LDS-staged kernels (conv_tile, conv_tile16) and the persistent conv_wlds48 run once more over DESIGNED tilebooks
(tests/data/gather_tile_class.json, groups gn.TILE_GROUPS): tables of 777 and 1031 tiles whose tiles are built from recipes — exactly
960, 961, 1023 and 1024 distinct rows, rows from both ends of the input (the builder's hash + sort form), one row, none, a ragged
last tile — and placed, by the kernels' tile schedule restated in Python, so that a persistent workgroup runs them one after the
other.  Every output row is compared with fp64, every workgroup's statistics row with the sums over exactly its tiles, and the
built tilebook with a numpy restatement.

One fresh child process per group (tools/gatherroutes.py --numerics GROUP); after a child that ended on a signal or at its
time limit the remaining groups fail without starting one."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "gatherroutes.py")


def _load():
    spec = importlib.util.spec_from_file_location("gathernumerics", os.path.join(ROOT, "tools", "gathernumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gn = _load()
TIMEOUT = 60       # seconds per child: process start (torch, the library) plus the few seconds the largest group's calls take
_dead = []      # groups whose child ended on a signal or at its time limit


@pytest.mark.parametrize("group", gn.GROUPS)
def test_every_reachable_instantiation_matches_fp64(native_lib, group):
    if _dead:
        pytest.fail("not started: the child of group %s ended on a signal or at its time limit" % _dead[0])
    probes = [p for p in gn.load_probes() if p["group"] == group]
    assert probes
    env = dict(os.environ, DODA_TRACE_GATHER="1")
    env.pop("DODA_F32_SPLIT_ROWS", None)
    if group == "f32split":
        env["DODA_F32_SPLIT_ROWS"] = "0"
    try:
        r = subprocess.run([sys.executable, TOOL, "--numerics", group], env=env, capture_output=True, text=True, timeout=TIMEOUT,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append(group)
        raise
    if r.returncode < 0 or "illegal memory access" in r.stderr:      # a signal, or a fault the child reported before it ended
        _dead.append(group)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    want = [(p, form) for p in probes for form in (("y", "bn") if p["stats"] else ("y",))]
    assert len(res) == len(want)
    f32 = lambda p: p["esz"] == 4 or bool(p["out32"])
    for (p, form), got in zip(want, res):
        e = got.get("err", {})
        print("%s %s n_out=%d n_in=%d: %s" % (got["route"], form, p["n_out"], p["n_in"], json.dumps(e)))
        assert got["status"] == 0 and got["want"] == p["route"] and got["form"] == form, got
        assert got["route"] == p["route"] and got["grid"] == p["grid"], got      # the route the planner predicted for this probe
        assert e["y"] < gn.Y_TOL[f32(p)], got
        if p["stats"]:
            assert got["rows"] == p["parts"] and e["stats0"] < gn.STATS_TOL and e["stats1"] < gn.STATS_TOL, got
        if p["pre"]:
            assert e["side"] < gn.SIDE_TOL[(p["pre"], p["esz"])], got
            if p["pre"] == 1:
                assert e["side_neg"] == 0 and max(e["mean"], e["invstd"], e["rm"], e["rv"]) <= 1.0 and e["nbt"] == 0, got
            else:
                assert e["dgamma"] <= 1.0 and e["dbeta"] <= 1.0, got     # (|a - b| <= rtol |b| + rtol max |b|, rtol 2e-3)
        assert e["guards"] is True and got["fails"] == [], got


@pytest.mark.parametrize("group", gn.TILE_GROUPS)
def test_tile_kernels_over_designed_tilebooks_match_fp64(native_lib, group):
    """Per probe, layout (forward, data gradient) and statistics form: the traced route and grid are the planned ones; y within
    1e-4 of the largest value (fp32 rows) or elementwise within 2^-7 |ref| + 1e-5 max |ref| (bf16 rows: printed as the largest
    ratio error / bound); rows without a neighbour — the empty tiles — bit-equal to the residual; the statistics totals within
    1e-5 and every workgroup's row within D 2^-24 sum |addend| of the fp64 sums over its own tiles (ratio printed, D: the fp32
    additions on the way into the row, gn.stats_chain); guards intact; a repeated call bit-equal; the pipelined and the dual
    kernels bit-equal to the plain conv_tile.  And the tilebook of the group's table equals the numpy restatement."""
    if _dead:
        pytest.fail("not started: the child of group %s ended on a signal or at its time limit" % _dead[0])
    probes = [p for p in gn.load_tile_class() if p["group"] == group]
    assert probes
    env = dict(os.environ, DODA_TRACE_GATHER="1")
    env.pop("DODA_F32_SPLIT_ROWS", None)
    try:
        r = subprocess.run([sys.executable, TOOL, "--numerics", group], env=env, capture_output=True, text=True, timeout=TIMEOUT,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append(group)
        raise
    if r.returncode < 0 or "illegal memory access" in r.stderr:
        _dead.append(group)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    table = probes[0]["table"]
    assert res[0]["tilebook"] == table and res[0]["tiles"] == gn.TILE_TABLES[table][0] and res[0]["differences"] == [], res[0]
    assert res[0]["n_over"][0] > res[0]["n_over"][1] >= 5
    want = [(p, layout, form) for p in probes for layout in p["layouts"] for form in (("y", "bn") if p["stats"] else ("y",))]
    assert len(res) - 1 == len(want)
    for (p, layout, form), got in zip(want, res[1:]):
        e = got.get("err", {})
        print("%s %s layout %d %s: %s" % (got["route"], table, layout, form, json.dumps(e)))
        assert got["status"] == 0 and (got["want"], got["table"], got["layout"], got["form"]) == (p["route"], table, layout, form), got
        assert got["route"] == p["route"] and got["grid"] == p["grid"], got
        if p["esz"] == 4 or p["out32"]:
            assert e["y"] < gn.Y_TOL[True], got
        else:
            assert e["y"] <= 1.0, got
        assert e["bare"] == 0, got
        if p["stats"]:
            assert got["rows"] == p["parts"] and e["stats0"] < gn.STATS_TOL and e["stats1"] < gn.STATS_TOL, got
            assert e["part0"] <= 1.0 and e["part1"] <= 1.0, got
        assert e["guards"] is True and e["repeat"] is True, got
        if p["plain"] and form == "y":
            assert e["plain"] is True, got
        assert got["fails"] == [], got

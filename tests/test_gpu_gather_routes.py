"""doda_spconv_gather_ex after the route plan (csrc/gather_plan.hpp): every probe of tools/gatherroutes.py up to 200 000 rows, made
in one fresh child process with DODA_TRACE_GATHER=1, reaches the kernel, grid, workgroup size and statistics rows that
tests/data/gather_routes.json records (a kernel trace of the selection ladders the plan replaced); an error return has enqueued
nothing (y and the workspace keep their sentinel); and one call per kernel family, at a small shape that reaches it, matches the
fp64 reference within the bounds of tests/test_gpu_tile.py / tests/test_gpu_round4.py (1e-4 of the largest value for fp32 outputs,
one bf16 rounding step, 2^-7, for bf16 outputs)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "gatherroutes.py")
MAX_ROWS = 200000


@pytest.mark.parametrize("group", ["main", "f32split"])
def test_probes_reach_the_recorded_routes_and_errors_enqueue_nothing(native_lib, group):
    env = dict(os.environ, DODA_TRACE_GATHER="1")
    env.pop("DODA_F32_SPLIT_ROWS", None)
    if group == "f32split":
        env["DODA_F32_SPLIT_ROWS"] = "0"
    r = subprocess.run([sys.executable, TOOL, "--run", group, "--max-rows", str(MAX_ROWS)], env=env, capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    trace = [re.search(r"n_out=(\d+) .* route=(.*) grid=(\d+) block=(\d+) parts=(\d+)$", l) for l in r.stderr.splitlines()
             if l.startswith("doda_gather ")]
    table = {t["name"]: t for t in json.load(open(os.path.join(ROOT, "tests", "data", "gather_routes.json")))[group]}
    assert len(res) == len(trace) >= (4 if group == "f32split" else 100) and all(trace)
    errors = 0
    for got, tr in zip(res, trace):
        want = table[got["name"]]
        assert got["status"] == want["status"], got
        if want["status"] != 0:
            errors += 1
            assert tr[2] == "none" and got["y_kept"] and got["ws_kept"], got      # nothing ran: not even the weight pack
            continue
        assert (tr[2], int(tr[3]), int(tr[4])) == (want["kernel"], want["grid"], want["block"]), (got, tr.group(0))
        if want["parts"] >= 0:       # the call asked for statistics: the rows it reports are the plan's
            assert got["rows"] == int(tr[5]) == want["parts"], (got, tr.group(0))
    assert errors == (7 if group == "main" else 0)


@pytest.fixture(scope="module")
def family_calls(native_lib):
    """One call per kernel family (tools/gatherroutes.py FAMILIES) in a fresh child with the trace on: (family, result, route)."""
    env = dict(os.environ, DODA_TRACE_GATHER="1")
    env.pop("DODA_F32_SPLIT_ROWS", None)
    r = subprocess.run([sys.executable, TOOL, "--families"], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    routes = [re.search(r" route=(.*) grid=", l)[1] for l in r.stderr.splitlines() if l.startswith("doda_gather ")]
    assert len(res) == len(routes) == 13
    return list(zip(res, routes))


def test_one_call_per_family_matches_fp64(family_calls):
    seen = set()
    for res, route in family_calls:
        print("%s -> %s: %d rows, max error %.3g of the largest value" % (res["family"], route, res["rows"], res["err"]))
        if not res["fp32_out"] or res["family"] == "conv_gather":     # the call as the family's row states it reaches the family
            assert route.startswith(res["family"]), (res, route)
            seen.add(res["family"])
        assert res["err"] < (1e-4 if res["fp32_out"] else 2.0 ** -7), (res, route)
    assert len(seen) == 7

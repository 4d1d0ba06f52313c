"""What the gather-table kernels behind doda_spconv_wgrad_multi COMPUTE, for every wgrad_multi_kernel instantiation the plan
(csrc/wgrad_plan.hpp) can reach: all 50 compiled names — dense_compiled decides what is compiled, and tests/test_wgrad_plan_host.py
holds admitted, compiled and probed names to one set — against an fp64 reference on the device (per offset index_select, then
matmul).  tests/data/wgrad_numerics.json is generated from the plan (tools/wgradnumerics.py): per name the smallest ca and cb that
reach it, K = 27 or 8 as the name requires, at 37 rows (one chunk, a ragged 64-row step) and at 1100 rows (chunks of 576 and 524
rows: the fold runs), tables with absent neighbours and empty rows, ld = n_rows + 3, n_a != n_rows, each once overwriting and once
accumulating into a random base.  All probes of a group travel in ONE call, which groups them by instantiation itself; the traced
launches (DODA_TRACE_WGRAD) must be exactly the planned ones.

Bounds.  bf16 and fp32: max error against the largest entry below 1e-4 (tests/test_gpu_wgrad_call.py and its predecessors).
F32S (fp32 rows multiplied as bf16 head / tail splits; no earlier test ran it): csrc/spconv_common.hpp documents x = hi + lo + e,
|e| <= 2^-17 |x|, all four partial products kept, so a product is off by less than 2^-15.9 |x dy|, and fp32 accumulation of n
addends adds at most n 2^-24 A[e], A[e] = the fp64 sum of |x| |dy| of element e: |got - ref| <= (2^-15.9 + n 2^-24) A[e]
elementwise, n = 4 x the rows that contribute to the element (accumulating: plus the one fp32 addition of the base, 2^-24 (|base|
+ A[e])).  At 37 rows that is below 2^-15 A — a dropped partial product is ~2^-9 |x dy| per term and cannot pass; at 1100 rows
the bound is loose by construction, that shape is there for the chunking.

One fresh child process per group (tools/wgradnumerics.py --numerics GROUP); after a child that ended on a signal, at its time
limit or with an illegal memory access in its output the remaining groups fail without starting one."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "wgradnumerics.py")


def _load():
    spec = importlib.util.spec_from_file_location("wgradnumerics", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wn = _load()
TIMEOUT = 60       # seconds per child: process start (torch, the library) plus one call of at most 72 jobs of at most 1100 rows
_dead = []      # groups whose child ended on a signal, at its time limit or after a fault


@pytest.mark.parametrize("group", wn.GROUPS)
def test_every_reachable_instantiation_matches_fp64(native_lib, group):
    if _dead:
        pytest.fail("not started: the child of group %s ended on a signal, at its time limit or after a fault" % _dead[0])
    probes = [p for p in wn.load_probes() if p["group"] == group]
    assert probes
    env = dict(os.environ, DODA_TRACE_WGRAD="1")
    env.pop("DODA_F32_WGRAD_SPLIT_ROWS", None)
    if group == "f32split":
        env["DODA_F32_WGRAD_SPLIT_ROWS"] = "0"
    try:
        r = subprocess.run([sys.executable, TOOL, "--numerics", group], env=env, capture_output=True, text=True, timeout=TIMEOUT,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append(group)
        raise
    if r.returncode < 0 or "illegal memory access" in r.stdout + r.stderr:
        _dead.append(group)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    traced = [(t["trace"], t["grid"], t["block"], t["jobs"]) for t in res if "trace" in t]
    kernels = [t for t in traced if t[0].startswith("wgrad_multi_kernel")]
    assert kernels == [(name, blocks, 256, jobs) for name, blocks, jobs in wn.planned_launches(probes)], traced
    # the rest of the call: one fold over the jobs with partials whose element count is a multiple of four, a scalar reduce each for the others
    with_partial = [(p, acc) for p in probes for acc in (0, 1) if acc or p["R"] > 1]
    scalar = sum(1 for p, _ in with_partial if p["K"] * p["ca"] * p["cb"] % 4)
    rest = [t for t in traced if not t[0].startswith("wgrad_multi_kernel")]
    assert [t[0] for t in rest] == ["wgrad_reduce_multi"] + ["wgrad_reduce"] * scalar and rest[0][3] == len(with_partial) - scalar, traced
    got = [g for g in res if "trace" not in g]
    want = [(p, acc) for p in probes for acc in (0, 1)]
    assert len(got) == len(want)
    for (p, acc), g in zip(want, got):
        print("%s n_rows=%d accumulate=%d: %s" % (g["route"], g["n_rows"], g["accumulate"], json.dumps(g["err"])))
        assert (g["route"], g["n_rows"], g["accumulate"]) == (p["route"], p["n_rows"], acc), g
        assert g["fails"] == [], g
        if group == "f32split":
            assert g["err"]["split_ratio"] <= 1.0, g
        else:
            assert g["err"]["max_rel"] < wn.TOL, g

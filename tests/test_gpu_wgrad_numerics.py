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

The other three kernel classes — wgrad_pairs_kernel<TA, TB>, wgrad_dma16, wgrad_wide — have a group each (pairs, tile, wide;
tests/data/wgrad_class_numerics.json, generated from the plan and held to it by tests/test_wgrad_plan_host.py).  tile and wide run
over synthetic tables of 37 and 1100 rows whose 256-row tiles are built from recipes (tools/wgradnumerics.py design_table): a local
tile, the largest tile that keeps its list (1023 distinct rows), the smallest without one (1024), a scattered one and a ragged last
one, in two arrangements, so that the gather-table plan's chunk boundary at row 576 falls once into an unlisted and once into a
listed tile; the tilebook's distinct counts are checked against numpy's.
  wide   one job per compiled slice shape at the smallest channel pair that reaches it — (2,3), (1,4) and (1,3) ran in no earlier
         test —, 96 -> 144 (two by three slices) and 224 -> 224 (fourteen by two), all in one launch; every result is also bit-equal
         to the same job without a tilebook (the gather-table kernel), as spconv_wwide.hip promises.
  tile   the twelve channel pairs of 16 .. 64 channels that are not the wide class's, alone and in compositions that put the
         kernel's block-major chunking into every regime (fewer items than workgroups, a workgroup with two and with three blocks,
         a full launch of 16 blocks and a shorter one, an unlisted tile first, last and twice in a row, the one ragged tile); the
         sums of a tile job depend on its call, so only a repeated identical call must be bit-equal.
  pairs  lists exported from tables whose per-offset pair counts inside a 2048-row range are 0, 1 and both sides of every 64-pair
         step up to 257, and larger; one and two ranges (the last one ending at pair_num), the four instantiations, 48 channels on
         either side (the ragged group), a K = 8 child table with n_a != n_rows, identity lists at 37, 2048 and 2049 rows, and a
         call of 49 jobs of one variant (MAX_GROUP = 48) plus one of another.
Every dw within 1e-4 of fp64 (largest error over the largest entry: operands are bf16, products exact in fp32), overwrite and
accumulate; the traced launches are exactly the planned ones.  Measured: profiles/r17_wgrad_class_numerics.txt.

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
TIMEOUT = 60       # seconds per child: process start (torch, the library) plus calls of at most 72 jobs of at most 2900 rows
_dead = []      # groups whose child ended on a signal, at its time limit or after a fault


def _child(group, split_rows=None):
    """the JSON lines of `tools/wgradnumerics.py --numerics group` run in a fresh process"""
    if _dead:
        pytest.fail("not started: the child of group %s ended on a signal, at its time limit or after a fault" % _dead[0])
    env = dict(os.environ, DODA_TRACE_WGRAD="1")
    env.pop("DODA_F32_WGRAD_SPLIT_ROWS", None)
    if split_rows is not None:
        env["DODA_F32_WGRAD_SPLIT_ROWS"] = split_rows
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
    return traced, [g for g in res if "trace" not in g]


@pytest.mark.parametrize("group", wn.GROUPS)
def test_every_reachable_instantiation_matches_fp64(native_lib, group):
    probes = [p for p in wn.load_probes() if p["group"] == group]
    assert probes
    traced, got = _child(group, "0" if group == "f32split" else None)
    kernels = [t for t in traced if t[0].startswith("wgrad_multi_kernel")]
    assert kernels == [(name, blocks, 256, jobs) for name, blocks, jobs in wn.planned_launches(probes)], traced
    # the rest of the call: one fold over the jobs with partials whose element count is a multiple of four, a scalar reduce each for the others
    with_partial = [(p, acc) for p in probes for acc in (0, 1) if acc or p["R"] > 1]
    scalar = sum(1 for p, _ in with_partial if p["K"] * p["ca"] * p["cb"] % 4)
    rest = [t for t in traced if not t[0].startswith("wgrad_multi_kernel")]
    assert [t[0] for t in rest] == ["wgrad_reduce_multi"] + ["wgrad_reduce"] * scalar and rest[0][3] == len(with_partial) - scalar, traced
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


@pytest.mark.parametrize("group", wn.CLASS_GROUPS)
def test_every_class_probe_matches_fp64(native_lib, group):
    """(the child makes one call for the wide group and its gather-table twin, two for the pair group, and one per composition,
    mode and repeat for the tile group: tables of at most 2900 rows)"""
    rec = wn.load_class_probes()
    traced, res = _child(group)
    assert traced == wn.class_launches(group, rec), traced
    books = [g for g in res if "tilebook" in g]
    got = [g for g in res if "probe" in g]
    assert len(books) + len(got) == len(res)
    # the tilebooks of the designed tables: a listed tile's count is numpy's, an unlisted one's is above 1023
    assert len(books) == {"pairs": 0, "tile": 3, "wide": 3 * len(rec["wide"])}[group]
    for b in books:
        assert b["ok"] and len(b["ucount"]) == len(b["distinct"]), b
        assert all(u == d if d <= wn.TILE_LMAX else u > wn.TILE_LMAX for u, d in zip(b["ucount"], b["distinct"])), b
    if group != "pairs":
        assert {tuple(b["distinct"][1:3]) for b in books if len(b["distinct"]) == 5} == {(1023, 1024), (1024, 1023)}
    want = wn.class_results(group, rec)
    assert len(got) == len(want)
    for (name, shape, acc), g in zip(want, got):
        print("%s [%s] accumulate=%d: %s" % (g["probe"], g["shape"], g["accumulate"], json.dumps(g["err"])))
        assert (g["probe"], g["shape"], g["accumulate"]) == (name, shape, acc), g
        assert g["fails"] == [], g
        assert g["err"]["max_rel"] < wn.TOL, g
        if group == "wide":
            assert g["bit_equal"] is True, g        # with the gather-table kernel, in both modes
        if group == "tile":
            assert g["repeat_equal"] is True, g
    if group == "wide":
        assert {(p["ta"], p["tb"]) for p in rec["wide"]} == set(wn.WIDE_SHAPE_PAIRS) and len(wn.WIDE_SHAPE_PAIRS) == 8
    if group == "tile":
        assert {g["probe"] for g in got} == {"tile %d->%d" % p for p in wn.TILE_PAIRS}
    if group == "pairs":
        assert len([g for g in got if g["probe"].startswith("pairs tiny")]) == wn.MAX_GROUP + 2

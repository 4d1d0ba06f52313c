"""doda_amd/csrc/wgrad_plan.hpp on the CPU: which kernel class takes a weight-gradient job, which wgrad_multi_kernel instantiation
runs a gather-table job over which row chunks, and how much workspace the call needs, are pure host functions, so they are checked
without a GPU.  A stand-alone program (tests/host/wgrad_plan_main.cpp, g++, once more with -fsanitize=address,undefined) answers
for a sweep of 15 704 single-job lists, asserted against tests/data/wgrad_plan_parent.json: what
doda_spconv_wgrad_multi_workspace_bytes returned for them on the commit before the selection moved into the header (the library of
this tree is held to the same record).  Both sides of every threshold are named; the instantiations dense_compiled admits (the
program's `--compiled` mode; launch_multi_variant instantiates nothing else), the wgrad_multi_kernel symbols of the built object
(tests/data/wgrad_instantiations.json), the routes of the sweep and the routes of the numerics probes of
tests/test_gpu_wgrad_numerics.py (tests/data/wgrad_numerics.json, regenerated here from the plan) are one set of 50 names: the
gather-table class.  The other three classes have their own set: the program names what it chose for a wide, pair or tile job
(slice shape and counts, PairsGeo, channel blocks and workgroups) and lists the compiled wide and pair shapes (`--shapes`); listed =
walked = probed holds for the eight wgrad_wide slice shapes and the four wgrad_pairs_kernel shapes, and
tests/data/wgrad_class_numerics.json — the pair, tile and wide probes of tests/test_gpu_wgrad_numerics.py, with wgrad_dma16's
chunking regimes asserted from its formula — is regenerated here byte for byte.  The 1e-4 bound of those probes is shown to reject
a missing row and local indices that are off by one list position."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wgrad_plan_main.cpp")


def _tool():
    spec = importlib.util.spec_from_file_location("wgradnumerics", os.path.join(ROOT, "tools", "wgradnumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wn = _tool()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def planner(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / ("plan_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], check=True)

    def ask(lines):
        return wn.ask_planner(exe, lines)
    ask.compiled = lambda: subprocess.run([exe, "--compiled"], capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    ask.shapes = lambda: subprocess.run([exe, "--shapes"], capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    return ask


@pytest.fixture(scope="module")
def swept(planner):
    lines = wn.sweep()
    return lines, planner(lines)


def test_the_planner_names_the_parents_workspace_for_every_swept_job(swept):
    lines, got = swept
    rec = wn.load_record()
    assert rec["n"] == len(lines) == len(rec["workspace_bytes"]) and rec["lines_sha256"] == wn.lines_digest(lines)
    # (the size query returns at least 256 bytes)
    bad = [(l, g, w) for l, g, w in zip(lines, got, rec["workspace_bytes"]) if max(g["partial_bytes"], 256) != w]
    assert not bad, (len(bad), bad[:5])
    assert {g["cls"] for g in got} == {"dense", "pairs", "tile", "wide"}


def test_the_library_returns_the_parents_workspace_for_every_swept_job(native_lib):
    lines = wn.sweep()
    rec = wn.load_record()
    got = wn.workspace_bytes(native_lib, lines)
    bad = [(l, g, w) for l, g, w in zip(lines, got, rec["workspace_bytes"]) if g != w]
    assert not bad, (len(bad), bad[:5])


def test_rows_are_covered(swept):
    lines, got = swept
    chunked = 0
    for l, g in zip(lines, got):
        kv = dict(w.split("=") for w in l.split())
        n, ca, cb, K = int(kv["n_rows"]), int(kv["ca"]), int(kv["cb"]), int(kv.get("K", 27))
        if g["cls"] not in ("dense", "wide"):
            assert g["R"] == 0
            continue
        chunked += 1
        assert g["R"] * g["rows_per_chunk"] >= n and (g["R"] - 1) * g["rows_per_chunk"] < n and g["rows_per_chunk"] % 64 == 0, (l, g)
        if g["cls"] == "dense":
            _, ta, tb, ogw, _ = wn.name_parts(g["route"])
            cdiv = lambda a, b: (a + b - 1) // b
            n_tag, n_tbg, n_og = cdiv(ca, 16) // ta, cdiv(cb, 16) // tb, cdiv(K, 4 * ogw)
            assert n_tag * ta == cdiv(ca, 16) and n_tbg * tb == cdiv(cb, 16) and 4 * ogw * n_og >= K, (l, g)
            assert g["blocks"] == g["R"] * n_tag * n_tbg * n_og, (l, g)
    assert chunked > 12000


def routes(planner, *lines):
    return [(g["cls"], g["route"]) for g in planner(list(lines))]


def test_wdma_min_rows_with_pair_lists_present(planner):
    """32 767 rows go to the pair lists, 32 768 to the tile kernel; without lists the tile kernel takes both; the switch moves it."""
    got = routes(planner, "n_rows=32767 tilebook=1 pairs=1", "n_rows=32768 tilebook=1 pairs=1", "n_rows=32767 tilebook=1",
                 "n_rows=32767 tilebook=1 pairs=1 sw.wdma_min_rows=32767", "n_rows=32768 tilebook=1 pairs=1 sw.wdma_min_rows=32769")
    assert got == [("pairs", "wgrad_pairs_kernel<1, 1>"), ("tile", "wgrad_dma16"), ("tile", "wgrad_dma16"), ("tile", "wgrad_dma16"),
                   ("pairs", "wgrad_pairs_kernel<1, 1>")]


def test_wdma_off_no_pairs_and_no_table(planner):
    got = routes(planner, "n_rows=40000 tilebook=1 sw.wdma=0", "n_rows=40000 tilebook=1 pairs=1 sw.wdma=0",
                 "n_rows=40000 pairs=1 sw.no_pairs=1", "n_rows=40000 pairs=1 sw.no_pairs=1 tbl=0", "n_rows=40000 ca=64 cb=64 tilebook=1 sw.wdma=0")
    assert got == [("dense", "wgrad_multi_kernel<BF16, 1, 1, 4, true>"), ("pairs", "wgrad_pairs_kernel<1, 1>"),
                   ("dense", "wgrad_multi_kernel<BF16, 1, 1, 4, true>"), ("pairs", "wgrad_pairs_kernel<1, 1>"), ("wide", "wgrad_wide")]


def test_the_wide_class_takes_48_to_224_channels(planner):
    """Both sides of both limits, on both operands: below 48 the 16 x 16 tile kernel, above 224 (or off the 16-channel grid, or with
    pair lists) the gather-table kernel or the lists."""
    job = lambda ca, cb, more="": "n_rows=5000 ca=%d cb=%d tilebook=1 %s" % (ca, cb, more)
    got = [c for c, _ in routes(planner, job(48, 48), job(32, 48), job(48, 32), job(224, 224), job(240, 224), job(224, 240), job(64, 64),
                                job(48, 41), job(96, 96, "pairs=1"), job(96, 96, "esz=4"), job(96, 96, "K=8"), job(96, 96, "dw_al=4"))]
    assert got == ["wide", "tile", "tile", "wide", "dense", "dense", "wide", "dense", "pairs", "dense", "dense", "dense"]


def test_three_by_three_blocks_only_for_bf16_with_more_than_8_offsets_and_33_to_48_channels(planner):
    job = lambda ca, cb, more="": "n_rows=5000 ca=%d cb=%d %s" % (ca, cb, more)
    got = [r for _, r in routes(planner, job(33, 33), job(48, 48), job(32, 48), job(48, 32), job(49, 48), job(48, 49), job(48, 48, "K=9"),
                                job(48, 48, "K=8"), job(48, 48, "esz=4"), job(48, 48, "sw.no33=1"))]
    k = "wgrad_multi_kernel<%s>"
    assert got == [k % "BF16, 3, 3, 2, false", k % "BF16, 3, 3, 2, true", k % "BF16, 2, 1, 4, true", k % "BF16, 1, 2, 4, true",
                   k % "BF16, 2, 1, 4, false", k % "BF16, 1, 2, 4, false", k % "BF16, 3, 3, 2, true", k % "BF16, 1, 1, 2, true",
                   k % "F32, 1, 1, 7, true", k % "BF16, 1, 1, 4, true"]
    # DODA_WGRAD_T33: 128 blocks over four offset groups are 32 chunks at most; 5 000 rows allow nine of 512 rows or more; with
    # DODA_WGRAD_MIN_ROWS=64 the 32 chunks of 157 rows are rounded up to 192 rows each, which leaves 27
    a, b, c = planner([job(48, 48), job(48, 48, "sw.t33=16"), job(48, 48, "sw.min_rows=64")])
    assert (a["R"], a["rows_per_chunk"], b["R"], c["R"], c["rows_per_chunk"]) == (9, 576, 4, 27, 192)


def test_f32_split_rows_at_0_n_minus_1_and_n(planner):
    got = [r for _, r in routes(planner, *("n_rows=5000 esz=4 sw.f32_split_rows=%d" % v for v in (-1, 0, 4999, 5000, 5001)),
                                "n_rows=5000 esz=2 sw.f32_split_rows=0")]
    k = "wgrad_multi_kernel<%s, 1, 1, 7, true>"
    assert got == [k % "F32", k % "F32S", k % "F32S", k % "F32S", k % "F32", "wgrad_multi_kernel<BF16, 1, 1, 4, true>"]


def test_empty_and_invalid_jobs(planner):
    got = routes(planner, "n_rows=0", "n_rows=0 acc=1", "n_rows=10 K=29", "n_rows=10 ld=9", "n_rows=10 esz=3", "n_rows=10 tbl=0")
    assert got == [("zero", "none"), ("skip", "none")] + [("dense", "invalid")] * 4


def test_one_set_of_names(planner, swept):
    """Admitted = built = swept = probed: 50 instantiations (18 bf16, 16 fp32, 16 fp32 split); the recorded probe list is the one
    the plan generates, each name at the smallest channel counts that reach it, at 37 and at 1100 rows."""
    compiled = set(json.load(open(os.path.join(ROOT, "tests", "data", "wgrad_instantiations.json"))))
    admitted = planner.compiled()
    assert len(admitted) == len(set(admitted)) == 50
    split = planner([l + " sw.f32_split_rows=0" for l in swept[0] if "esz=4" in l])
    produced = {g["route"] for g in swept[1] + split if g["route"].startswith("wgrad_multi_kernel")}
    walked = set()
    probes = wn.generate(planner, admitted, walked)
    recorded = wn.load_probes()
    probed = {p["route"] for p in recorded}
    assert probes == wn.load_probes(compact=True)        # regenerate: python tools/wgradnumerics.py --probes PLANNER
    assert set(admitted) == compiled == produced == walked == probed, [sorted(set(admitted) ^ s) for s in (compiled, produced, walked, probed)]
    policies = [wn.name_parts(n)[0] for n in admitted]
    assert {p: policies.count(p) for p in policies} == {"BF16": 18, "F32": 16, "F32S": 16}
    for p in recorded:
        assert p["n_rows"] in wn.SHAPES and p["ld"] == p["n_rows"] + 3 and p["n_a"] != p["n_rows"], p
        assert (p["R"], p["rows_per_chunk"]) == ((1, 64) if p["n_rows"] == 37 else (2, 576)), p
    assert all(len([p for p in recorded if p["route"] == n]) == 2 for n in admitted)


def test_one_set_of_names_for_the_wide_and_pair_classes(planner):
    """Listed = walked = probed: the eight slice shapes of WW_SHAPES are the shapes ww_shape produces over every channel pair of
    48 .. 224 channels, and the shapes of the recorded wide probes; the four shapes of WP_PAIR_SHAPES are the ones pairs_geo
    produces and the recorded pair probes run.  cb = 176 and 208 (11 and 13 blocks: no slice of at most 7 blocks but 1 divides
    them) stay with the gather-table class.  The recorded list is the one the plan generates."""
    listed = [tuple(l.split()) for l in planner.shapes()]
    wide = {(int(a), int(b)) for k, a, b in listed if k == "wide"}
    pair = {"wgrad_pairs_kernel<%s, %s>" % (a, b) for k, a, b in listed if k == "pairs"}
    assert len(listed) == 12 and len(wide) == 8 and len(pair) == 4
    first, refused = wn.wide_walk(planner)
    assert refused and {cb for _, cb in refused} == {176, 208} and len(refused) == 2 * len(wn.WIDE_CHANNELS), refused
    rec = wn.generate_class(planner)
    assert wn.dump_class(rec) == open(wn.CLASS_PROBES).read()       # regenerate: python tools/wgradnumerics.py --class-probes PLANNER
    rec = wn.load_class_probes()
    assert wide == set(first) == {(p["ta"], p["tb"]) for p in rec["wide"]} == set(wn.WIDE_SHAPE_PAIRS)
    channels = (16, 32, 48, 64)
    got = planner([wn.job(n_rows=3000, ca=ca, cb=cb, pairs=1) for ca in channels for cb in channels])
    assert all(g["cls"] == "pairs" for g in got)
    assert pair == {g["route"] for g in got} == {p["route"] for p in rec["pairs"]}
    # the tile group: all twelve channel pairs, every regime of the chunking in some composition, every composition at every shape
    assert {tuple(j) for c in rec["tile"] for j in c["jobs"]} == set(wn.TILE_PAIRS) and len(wn.TILE_PAIRS) == 12
    assert {r for c in rec["tile"] for v in c["regimes"].values() for r in v} == set(wn.TILE_REGIMES)
    assert all(set(c["regimes"]) == set(wn.SHAPE_ROWS) for c in rec["tile"])
    # what the device run reports and what it must trace are functions of the record
    assert [len(wn.class_results(g, rec)) for g in wn.CLASS_GROUPS] == [86, 180, 60]
    assert len(set(wn.class_results("wide", rec))) == 60 and len(set(wn.class_results("tile", rec))) == 180


def test_the_designed_tables_hold_what_their_recipes_say():
    """tools/wgradnumerics.py design_table: the distinct rows of every tile (numpy.unique) — 1023 for the full list, 1024 just over
    it, more for the scattered tile; the chunk boundary of the gather-table plan (row 576) lies in tile 2, once unlisted, once
    listed — for the tile group's tables and for every wide probe's."""
    rec = wn.load_class_probes()
    for name in ["tile"] + [p["name"] for p in rec["wide"]]:
        for shape, n in wn.SHAPE_ROWS.items():
            t, distinct = wn.design_table(name, shape)
            assert t.shape == (27, n + 3) and t.min() == -1 and t.max() < n
            unlisted = tuple(k for k, d in enumerate(distinct) if d > wn.TILE_LMAX)
            assert unlisted == wn.UNLISTED[shape]
            if n == 1100:
                assert wn.CHUNKS[n] == (2, 576) and 576 // wn.TILE_ROWS == 2 and 576 % wn.TILE_ROWS == 64
                assert sorted(distinct[1:3]) == [1023, 1024] and len(distinct) == 5
    assert (2 in wn.UNLISTED["1100A"]) != (2 in wn.UNLISTED["1100B"])


def test_the_class_bound_rejects_a_missing_row_and_shifted_local_indices():
    """tools/wgradnumerics.py check() on the CPU, for the smallest and the largest probe of each class group: the fp64 reference
    rounded to fp32 passes in both modes; the same sum without one row's contribution, and with the local indices of one tile moved
    one list position on, misses the 1e-4 bound."""
    import torch
    rec = wn.load_class_probes()
    cases = [(wn.tile_probe(48, 48, "37", "wide"), "37", 0), (wn.tile_probe(224, 224, "1100A", "wide"), "1100A", 1),
             (wn.tile_probe(16, 16, "37"), "37", 0), (wn.tile_probe(64, 32, "1100B"), "1100B", 2)]
    pairs = {p["name"]: p for p in rec["pairs"]}
    cases += [(pairs["pairs identity 37 rows 16->16"], "identity", 0), (pairs["pairs two ranges 48->48"], "two ranges", 9)]
    for p, shape, tile in cases:
        tbl = wn.class_table(p, shape)
        I = wn.class_inputs(p, shape, tbl, torch.device("cpu"))
        R = wn.class_reference(p, I)
        side = "a" if "table" in p else "b"        # the operand the table's columns count
        col = tile * wn.TILE_ROWS + int((tbl[:, tile * wn.TILE_ROWS:I[side].shape[0]] >= 0).any(0).nonzero()[0])
        less = I[side].clone()
        less[col] = 0
        no_row = wn.class_reference(p, dict(I, **{side: less}))[0]
        shifted = wn.class_reference(p, dict(I, tbl=wn.shift_tile(tbl, tile)))[0]
        for acc in (0, 1):
            base = I["base"].double() if acc else 0.0
            err, fails = wn.check(p, I, (R[0] + base).float(), acc, R)
            assert fails == [] and err["max_rel"] < 1e-6, (p["name"], acc, err)
            for bad in (no_row, shifted):
                assert wn.check(p, I, (bad + base).float(), acc, R)[1], (p["name"], acc)


def test_the_split_bound_rejects_a_dropped_partial_product():
    """tools/wgradnumerics.py check() on the CPU: the fp64 reference rounded to fp32 passes in both modes; the same sum with dy's
    bf16 tail dropped (one of the four partial products pairs missing: ~2^-9 per term) misses the F32S bound at 37 rows, and a single
    wrong element misses the 1e-4 bound of the exact kernels."""
    import torch
    for route in ("wgrad_multi_kernel<F32S, 2, 2, 4, false>", "wgrad_multi_kernel<F32, 1, 1, 7, true>", "wgrad_multi_kernel<BF16, 3, 3, 2, true>"):
        p = next(p for p in wn.load_probes() if p["route"] == route and p["n_rows"] == 37)
        I = wn.make_inputs(p, torch.device("cpu"))
        ref, A, rows = wn.reference(p, I)
        assert float(rows.min()) < 37 and int((I["tbl"][:, :37] >= 0).any(0).sum()) < 37      # absent neighbours, empty rows
        for acc in (0, 1):
            ideal = (ref + (I["base"].double() if acc else 0.0)).float()
            err, fails = wn.check(p, I, ideal, acc)
            assert fails == [], (route, acc, err)
            if route.startswith("wgrad_multi_kernel<F32S"):
                assert err["split_ratio"] < 0.01
                lossy = dict(I, b=I["b"].bfloat16().float())
                bad = (wn.reference(p, lossy)[0] + (I["base"].double() if acc else 0.0)).float()
            else:
                bad = ideal.clone()
                bad.view(-1)[5] += 2e-4 * float(ref.abs().max())
            assert wn.check(p, I, bad, acc)[1], (route, acc)

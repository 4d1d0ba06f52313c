"""doda_amd/csrc/gather_plan.hpp on the CPU: the route plan of doda_spconv_gather_ex is one pure host function, so which kernel
instantiation a call reaches, with which grid and how many statistics rows, is checked without a GPU.  A stand-alone program
(tests/host/gather_plan_main.cpp, g++, once more with -fsanitize=address,undefined) answers for the probe list of
tools/gatherroutes.py — asserted against tests/data/gather_routes.json, the routes recorded on an MI355X (kernel trace) from the
ladders the plan replaced — and for a dense sweep over row counts, whose routes must be compiled instantiations
(tests/data/gather_instantiations.json, the kernel symbols of the three code objects) with grids that cover the rows.  An extended sweep (tools/gathernumerics.py: out32, the prologue kinds, K, kc,
the broadcast residual, every switch off, f32_split_rows = 0) settles every compiled name: the instantiations the predicates of
gather_plan.hpp admit (the program's `--compiled` mode; the launchers instantiate nothing else), the kernel symbols of the built
objects, the routes of that sweep and the routes of the numerics probes of tests/test_gpu_gather_numerics.py
(tests/data/gather_numerics.json, regenerated here from the plan) are one set of 247 names."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "gather_plan_main.cpp")


def _probes():
    spec = importlib.util.spec_from_file_location("gatherroutes", os.path.join(ROOT, "tools", "gatherroutes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _numerics():
    spec = importlib.util.spec_from_file_location("gathernumerics", os.path.join(ROOT, "tools", "gathernumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def planner(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_plan") / ("plan_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [re.match(r"status=(-?\d+) route=(.*) grid=(\d+) block=(\d+) parts=(\d+) frags=(\d+) wbytes=(\d+)$", l)
               for l in r.stdout.splitlines()]
        assert len(out) == len(lines) and all(out)
        return [dict(status=int(m[1]), route=m[2], grid=int(m[3]), block=int(m[4]), parts=int(m[5]), frags=int(m[6]))
                for m in out]
    ask.compiled = lambda: subprocess.run([exe, "--compiled"], capture_output=True, text=True, check=True, timeout=300).stdout.splitlines()
    ask.constants = lambda: {k: int(v) for k, v in (l.split("=") for l in subprocess.run(
        [exe, "--constants"], capture_output=True, text=True, check=True, timeout=300).stdout.splitlines())}
    return ask


def test_probe_list_reaches_the_recorded_routes(planner):
    gr = _probes()
    table = json.load(open(os.path.join(ROOT, "tests", "data", "gather_routes.json")))
    for group in ("main", "f32split"):
        ps = gr.probes(group)
        rec = table[group]
        assert [p["name"] for p in ps] == [r["name"] for r in rec]
        for p, r, got in zip(ps, rec, planner([gr.plan_line(p, group) for p in ps])):
            assert got["status"] == r["status"] == p["err"], (p["name"], got)
            if r["status"] != 0:
                assert got["route"] == "none" and got["grid"] == 0
                continue
            assert (got["route"], got["grid"], got["block"]) == (r["kernel"], r["grid"], r["block"]), (p["name"], got, r)
            if r["parts"] >= 0:     # (recorded where the call asked for statistics)
                assert got["parts"] == r["parts"], (p["name"], got, r)
            if r["pack"]:           # the pack kernel the call enqueues first: one thread per fragment
                wide = p["esz"] == 2 and not got["route"].startswith("conv_gather") and (
                    (p["kc"] >= 32 and p["kc"] % 8 == 0) or (p["kc"] == 16 and p["K"] >= 2))
                name = "pack_weights_wide" if wide else "pack_weights<%s>" % ("F32" if p["esz"] == 4 else "BF16")
                assert r["pack"] == [name, (got["frags"] + 255) // 256, 256], (p["name"], got, r)


def test_conv_tile16_starts_at_769_tiles(planner):
    """196 608 rows are 768 tiles, 196 609 are 769: DODA_TILE16_MIN_TILES' default, and the switch that moves it."""
    got = planner(["kc=16 nc=16 tilebook=1 n_out=196608", "kc=16 nc=16 tilebook=1 n_out=196609",
                   "kc=16 nc=16 tilebook=1 n_out=196609 sw.tile16_min_tiles=770", "kc=16 nc=16 tilebook=1 n_out=196609 sw.tile_pipeline=0"])
    assert [g["route"] for g in got] == ["conv_tile<0, false, false, 1, false>", "conv_tile16<false, false>",
                                         "conv_tile<0, false, false, 1, false>", "conv_tile<0, false, false, 1, false>"]
    assert [g["grid"] for g in got] == [768, 512, 768, 768]


def _sweep_rows():
    rows = set(range(1, 80)) | set(range(4099, 300001, 4099)) | {300000}
    for wf in (170, 171, 256, 341, 342, 512, 682, 683, 1024, 2048, 4096, 8192, 12288, 16384):   # thresholds, in 16-row tiles (/ NB)
        rows |= set(range(16 * (wf - 3), 16 * (wf + 3) + 2))
    return sorted(r for r in rows if 1 <= r <= 300000)


def test_every_route_of_a_dense_sweep_is_compiled_and_covers_its_rows(planner):
    compiled = set(json.load(open(os.path.join(ROOT, "tests", "data", "gather_instantiations.json"))))
    calls = []
    for n in _sweep_rows():
        for nc in (16, 32, 48, 64, 96):
            for esz in (2, 4):
                for stats in (0, 1):
                    for kc, K, n_in, tb, pre in ((16, 27, n, 0, 0), (16, 27, n, 1, 0), (32, 27, n, 0, 0), (32, 27, n, 1, 0), (48, 27, n, 0, 0),
                                                 (32, 8, n // 4 + 1, 0, 0), (32, 27, n, 0, 1), (16, 1, n, 0, 0), (3, 27, n, 0, 0)):
                        calls.append(dict(n_out=n, nc=nc, esz=esz, stats=stats, kc=kc, K=K, n_in=n_in, tilebook=tb, pre_kind=pre))
    got = planner([" ".join("%s=%d" % it for it in c.items()) for c in calls])
    cdiv = lambda a, b: (a + b - 1) // b
    seen = set()
    for c, g in zip(calls, got):
        n, NB = c["n_out"], cdiv(c["nc"], 16)
        if g["status"] != 0:      # the only rejections of this sweep: statistics on the generic kernel, a prologue on 16-byte-less rows
            assert g["status"] == -4 and g["route"] == "none", (c, g)
            continue
        assert g["route"] in compiled, (c, g)
        seen.add(g["route"])
        fam, args = re.match(r"(\w+)<(.*)>$", g["route"]).groups()
        a = [s.strip() for s in args.split(",")]
        nt = cdiv(n, 256)
        if c["tilebook"] and c["esz"] == 2 and c["kc"] == 16 and c["K"] == 27 and c["nc"] == 16:   # 16 -> 16 over a tilebook: the tile count decides
            assert fam == ("conv_tile16" if nt >= 769 else "conv_tile"), (c, g)
        if fam in ("conv_fast", "conv_gather"):
            nbw, s = int(a[1]), int(a[2])
            split = fam == "conv_fast" and a[5] == "true"
            rpb = (1 if split else 4) * 16 * s
            assert g["block"] == 256 and g["grid"] == cdiv(n, rpb) * cdiv(NB, nbw), (c, g)
            assert (g["grid"] // cdiv(NB, nbw)) * rpb >= n
            assert g["parts"] == (cdiv(n, rpb) if fam == "conv_fast" else 0), (c, g)
            if fam == "conv_fast":
                assert (a[6] == "true") == bool(c["stats"]) and int(a[7]) == c["pre_kind"], (c, g)
        elif fam == "conv_up32":
            assert g["grid"] == g["parts"] == nt and g["block"] == 256 and g["grid"] * 256 >= n, (c, g)
        elif fam == "conv_tile16":
            assert g["grid"] == g["parts"] == 512 and nt >= 769 and NB == 1 and g["block"] == 256, (c, g)
        elif fam == "conv_tile":
            cap = 768 if a[0] == "0" else 512
            assert g["grid"] == g["parts"] == min(cdiv(nt, 8) * 8, cap) and g["block"] == 256, (c, g)
            assert not c["stats"] or NB <= int(a[3]), (c, g)      # the statistics of every channel block fit the instantiation
        else:
            assert fam == "conv_wlds48" and g["block"] == 512 and g["parts"] == nt and g["grid"] == min(nt, 256), (c, g)
    assert {re.match(r"\w+", r).group(0) for r in seen} == {"conv_fast", "conv_gather", "conv_up32", "conv_tile", "conv_tile16", "conv_wlds48"}


def test_extended_sweep_settles_every_instantiation(planner):
    """The names the predicates admit, the compiled names, the routes of the extended sweep and the routes of the numerics probes are
    the same 247; the recorded probe list is the one the plan generates, and every probe is the smallest shape with a ragged last
    wave tile."""
    gn = _numerics()
    compiled = set(json.load(open(os.path.join(ROOT, "tests", "data", "gather_instantiations.json"))))
    admitted = planner.compiled()
    assert len(admitted) == len(set(admitted)) == 247
    produced = set()
    probes = gn.generate(planner, produced)
    recorded = gn.load_probes()
    probed = {p["route"] for p in recorded}
    assert set(admitted) == compiled == produced == probed, [sorted(set(admitted) ^ s) for s in (compiled, produced, probed)]
    families = [re.match(r"\w+", n).group(0) for n in admitted]
    assert {f: families.count(f) for f in families} == {"conv_fast": 200, "conv_gather": 16, "conv_tile": 21, "conv_tile16": 4,
                                                        "conv_up32": 4, "conv_wlds48": 2}
    assert probes == recorded        # regenerate: see tools/gathernumerics.py generate()
    assert {p["group"] for p in recorded} == set(gn.GROUPS)
    # the planner names the recorded route for the recorded shape, and no probe has only full wave tiles
    for p, g in zip(recorded, planner([gn.plan_line(p) for p in recorded])):
        assert (g["status"], g["route"], g["grid"], g["parts"]) == (0, p["route"], p["grid"], p["parts"]), (p, g)
        assert p["n_out"] % 16 != 0 and p["n_out"] >= 37 and p["ld"] == p["n_out"] + 3 and p["n_in"] != p["n_out"], p
        assert not p["res_bcast"] or p["group"].startswith("fast")


def test_tile_class_probes_regenerate_and_cover_every_tile_kernel(planner):
    """tests/data/gather_tile_class.json (the probes of the LDS-staged kernels over designed tilebooks, tools/gathernumerics.py) is
    the list the plan generates; the names it probes, the tile-kernel names the predicates admit and the compiled ones are one
    set of 27; the tilebook constants the generator restates are those of tilebook.hpp and gather_plan.hpp."""
    gn = _numerics()
    k = planner.constants()
    assert (k["TB_T"], k["TB_UMAX"], k["TB_LMAX"], k["TB_CAP64"], k["TB_K"], k["TB_LW"], k["TB_BITMAP_BITS"]) == (
        gn.TB_T, gn.TB_UMAX, gn.TB_LMAX, gn.TB_CAP64, gn.TB_K, gn.TB_LW, gn.TB_BITMAP_BITS) and k["TB_BITMAP_BITS"] == 196608
    widths = {w for _, _, w in gn.TILE_TABLES.values()}
    assert widths == {k["GP_TILE_MAX_GROUPS"], k["GP_TILE16_GROUPS"]} == {768, 512}
    tile = lambda names: {n for n in names if re.match(r"conv_(tile|tile16|wlds48)<", n)}
    compiled = tile(json.load(open(os.path.join(ROOT, "tests", "data", "gather_instantiations.json"))))
    admitted = planner.compiled()
    recorded = gn.load_tile_class()
    assert gn.generate_tile_class(planner, admitted) == recorded
    assert gn.dump_tile_class(recorded) == open(gn.TILE_CLASS).read()
    probed = {p["route"] for p in recorded}
    assert tile(admitted) == compiled == probed and len(probed) == 27
    families = [re.match(r"\w+", n).group(0) for n in probed]
    assert {f: families.count(f) for f in families} == {"conv_tile": 21, "conv_tile16": 4, "conv_wlds48": 2}
    for name in probed:         # both arrangements of the launch width; the 1031-tile table for six names
        tables = sorted(p["table"] for p in recorded if p["route"] == name)
        w = "w768" if name.startswith("conv_tile<0") else "w512"
        assert tables == [w + "A", w + "B"] + (["w512C"] if name in gn.ON_1031 else []), (name, tables)
    on_1031 = [n for n in gn.ON_1031 if not n.startswith("conv_tile16")]
    assert len(on_1031) == 2 and on_1031[0].endswith("true>") and on_1031[1].startswith("conv_tile<2")
    for p, g in zip(recorded, planner([gn.plan_line(p) for p in recorded])):
        assert (g["status"], g["route"], g["grid"], g["parts"]) == (0, p["route"], p["grid"], p["parts"]), (p, g)
        assert p["ld"] == p["n_out"] + 3 and p["n_in"] == p["n_out"] + 5 and p["layouts"] == [0, 2] and not p["res_bcast"]
        assert (p["n_out"], p["n_in"], p["ld"]) == gn.table_rows(p["table"]) and p["n_out"] <= 264000
        assert p["group"] in gn.TILE_GROUPS
        # conv_tile<0, ., ., 1, false> at 769 tiles or more: only with the pipeline option off
        assert (p["off"] == ["tile_pipeline"]) == bool(re.match(r"conv_tile<0, \w+, \w+, 1, false>", p["route"])), p

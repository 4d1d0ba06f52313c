"""The checkers of the gather numerics probes (tools/gathernumerics.py: make_inputs, check) on CPU tensors: the fp64 reference
rounded once to the storage types passes every bound of tests/test_gpu_gather_numerics.py, and the outputs of a subtly wrong
kernel — one offset dropped in the last, ragged row; the last row missing from the statistics; one channel block of a multi-block
tile zeroed; one guard element overwritten; one flipped ReLU mask in the prologue's side output — are rejected, each by the bound
that is there for it.  So the GPU test would fail for such a kernel.

Second half: the designed tilebooks of the tile class (design_tiles, tile_schedule, tilebook_numpy, tile_check).  The recipes hold
what they promise (distinct rows, spans against the builder's bitmap, rows without neighbours, row 0 and row n_in - 1), the restated
tile schedule equals a walk over the tiles, the numpy tilebook round-trips to the table, and the checkers reject a tile computed
from the previous tile's rows, a wrong row in the last slot of a full list, a non-zero empty tile and a workgroup's statistics row
without its second tile."""
import importlib.util
import os

import numpy as np
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


# ---------------------------------------------------------------------------------------- the tile class: designed tilebooks
# (tools/gathernumerics.py, second half: design_tiles, tile_schedule, tilebook_numpy, tile_check)
ALL_BUT_LISTED = set(gn.WANTED) - {"staged -> unstaged with a list"}


def _distinct(t, n, tile):
    blk = t[:, tile * 256:min((tile + 1) * 256, n)]
    ent = blk[blk >= 0]
    return np.unique(ent), blk


@pytest.mark.parametrize("name", list(gn.TILE_TABLES))
def test_designed_table_holds_its_recipes(name):
    """Distinct counts, spans, rows without neighbours, row 0 and row n_in - 1, recomputed from the table's entries."""
    t, info = gn.design_tiles(name)
    nt, last, width = gn.TILE_TABLES[name]
    n, n_in, ld = gn.table_rows(name)
    assert t.shape == (27, n + 3) and t.dtype == np.int32 and len(info) == nt == -(-n // 256) and n <= 264000 and n % 256 == last
    assert (n_in, ld) == (n + 5, n + 3) and t[:, n:].min() >= 0 and t[:, n:].max() < n_in and t.max() < n_in and t.min() == -1
    assert {i["recipe"] for i in info} == set(gn.RECIPES) and info[-1]["recipe"] == "ragged"
    exact = {"cap64": 960, "cap64+1": 961, "full list": 1023, "just over": 1024, "one row": 1, "empty": 0}
    assert (gn.TB_CAP64, gn.TB_LMAX, gn.TB_UMAX) == (960, 1023, 1024)
    for tile, i in enumerate(info):
        uniq, blk = _distinct(t, n, tile)
        span = int(uniq[-1] - uniq[0] + 1) if len(uniq) else 0
        assert (i["U"], i["span"]) == (len(uniq), span), (tile, i)
        r = i["recipe"]
        if r in exact:
            assert len(uniq) == exact[r], (tile, i)
        if r.startswith("far"):
            assert span > gn.TB_BITMAP_BITS and uniq[0] == 0 and uniq[-1] == n_in - 1, (tile, i)
            assert len(uniq) <= 960 if r == "far listed" else len(uniq) > 1023, (tile, i)
        else:
            assert span <= gn.TB_BITMAP_BITS, (tile, i)
        if r in ("local", "ragged"):
            assert 0 < len(uniq) <= 600 and uniq[0] >= tile * 256 - 150 and uniq[-1] < tile * 256 + 256 + 150, (tile, i)
        if r == "local":        # 25 % absent, 10 % of the rows without any neighbour
            assert 0.25 < float((blk < 0).mean()) < 0.42 and 5 <= int((~(blk >= 0).any(0)).sum()) <= 60, (tile, i)
        if r == "empty":
            assert (blk == -1).all()
        if r != "empty" and r != "ragged":
            assert blk.shape[1] == 256 and (blk >= 0).any()
    assert t[:, (nt - 1) * 256:n].shape[1] == last and (t[:, (nt - 1) * 256:n] >= 0).any()
    for family, grid, cap in gn.TABLE_USERS[name]:
        assert grid == (256 if family == "conv_wlds48" else width)
        seen = gn.transitions(family, grid, cap, info)
        assert seen >= (ALL_BUT_LISTED if cap == 1023 else set(gn.WANTED)), (family, sorted(set(gn.WANTED) - seen))
        if nt == 1031:
            assert gn.CHAIN in seen, family
        tiles = gn.tile_schedule(family, grid, nt)
        assert {len(b) for b in tiles} == ({3, 4} if family == "conv_wlds48" else {1, 2} if nt == 777 else {2, 3})


@pytest.mark.parametrize("nt", [2, 769, 777, 1024, 1031])
@pytest.mark.parametrize("grid", [8, 512, 768])
def test_schedule_restatement_matches_a_walk_over_the_tiles(grid, nt):
    """tile -> (workgroup, turn), enumerated tile by tile: the XCDs own contiguous runs whose lengths differ by at most one (the
    first nt mod 8 are longer); inside a run the tiles are dealt to the XCD's grid / 8 workgroups in turn."""
    L = grid // 8
    want = [[] for _ in range(grid)]
    tile = 0
    for xcd in range(8):
        for k in range(nt // 8 + (1 if xcd < nt % 8 else 0)):
            b = (k % L) * 8 + xcd
            assert len(want[b]) == k // L
            want[b].append(tile)
            tile += 1
    assert tile == nt
    for family in ("conv_tile", "conv_tile16"):
        got = gn.tile_schedule(family, grid, nt)
        assert got == want and sorted(t for b in got for t in b) == list(range(nt))
        assert gn.stats_owner(family, grid, nt) == want
    w = gn.tile_schedule("conv_wlds48", grid, nt)
    assert len(w) == grid and all(t % grid == b for b, ts in enumerate(w) for t in ts) and all(ts == sorted(ts) for ts in w)
    assert sorted(t for b in w for t in b) == list(range(nt)) and gn.stats_owner("conv_wlds48", grid, nt) == [[t] for t in range(nt)]


def test_numpy_tilebook_round_trips_to_the_table():
    t, info = gn.design_tiles("w512B")
    n = gn.table_rows("w512B")[0]
    tb = gn.tilebook_numpy(t, n)
    over960 = over1023 = 0
    for tile, i in enumerate(info):
        uniq, blk = _distinct(t, n, tile)
        over960 += len(uniq) > 960
        over1023 += len(uniq) > 1023
        assert tb["ucount"][tile] == len(uniq)
        ent = gn.tilebook_entries(tb, tile)
        if len(uniq) > 1023:
            assert ent is None and (tb["ulist"][tile] == -2).all()
            continue
        want = np.full((27, 256), -1, np.int64)
        want[:, :blk.shape[1]] = blk
        assert np.array_equal(ent, want), tile
        # the list itself: ascending in entry order (tb_upos), -1 past the count
        e = np.arange(1024)
        logical = tb["ulist"][tile][(((e >> 5) & 7) * 32 + (e & 31)) * 4 + (e >> 8)]
        assert np.array_equal(logical[:len(uniq)], uniq) and (logical[len(uniq):] == -1).all()
    assert list(tb["n_over"]) == [over960, over1023] and over1023 >= 8 and over960 > over1023
    # a built tilebook that differs in one list entry, one local index, one count or the totals is reported
    assert gn.tilebook_differences(tb, tb) == []
    full = next(k for k, i in enumerate(info) if i["recipe"] == "full list")
    for key, where, value in (("ulist", (full, 5), 7), ("lidx", (full, 9, 255), 1), ("ucount", (full,), 1022), ("n_over", (1,), 0)):
        bad = {k: v.copy() for k, v in tb.items()}
        bad[key][where] = value
        assert gn.tilebook_differences(bad, tb), key
    over = next(k for k, i in enumerate(info) if i["recipe"] == "just over")
    bad = {k: v.copy() for k, v in tb.items()}
    bad["lidx"][over] = 77          # (a tile without a list has no local indices to compare)
    assert gn.tilebook_differences(bad, tb) == []
    bad["ucount"][over] = 1025      # (the bitmap form counts exactly)
    assert gn.tilebook_differences(bad, tb)


TILE_CASES = ["conv_tile<0, false, true, 1, false>", "conv_tile<0, true, true, 1, false>"]
_tile_cache = {}


def _tile_case(route):
    """the recorded probe of `route` on table w768A (16 -> 16, statistics), forward, on the CPU: inputs, fp64 reference, tiles"""
    if route not in _tile_cache:
        p = next(q for q in gn.load_tile_class() if q["route"] == route and q["table"] == "w768A")
        t, info = gn.design_tiles("w768A")
        I = gn.tile_inputs(p, 0, torch.device("cpu"), torch.from_numpy(t.copy()))
        _tile_cache[route] = (p, I, gn.tile_reference(p, I), info, t)
    return _tile_cache[route]


def _pair(info, first, second):
    """consecutive tiles (a, b) of one workgroup of the 768-wide launch with these recipes"""
    for tiles in gn.tile_schedule("conv_tile", 768, len(info)):
        for a, b in zip(tiles, tiles[1:]):
            if info[a]["recipe"] == first and info[b]["recipe"] == second:
                return a, b
    raise AssertionError((first, second))


def _tile_rows(p, I, ent):
    """fp64 rows of one tile computed from the [27, 256] entries `ent`"""
    return gn.conv64(I["x"].double(), I["w"], torch.from_numpy(ent).int(), 256)


@pytest.mark.parametrize("form", ["y", "bn"])
@pytest.mark.parametrize("route", TILE_CASES)
def test_tile_class_rounded_reference_passes(route, form):
    p, I, ref, info, _ = _tile_case(route)
    err, fails = gn.tile_check(p, form, I, gn.tile_ideal(p, form, I, ref), ref)
    assert fails == [] and err["y"] <= 1.0 and err["bare"] == 0 and max(err["part0"], err["part1"]) <= 1.0, (err, fails)


@pytest.mark.parametrize("route", TILE_CASES)
def test_tile_computed_from_the_previous_tiles_rows_is_rejected(route):
    """the second tile of a workgroup multiplied over the rows its first tile left in LDS: its own local indices, the other list"""
    p, I, ref, info, t = _tile_case(route)
    a, b = _pair(info, "cap64", "cap64+1")
    tb = gn.tilebook_numpy(t, p["n_out"])
    e = np.arange(1024)
    stale = tb["ulist"][a][(((e >> 5) & 7) * 32 + (e & 31)) * 4 + (e >> 8)].astype(np.int64)
    mine = gn.tilebook_entries(tb, b)
    loc = np.where(mine >= 0, np.searchsorted(np.unique(mine[mine >= 0]), mine) + 1, 0)
    wrong = np.where(loc == 0, -1, stale[np.maximum(loc - 1, 0)])
    O = gn.tile_ideal(p, "y", I, ref)
    O["y"][b * 256:(b + 1) * 256] = (_tile_rows(p, I, wrong) + I["res"][b * 256:(b + 1) * 256].double()).to(O["y"].dtype)
    err, fails = gn.tile_check(p, "y", I, O, ref)
    assert any(f.startswith("y ") for f in fails), (err, fails)


@pytest.mark.parametrize("route", TILE_CASES)
def test_wrong_row_in_the_last_slot_of_a_full_list_is_rejected(route):
    """LDS slot 1023 of a tile of 1023 distinct rows holding the row before it"""
    p, I, ref, info, t = _tile_case(route)
    f = next(k for k, i in enumerate(info) if i["recipe"] == "full list")
    ent = t[:, f * 256:(f + 1) * 256].astype(np.int64)
    uniq = np.unique(ent[ent >= 0])
    assert len(uniq) == 1023 and (ent == uniq[-1]).sum() >= 1
    wrong = np.where(ent == uniq[-1], uniq[-2], ent)
    O = gn.tile_ideal(p, "y", I, ref)
    O["y"][f * 256:(f + 1) * 256] = (_tile_rows(p, I, wrong) + I["res"][f * 256:(f + 1) * 256].double()).to(O["y"].dtype)
    err, fails = gn.tile_check(p, "y", I, O, ref)
    assert any(f.startswith("y ") for f in fails), (err, fails)


@pytest.mark.parametrize("route", TILE_CASES)
def test_non_zero_empty_tile_is_rejected(route):
    """one element of an all-absent tile one unit in the last place off the residual: inside every tolerance, not bit-equal"""
    p, I, ref, info, _ = _tile_case(route)
    k = next(k for k, i in enumerate(info) if i["recipe"] == "empty")
    O = gn.tile_ideal(p, "y", I, ref)
    assert torch.equal(O["y"][k * 256:(k + 1) * 256], I["res"][k * 256:(k + 1) * 256])
    O["y"][k * 256 + 200].view(torch.int16 if O["y"].dtype == torch.bfloat16 else torch.int32)[3] += 1
    err, fails = gn.tile_check(p, "y", I, O, ref)
    names = [f.split()[0] for f in fails]       # (the statistics rows of the copy are those of the uncorrupted y)
    assert err["bare"] == 1 and "bare" in names and "y" not in names and err["guards"], (err, fails)


@pytest.mark.parametrize("form", ["y", "bn"])
@pytest.mark.parametrize("route", TILE_CASES)
def test_statistics_row_without_its_second_tile_is_rejected(route, form):
    p, I, ref, info, _ = _tile_case(route)
    blocks = gn.tile_schedule("conv_tile", 768, len(info))
    b = next(k for k, tiles in enumerate(blocks) if len(tiles) == 2 and info[tiles[1]]["recipe"] == "one row")
    O = gn.tile_ideal(p, form, I, ref)
    a = gn.stats_addends(p, form, I, O["y"])
    first = slice(blocks[b][0] * 256, blocks[b][0] * 256 + 256)
    O["stats"][b] = torch.stack([a[0][first].sum(0), a[1][first].sum(0)]).float()
    err, fails = gn.tile_check(p, form, I, O, ref)
    assert any(f.startswith("part") for f in fails), (err, fails)

"""GPU test of the pyramid's level policy (doda_amd.spconv.ops.level_policy): which SubM rulebook of a pyramid gets a tilebook,
which gets pair lists, and what a 16-channel bf16 layer's weight gradient then finds (spconv.functional._lists) — per level,
against the record of the parent commit (tests/data/pyramid_policy_parent.json, written by observe() below on the GPU at that
commit: the body uses nothing whose signature the policy's move changed).

Scenes (tests.util.surface_voxels, sorted x-major so the finest tilebooks stay below the overflow back-off; level sizes from
the oracle's k2 s2 builder on the CPU):
  20 000 rows [20000, 18699, 11853, 2301]  below TILE_MIN_ROWS (32 768) at both finest levels
  40 000 rows [40000, 35237, 16131, 2304]  above it at both, below PAIRS_MIN_ROWS (65 536)
  80 000 rows [80000, 62905, 18158, 2304]  level 1 above PAIRS_MIN_ROWS, level 2 between the two thresholds
  72 000 rows [72000, 71383, 66960, 42971] sparse: level 3 keeps 66 960 rows — lists instead of the weight-gradient-only
                                           tilebook that the coarse levels of the other scenes (and its level 4) take"""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import surface_voxels

pytestmark = pytest.mark.gpu

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "pyramid_policy_parent.json")
SCENES = [(11, 20000, [96, 96, 64]), (12, 40000, [96, 96, 64]), (13, 80000, [96, 96, 64]), (14, 72000, [256, 256, 256])]
CONFIGS = [(False, 0), (False, 2), (True, 2)]   # (with_pairs, with_tiles)
N_LEVELS, BATCH = 4, 2


def observe():
    """{"<rows>/<with_pairs>/<with_tiles>": per level [rows, SubM tilebook, SubM lists on the record, strided record without
    lists, _lists(SubM) gives lists, _lists(strided) gives lists]}"""
    from doda_amd import spconv
    from doda_amd._ext import ext
    from doda_amd.spconv import functional as Fsp
    assert ext is not None and torch.cuda.is_available()
    d = torch.device("cuda:0")
    weight = torch.zeros(27, 16, 16, device=d, requires_grad=True)
    weight8 = torch.zeros(8, 16, 16, device=d, requires_grad=True)
    state = spconv.ops._tile_state
    saved = dict(state)
    out = {}
    try:
        for seed, n, shape in SCENES:
            idx = surface_voxels(seed, n, BATCH, shape)
            idx = idx[np.lexsort((idx[:, 3], idx[:, 2], idx[:, 1], idx[:, 0]))]
            idx = torch.from_numpy(np.ascontiguousarray(idx)).to(d)
            for with_pairs, with_tiles in CONFIGS:
                state["skip"] = 0
                t = spconv.SparseConvTensor(None, idx, shape, BATCH)
                books = spconv.ops.build_pyramid(t, N_LEVELS, with_pairs=with_pairs, with_tiles=with_tiles)
                assert state["skip"] == 0, "the scene tripped the overflow back-off: %r" % (state["last"],)
                levels = []
                for lvl in range(1, N_LEVELS + 1):
                    subm, down = books["subm%d" % lvl], books.get("spconv%d" % lvl)
                    rows = int(subm.indices.shape[0])
                    row = [rows, bool(ext.has_tilebook(subm.tbl)), subm._wpairs is not None, down is None or down._wpairs is None]
                    feats = torch.zeros(rows, 16, dtype=torch.bfloat16, device=d)
                    row.append(Fsp._lists(subm, feats, weight) is not None)
                    row.append(down is not None and Fsp._lists(down, feats, weight8) is not None)
                    levels.append(row)
                out["%d/%d/%d" % (n, with_pairs, with_tiles)] = levels
        torch.cuda.synchronize()
    finally:
        state.update(saved)
    return out


def test_pyramid_policy_matches_the_parent_record(native_lib):
    with open(RECORD) as f:
        want = json.load(f)
    got = observe()
    assert sorted(got) == sorted(want) and len(got) == len(SCENES) * len(CONFIGS)
    for key in sorted(want):
        assert got[key] == want[key], key
    # the record itself covers what it is there for: both sides of both thresholds at the finest levels, a coarse level with
    # the weight-gradient-only tilebook, and a level beyond the second that is large enough for lists instead
    from doda_amd.spconv import ops as sops
    rows = {k: [lv[0] for lv in v] for k, v in want.items()}
    assert rows["20000/1/2"][0] < sops.TILE_MIN_ROWS <= rows["40000/1/2"][1] < sops.PAIRS_MIN_ROWS <= rows["80000/1/2"][0]
    assert want["40000/1/2"][2][1] and not want["40000/0/2"][2][1] and not want["40000/1/2"][2][2]
    big = want["72000/1/2"]
    assert big[2][0] >= sops.PAIRS_MIN_ROWS and big[2][2] and not big[2][1] and big[3][1]
    assert all(lv[3] and not lv[5] for v in want.values() for lv in v)   # strided rulebooks: no lists, none exported

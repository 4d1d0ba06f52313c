"""pointops, host side (no GPU): the companion C ABI include/doda_pointops.h and its argument errors, the `pointops2_cuda` surface,
and the restatements of tests/pointops_cases.py against float64 and against the reference's tie rule."""
import numpy as np
import pytest
import torch

from tests import pointops_cases as pc

INVALID, WORKSPACE = -1, -5


def _calls(lib):
    """name -> (function, default arguments): made-up non-null addresses and small positive sizes; nothing is dereferenced on the
    paths under test."""
    return {
        "transpose": (lib.doda_po_transpose, dict(idx=16, m=5, nsample=3, n=4, start=32, pos=48, ws=64, wsb=1 << 20, stream=None)),
        "grouping_fwd": (lib.doda_po_grouping_fwd, dict(inp=16, idx=32, out=48, n=4, m=5, nsample=3, c=2, stream=None)),
        "grouping_bwd": (lib.doda_po_grouping_bwd, dict(d_out=16, start=32, pos=48, d_inp=64, n=4, total=15, c=2, stream=None)),
        "interpolation_fwd": (lib.doda_po_interpolation_fwd, dict(inp=16, idx=32, w=48, out=64, n=4, m=5, k=3, c=2, stream=None)),
        "interpolation_bwd": (lib.doda_po_interpolation_bwd,
                              dict(d_out=16, w=32, start=48, pos=64, d_inp=80, n=4, m=5, k=3, c=2, stream=None)),
        "subtraction_fwd": (lib.doda_po_subtraction_fwd, dict(a=16, b=32, idx=48, out=64, n=4, m=5, nsample=3, c=2, stream=None)),
        "subtraction_bwd": (lib.doda_po_subtraction_bwd,
                            dict(d_out=16, start=32, pos=48, d_a=64, d_b=80, n=4, m=5, nsample=3, c=2, stream=None)),
        "aggregation_fwd": (lib.doda_po_aggregation_fwd,
                            dict(inp=16, position=32, w=48, idx=64, out=80, n=4, m=5, nsample=3, c=2, w_c=1, stream=None)),
        "aggregation_bwd": (lib.doda_po_aggregation_bwd,
                            dict(inp=16, position=32, w=48, idx=64, start=80, pos=96, d_out=112, d_inp=128, d_position=144, d_w=160,
                                 n=4, m=5, nsample=3, c=2, w_c=1, stream=None)),
        "furthestsampling": (lib.doda_po_furthestsampling,
                             dict(xyz=16, offset=32, new_offset=48, ws=64, idx=80, n=4, m=5, nbatch=2, dim=3, stream=None)),
    }


SIZES = ("m", "nsample", "n", "total", "k", "c", "w_c", "nbatch")
# the sizes that, set to zero, leave an entry point nothing to write (all pointers may then be null)
NOTHING = {"transpose": ("n",), "grouping_fwd": ("m", "nsample", "c"), "grouping_bwd": ("n", "c"), "interpolation_fwd": ("m", "c"),
           "interpolation_bwd": ("n", "c"), "subtraction_fwd": ("m", "nsample", "c"), "subtraction_bwd": ("c",),
           "aggregation_fwd": ("m", "c"), "aggregation_bwd": ("c",), "furthestsampling": ("m", "nbatch")}


def test_pointops_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses before anything is launched (no GPU here: a launch would fail differently); a count of
    zero is nothing to do."""
    for name, (fn, defaults) in _calls(native_lib).items():
        def call(**kw):
            d = dict(defaults)
            d.update(kw)
            return fn(*d.values())
        pointers = [k for k in defaults if k not in SIZES + ("dim", "wsb", "stream")]
        for size in (k for k in defaults if k in SIZES):
            assert call(**{size: -1}) == INVALID, (name, size)
        for p in pointers:
            assert call(**{p: None}) == INVALID, (name, p)
        for size in NOTHING[name]:
            assert call(**{size: 0}, **{p: None for p in pointers}) == 0, (name, size)
    fn, d = _calls(native_lib)["furthestsampling"]
    for dim in (0, 9, -3):
        assert fn(*dict(d, dim=dim).values()) == INVALID
    fn, d = _calls(native_lib)["transpose"]
    need = native_lib.doda_po_transpose_workspace_bytes(4)
    assert need >= 4 * 4 and native_lib.doda_po_transpose_workspace_bytes(0) == 0
    assert native_lib.doda_po_transpose_workspace_bytes(1 << 20) >= 4 << 20
    assert fn(*dict(d, wsb=need - 1).values()) == WORKSPACE and fn(*dict(d, ws=66).values()) == INVALID
    assert fn(*dict(d, m=1 << 20, nsample=1 << 12).values()) == INVALID           # positions are int32
    fn, d = _calls(native_lib)["aggregation_fwd"]
    assert fn(*dict(d, w_c=0).values()) == INVALID


def test_wrappers_refuse_cpu_tensors_and_other_dtypes(native_lib):
    from doda_amd import ops, pointops2
    x, idx = torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int32)
    off = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        pointops2.grouping(x, idx)
    with pytest.raises(RuntimeError, match="device"):
        pointops2.subtraction(x, x, idx)
    with pytest.raises(RuntimeError, match="device"):
        pointops2.aggregation(x, torch.zeros(4, 2, 3), torch.zeros(4, 2, 1), idx)
    with pytest.raises(RuntimeError, match="device"):
        ops.po_transpose(idx, 4)
    with pytest.raises(TypeError):
        pointops2.furthestsampling(x.double(), off, off)
    for name in ("furthestsampling", "FurthestSampling", "grouping", "Grouping", "queryandgroup", "subtraction", "Subtraction",
                 "aggregation", "Aggregation", "interpolation", "Interpolation", "interpolation2", "knnquery", "KNNQuery"):
        assert callable(getattr(pointops2, name)), name


def test_pointops2_cuda_exposes_the_reference_module_surface():
    """The eleven names of pointops_api.cpp, as real functions: none is the stub that raised NotImplementedError."""
    import inspect
    from doda_amd import pointops2_cuda
    from doda_amd.shims import pointops2_cuda as shim
    names = ("furthestsampling_cuda", "furthestsampling_dim_cuda", "knnquery_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
             "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda", "subtraction_backward_cuda",
             "aggregation_forward_cuda", "aggregation_backward_cuda")
    want_args = {"furthestsampling_cuda": 7, "furthestsampling_dim_cuda": 8, "knnquery_cuda": 8, "grouping_forward_cuda": 6,
                 "grouping_backward_cuda": 6, "interpolation_forward_cuda": 7, "interpolation_backward_cuda": 7,
                 "subtraction_forward_cuda": 7, "subtraction_backward_cuda": 7, "aggregation_forward_cuda": 9,
                 "aggregation_backward_cuda": 12}
    for name in names:
        fn = getattr(pointops2_cuda, name)
        assert getattr(shim, name) is fn
        assert len(inspect.signature(fn).parameters) == want_args[name], name       # a stub took (*args, **kwargs)
        assert "NotImplementedError" not in inspect.getsource(fn)
    assert not hasattr(pointops2_cuda, "_out_of_scope")
    x = torch.zeros(4, 3)
    idx = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):                                 # it reaches the checked wrapper
        pointops2_cuda.grouping_forward_cuda(4, 2, 3, x, idx, torch.zeros(4, 2, 3))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
def test_fps_restatement_on_the_grid_separates_the_two_tie_rules():
    """On the 6x6x6 integer grid exact ties decide almost every sample: the lowest-index rule and the reference's rule (for the block
    of 128 threads that it picks for 216 points) choose differently, so the device test on this cloud does exercise ties."""
    xyz = pc.grid_cloud()
    ends, new_ends = np.array([216], np.int32), np.array([60], np.int32)
    ours = pc.fps(xyz, ends, new_ends)
    theirs = pc.fps(xyz, ends, new_ends, pick=pc.block_tie_rule(128))
    assert ours[0] == theirs[0] == 0 and len(set(ours.tolist())) == 60 and len(set(theirs.tolist())) == 60
    assert (ours != theirs).sum() == 58                                                 # of 60
    assert (pc.fps(xyz, ends, new_ends, pick=pc.block_tie_rule(64)) != theirs).any()     # and their rule depends on the block


def test_fps_restatement_edges():
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((10, 3)).astype(np.float32)
    got = pc.fps(xyz, np.array([4, 4, 10], np.int32), np.array([6, 8, 9], np.int32))
    assert got[0] == 0 and sorted(got[:4].tolist()) == [0, 1, 2, 3] and (got[:6] < 4).all()      # more samples than points: repeats
    assert (got[6:8] == -1).all() and got[8] == 4
    # by hand on a line: 0, then the far end, then the middle's lowest index among the equidistant pair
    line = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)
    assert pc.fps(line, np.array([4], np.int32), np.array([4], np.int32)).tolist() == [0, 3, 1, 2]


def test_transpose_restatement():
    idx, n = pc.transpose_case(37, 16)
    start, pos = pc.transpose(idx, n)
    flat = idx.reshape(-1)
    assert np.diff(start)[:4].tolist() == [63, 64, 65, 0] and start[-1] == ((flat >= 0) & (flat < n)).sum() < flat.size
    for j in range(n):
        mine = pos[start[j]:start[j + 1]]
        assert (flat[mine] == j).all() and (np.diff(mine) > 0).all()


FORWARD_CASES = [pc.OpCase(c, ns, False) for c in (3, 67) for ns in (1, 16, 33)]


@pytest.mark.parametrize("case", FORWARD_CASES, ids=[c.name for c in FORWARD_CASES])
def test_forward_restatements_stay_inside_the_float64_bound(case):
    """A sum of k rounded products, added in order: |error| <= (k + 2) * 2^-24 * sum|terms| (first order: one rounding per product,
    k - 1 per partial sum, and for aggregation one more for the rounded inner sum, whose |a + b| <= |a| + |b|)."""
    k, i64 = case.nsample, np.float64
    rows = pc._rows(case.inp, case.idx[:, :]).astype(i64)                              # [m, k, c]
    w = case.w1.astype(i64)[:, :, None]
    worst = pc.worst_ratio(pc.interpolation_fwd(case.inp, case.idx, case.w1), (rows * w).sum(1), (np.abs(rows) * np.abs(w)).sum(1), k)
    assert worst <= 1.0
    for w_c in case.w_cs:
        wt = case.weight(w_c)
        ww = pc._wide(wt, case.c).astype(i64)
        position = case.position.astype(i64)
        worst = pc.worst_ratio(pc.aggregation_fwd(case.inp, case.position, wt, case.idx), ((rows + position) * ww).sum(1),
                               ((np.abs(rows) + np.abs(position)) * np.abs(ww)).sum(1), k)
        assert worst <= 1.0, w_c
    assert np.array_equal(pc.subtraction_fwd(case.a, case.inp, case.idx), (case.a.astype(i64)[:, None] - rows).astype(np.float32))
    assert np.array_equal(pc.grouping_fwd(case.inp, case.idx), rows.astype(np.float32))


@pytest.mark.parametrize("case", FORWARD_CASES[1::2], ids=[c.name for c in FORWARD_CASES[1::2]])
def test_backward_restatements_stay_inside_the_float64_bound(case):
    """The same form with the list length (or nsample, or the channels of a weight group) in place of k."""
    i64, n, c, k = np.float64, case.n, case.c, case.nsample
    g = case.g_full.reshape(-1, c)
    exact, length = pc.gather_sum64(g, case.idx, n)
    mag, _ = pc.gather_sum64(np.abs(g), case.idx, n)
    assert length[5] >= pc.HOT_ROWS
    assert pc.worst_ratio(pc.grouping_bwd(case.g_full, case.idx, n), exact, mag, length[:, None]) <= 1.0
    d_a, d_b = pc.subtraction_bwd(case.g_full, case.idx, n)
    assert pc.worst_ratio(d_b, -exact, mag, length[:, None]) <= 1.0
    assert pc.worst_ratio(d_a, case.g_full.astype(i64).sum(1), np.abs(case.g_full.astype(i64)).sum(1), k) <= 1.0
    term = (case.g_rows.astype(i64)[:, None, :] * case.w1.astype(i64)[:, :, None]).reshape(-1, c)
    exact, _ = pc.gather_sum64(term, case.idx, n)
    mag, _ = pc.gather_sum64(np.abs(term), case.idx, n)
    assert pc.worst_ratio(pc.interpolation_bwd(case.g_rows, case.idx, case.w1, n), exact, mag, length[:, None]) <= 1.0
    sq = pc.OpCase(c, k, True)
    for w_c in sq.w_cs:
        wt = sq.weight(w_c)
        d_inp, d_position, d_w = pc.aggregation_bwd(sq.inp, sq.position, wt, sq.idx, sq.g_rows)
        g64, ww = sq.g_rows.astype(i64)[:, None, :], pc._wide(wt, c).astype(i64)
        assert np.array_equal(d_position, (g64 * ww).astype(np.float32))
        exact, length = pc.gather_sum64((g64 * ww).reshape(-1, c), sq.idx, sq.n)
        mag, _ = pc.gather_sum64(np.abs(g64 * ww).reshape(-1, c), sq.idx, sq.n)
        assert pc.worst_ratio(d_inp, exact, mag, length[:, None]) <= 1.0, w_c
        inner = pc._rows(sq.inp, sq.idx).astype(i64) + sq.position.astype(i64)
        inner_mag = np.abs(pc._rows(sq.inp, sq.idx).astype(i64)) + np.abs(sq.position.astype(i64))
        exact_w, mag_w = np.zeros(wt.shape), np.zeros(wt.shape)
        for ch in range(c):
            exact_w[:, :, ch % w_c] += g64[:, 0, ch, None] * inner[:, :, ch]
            mag_w[:, :, ch % w_c] += np.abs(g64[:, 0, ch, None]) * inner_mag[:, :, ch]
        assert pc.worst_ratio(d_w, exact_w, mag_w, -(-c // w_c)) <= 1.0, w_c

"""The rest of PG_OP, host side (no GPU): the companion C ABI include/doda_pgops.h and its argument errors, the host BFS route
against the restatement of tests/pgops_cases.py (cluster order and order inside a cluster), the two restatements against each other
on symmetric graphs, the wrappers' shapes and dtypes, and the restatement of sec_mean against its float64 bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pgops_cases as pc

GRAPHS = pc.graph_cases()


def test_pgops_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses before anything is launched (no GPU here: a launch would fail differently); a count
    of zero is nothing to do.  Pointers are made-up addresses: nothing is dereferenced on these paths."""
    lib = native_lib
    INVALID, WORKSPACE = -1, -5

    def comp(**kw):
        d = dict(label=16, idxs=32, sl=48, n=5, na=7, root=64, size=80, stream=None)
        d.update(kw)
        return lib.doda_pg_components(*d.values())
    assert comp(n=0, label=None, idxs=None, sl=None, root=None, size=None) == 0
    assert comp(n=-1) == INVALID and comp(na=-1) == INVALID
    for name in ("label", "idxs", "sl", "root", "size"):
        assert comp(**{name: None}) == INVALID, name

    cnt = (C.c_int32 * 2)()
    p0, p1 = C.cast(cnt, C.POINTER(C.c_int32)), C.cast(C.byref(cnt, 4), C.POINTER(C.c_int32))
    off = (C.c_int32 * 4)()

    def bfs(**kw):
        d = dict(label=16, idxs=32, sl=48, n=5, na=7, thr=1, ci=64, co=C.cast(off, C.c_void_p), sum=p0, ncl=p1)
        d.update(kw)
        return lib.doda_pg_bfs_cluster_h(*d.values())
    assert bfs(n=0, na=0, label=None, idxs=None, sl=None, ci=None) == 0 and cnt[0] == 0 and cnt[1] == 0 and off[0] == 0
    assert bfs(n=-1) == INVALID and bfs(na=-1) == INVALID
    for name in ("label", "idxs", "sl", "ci", "co", "sum", "ncl"):
        assert bfs(**{name: None}) == INVALID, name

    def seg(fn, **kw):
        d = dict(a=16, offsets=32, b=48, rows=5, nseg=2, c=3, stream=None)
        d.update(kw)
        return getattr(lib, fn)(*d.values())
    for fn in ("doda_pg_sec_mean", "doda_pg_sec_min", "doda_pg_sec_max", "doda_pg_sec_mean_bp", "doda_pg_roipool_bp"):
        assert seg(fn, nseg=0, a=None, offsets=None, b=None) == 0 and seg(fn, c=0, a=None, offsets=None, b=None) == 0, fn
        assert seg(fn, rows=-1) == INVALID and seg(fn, nseg=-1) == INVALID and seg(fn, c=-1) == INVALID, fn
        for name in ("a", "offsets", "b"):
            assert seg(fn, **{name: None}) == INVALID, (fn, name)
    # nothing to write: no rows to receive a gradient
    assert seg("doda_pg_sec_mean_bp", rows=0, a=None) == 0 and seg("doda_pg_roipool_bp", rows=0, a=None) == 0

    def roi(**kw):
        d = dict(a=16, offsets=32, b=48, idx=64, rows=5, nseg=2, c=3, stream=None)
        d.update(kw)
        return lib.doda_pg_roipool_fp(*d.values())
    assert roi(nseg=0, a=None, offsets=None, b=None, idx=None) == 0 and roi(c=0) == 0
    assert roi(rows=-1) == INVALID and roi(nseg=-1) == INVALID and roi(c=-1) == INVALID
    for name in ("a", "offsets", "b", "idx"):
        assert roi(**{name: None}) == INVALID, name

    assert lib.doda_pg_get_iou_workspace_bytes(300, 300) == 0 and lib.doda_pg_get_iou_workspace_bytes(300, 8192) == 0
    assert lib.doda_pg_get_iou_workspace_bytes(3, 8193) == 3 * 8193 * 4 and lib.doda_pg_get_iou_workspace_bytes(0, 9000) == 0

    def iou(**kw):
        d = dict(idx=16, off=32, labels=48, pointnum=64, iou=80, npts=5, total=6, ninst=3, nprop=2, ws=None, wsb=0, stream=None)
        d.update(kw)
        return lib.doda_pg_get_iou(*d.values())
    assert iou(nprop=0, idx=None, off=None, labels=None, pointnum=None, iou=None) == 0 and iou(ninst=0) == 0
    for name in ("npts", "total", "ninst", "nprop"):
        assert iou(**{name: -1}) == INVALID, name
    for name in ("idx", "off", "labels", "pointnum", "iou"):
        assert iou(**{name: None}) == INVALID, name
    assert iou(ninst=8193) == INVALID                                    # a workspace is needed and none came
    assert iou(ninst=8193, ws=130, wsb=1 << 20) == INVALID               # misaligned
    assert iou(ninst=8193, ws=128, wsb=2 * 8193 * 4 - 1) == WORKSPACE


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _host(g, threshold):
    from doda_amd import ops
    return ops.pg_bfs_cluster_host(_t(g.label), _t(g.idxs), _t(g.start_len), threshold)


@pytest.mark.parametrize("g", GRAPHS, ids=[g.name for g in GRAPHS])
def test_host_bfs_route_is_the_sequential_rule(native_lib, g):
    """Cluster order and the order inside every cluster are the restatement's, at a threshold of 1, at one that keeps some
    components and drops others, and at one nothing survives."""
    sizes = sorted({len(c) for c in pc.bfs_clusters(g, 1)})
    for threshold in {1, sizes[len(sizes) // 2] if sizes else 1, (sizes[-1] if sizes else 0) + 1}:
        want_idxs, want_offsets = pc.pack_clusters(pc.bfs_clusters(g, threshold))
        idxs, offsets = _host(g, threshold)
        assert idxs.dtype == torch.int32 and offsets.dtype == torch.int32 and idxs.shape == (want_idxs.shape[0], 2)
        assert np.array_equal(idxs.numpy(), want_idxs) and np.array_equal(offsets.numpy(), want_offsets), threshold


@pytest.mark.parametrize("g", [g for g in GRAPHS if g.symmetric], ids=[g.name for g in GRAPHS if g.symmetric])
def test_restatements_agree_as_sets_on_symmetric_graphs(g):
    """BFS reachability and undirected components are the same clusters in the same order when every edge has its reverse."""
    root, size = pc.components(g)
    assert (root <= np.arange(g.n)).all() and size.sum() == g.n
    for threshold in (1, 3):
        bfs = pc.bfs_clusters(g, threshold)
        cc = pc.component_clusters(root, size, threshold)
        assert [sorted(c) for c in bfs] == cc


def test_asymmetric_graph_separates_the_two_rules():
    """The designed asymmetric graph is one on which reachability from the seed and undirected components differ, so the device
    test's comparison against the undirected restatement is not vacuous."""
    g = pc.asymmetric()
    root, size = pc.components(g)
    assert [sorted(c) for c in pc.bfs_clusters(g, 1)] != pc.component_clusters(root, size, 1)


def test_wrapper_shapes_and_dtypes_on_the_host_route(native_lib):
    from doda_amd import pg_op, pointgroup_ops
    g = pc.grid()
    label, idxs, sl = _t(g.label), _t(g.idxs), _t(g.start_len)
    ci, co = pointgroup_ops.bfs_cluster(label, idxs, sl, 64)
    assert ci.dtype == torch.int32 and co.dtype == torch.int32 and ci.shape == (g.n, 2) and co.shape == (26,)
    assert torch.equal(co, torch.arange(26, dtype=torch.int32) * 64)
    assert pointgroup_ops.BFSCluster.apply(label, idxs, sl, 64)[0].equal(ci)
    ci, co = pointgroup_ops.bfs_cluster(label, idxs, sl, 65)                       # nothing survives
    assert ci.shape == (0, 2) and ci.dtype == torch.int32 and co.tolist() == [0] and co.dtype == torch.int32
    a, b = label.new(), label.new()                                                 # the reference wrapper's call
    pg_op.bfs_cluster(label, idxs, sl, a, b, g.n, 64)
    assert a.shape == (g.n, 2) and b.shape == (26,) and a.dtype == torch.int32
    pg_op.bfs_cluster(label, idxs, sl, a, b, g.n, 65)
    assert a.shape == (0, 2) and b.tolist() == [0]
    e = torch.zeros(0, dtype=torch.int32)
    ci, co = pointgroup_ops.bfs_cluster(e, e, e.reshape(0, 2), 1)                   # no points at all
    assert ci.shape == (0, 2) and co.tolist() == [0]
    with pytest.raises(RuntimeError):
        pointgroup_ops.bfs_cluster(label.long(), idxs, sl, 1)
    for name in ("roipool", "get_iou", "sec_mean", "sec_min", "sec_max", "RoiPool", "GetIoU", "SecMean", "SecMin", "SecMax"):
        assert callable(getattr(pointgroup_ops, name))
    x, off = torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32)
    for fn in (pointgroup_ops.sec_mean, pointgroup_ops.sec_min, pointgroup_ops.sec_max, pointgroup_ops.roipool):
        with pytest.raises(RuntimeError, match="device"):                           # the seven other ops need device tensors
            fn(x, off)


@pytest.mark.parametrize("c", pc.SEG_CHANNELS)
def test_sequential_fp32_mean_stays_inside_the_float64_bound(c):
    """(len + 2) * 2^-24 * sum|x| / len holds for the index-order fp32 sum on every designed case, so it is a fair bound for a
    kernel that sums in another order."""
    for inp, offsets in (pc.seg_case(c), pc.seg_case_long(c), pc.seg_case_many(c, 500), pc.seg_case_corrupt(c)):
        worst = pc.check_sec_mean(pc.sec_mean(inp, offsets), inp, offsets)
        assert worst <= 1.0


def test_restatement_edge_values():
    inp, offsets = pc.seg_case(16)
    val, arg = pc.roipool(inp, offsets)
    k = {l: i for i, l in enumerate(pc.SEG_LENGTHS)}
    assert np.isneginf(val[k[0]]).all() and (arg[k[0]] == -1).all() and np.isposinf(pc.sec_min(inp, offsets)[k[0]]).all()
    assert (pc.sec_mean(inp, offsets)[k[0]] == 0).all()
    assert np.isneginf(val[k[64], 0]) and arg[k[64], 0] == -1                       # -inf never wins the strict compare
    assert not np.isnan(val).any() and arg[k[5000], 0] >= 0                         # nor does NaN
    assert val[k[65], 15] == 100.0 and arg[k[65], 15] == offsets[k[65]] + 9         # the first of three equal maxima
    idx, offset, labels, pointnum = pc.iou_case(37)
    iou = pc.get_iou(idx, offset, labels, pointnum)
    assert (iou[2] == 0).all() and iou[5, 36] > 0.99 and (iou[5, :36] == 0).all()

"""GPU tests of the pointops operators (include/doda_pointops.h, csrc/pointops.hip, doda_amd.ops / pointops2 / pointops2_cuda) on the
designed inputs of tests/pointops_cases.py against its numpy restatements.

Everything is bit equality: the kernels round every operation once and sum in the stated order, as the restatements do (which
tests/test_pointops_host.py holds to their float64 bounds).  Every operator runs twice and must give identical bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointops_cases as pc   # noqa: E402

pytestmark = pytest.mark.gpu
FPS = pc.fps_cases()
GROUP_CASES, SQUARE_CASES = pc.op_cases(False), pc.op_cases(True)
_REF = {}


def dev():
    return torch.device("cuda:0")


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ref(key, make):
    """A restatement's result, computed once and shared."""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def same(t, want):
    """bit equality with a numpy array (NaN-free inputs; -0 and +0 differ)"""
    got = t.detach().cpu().numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32))


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    return a


# ---- furthest point sampling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FPS, ids=[c.name for c in FPS])
def test_furthestsampling_equals_the_lowest_index_restatement(native_lib, case):
    from doda_amd import pointops2, pointops2_cuda
    want = ref(("fps", case.name), lambda: pc.fps(case.xyz, case.offset[1:], case.new_offset[1:]))
    xyz, offset, new_offset = d(case.xyz), d(case.offset), d(case.new_offset)
    idx = twice(lambda: pointops2.furthestsampling(xyz, offset, new_offset))
    assert idx.dtype == torch.int32 and idx.is_cuda and not idx.requires_grad and idx.grad_fn is None
    assert same(idx, want)
    got = idx.cpu().numpy()
    for b, (size, n_want) in enumerate(zip(case.sizes, case.wants)):      # every sample inside its own segment
        mine = got[case.new_offset[b]:case.new_offset[b + 1]]
        assert mine.size == n_want
        if size:
            assert (mine >= case.offset[b]).all() and (mine < case.offset[b + 1]).all()
            assert len(set(mine[:size].tolist())) == min(size, n_want) or case.name in ("duplicates",)
        else:
            assert (mine == -1).all()
    # the raw entry point fills a caller's buffer with the same bits, whatever the workspace held
    raw = torch.full((want.size,), -7, dtype=torch.int32, device=dev())
    tmp = torch.full((case.xyz.shape[0],), -3.0, device=dev())
    b, n_max, dim = len(case.sizes), max(case.sizes), case.xyz.shape[1]
    pointops2_cuda.furthestsampling_dim_cuda(b, n_max, dim, xyz, offset[1:], new_offset[1:], tmp, raw)
    assert torch.equal(raw, idx)
    if dim == 3:
        raw.fill_(-7)
        pointops2_cuda.furthestsampling_cuda(b, n_max, xyz, offset[1:], new_offset[1:], tmp, raw)
        assert torch.equal(raw, idx)
    assert pointops2.FurthestSampling.apply(xyz, offset, new_offset).equal(idx)


# ---- the index by destination ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,nsample", [(300, 1), (37, 16), (37, 33)])
def test_transpose_designed_lists(native_lib, m, nsample):
    from doda_amd import ops
    idx, n = pc.transpose_case(m, nsample)
    want_start, want_pos = pc.transpose(idx, n)
    assert np.diff(want_start)[:4].tolist() == [pc.WAVE_LIST - 1, pc.WAVE_LIST, pc.WAVE_LIST + 1, 0]
    start, pos = twice(lambda: tuple(t.clone() for t in _transposed_valid(ops, d(idx), n)))
    assert same(start, want_start) and same(pos, want_pos)


def _transposed_valid(ops, idx, n):
    start, pos = ops.po_transpose(idx, n)
    return start, pos[:int(start[-1])]


def test_transpose_one_long_list(native_lib):
    from doda_amd import ops
    idx = np.zeros((3000, 1), np.int32)
    start, pos = twice(lambda: _transposed_valid(ops, d(idx), 1))
    assert start.tolist() == [0, 3000] and torch.equal(pos.cpu(), torch.arange(3000, dtype=torch.int32))


# ---- the four pairs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GROUP_CASES, ids=[c.name for c in GROUP_CASES])
def test_grouping_and_interpolation_pairs(native_lib, case):
    """m != n; destination 5 is hit by 3000 rows; invalid indices present."""
    from doda_amd import ops, pointops2, pointops2_cuda
    assert case.m != case.n
    inp, idx, w1, g_full, g_rows = d(case.inp), d(case.idx), d(case.w1), d(case.g_full), d(case.g_rows)
    want = ref(("grouping", case.name), lambda: (pc.grouping_fwd(case.inp, case.idx), pc.grouping_bwd(case.g_full, case.idx, case.n),
                                                  pc.interpolation_fwd(case.inp, case.idx, case.w1),
                                                  pc.interpolation_bwd(case.g_rows, case.idx, case.w1, case.n)))
    x = inp.clone().requires_grad_(True)

    def run_grouping():
        x.grad = None
        out = pointops2.grouping(x, idx)
        out.backward(g_full)
        return out.detach(), x.grad.clone()
    out, grad = twice(run_grouping)
    assert same(out, want[0]) and same(grad, want[1])
    assert pointops2.Grouping.apply(x, idx).equal(out)

    def run_interpolation():
        out = torch.empty(case.m, case.c, device=dev())
        grad = torch.empty(case.n, case.c, device=dev())
        ops.po_interpolation_fwd(inp, idx, w1, out)
        start, pos = ops.po_transpose(idx, case.n)
        ops.po_interpolation_bwd(g_rows, w1, start, pos, grad)
        return out, grad
    out, grad = twice(run_interpolation)
    assert same(out, want[2]) and same(grad, want[3])

    # the raw module fills caller-allocated buffers (full of something else) with the same bits
    o = torch.full((case.m, case.nsample, case.c), 9.0, device=dev())
    gi = torch.full((case.n, case.c), 9.0, device=dev())
    pointops2_cuda.grouping_forward_cuda(case.m, case.nsample, case.c, inp, idx, o)
    pointops2_cuda.grouping_backward_cuda(case.m, case.nsample, case.c, g_full, idx, gi)
    assert same(o, want[0]) and same(gi, want[1])
    o, gi = torch.full((case.m, case.c), 9.0, device=dev()), gi.fill_(9.0)
    pointops2_cuda.interpolation_forward_cuda(case.m, case.c, case.nsample, inp, idx, w1, o)
    pointops2_cuda.interpolation_backward_cuda(case.m, case.c, case.nsample, g_rows, idx, w1, gi)
    assert same(o, want[2]) and same(gi, want[3])


@pytest.mark.parametrize("case", SQUARE_CASES, ids=[c.name for c in SQUARE_CASES])
def test_subtraction_pair(native_lib, case):
    from doda_amd import pointops2, pointops2_cuda
    a, b, idx, g = d(case.a), d(case.inp), d(case.idx), d(case.g_full)
    want = ref(("subtraction", case.name), lambda: (pc.subtraction_fwd(case.a, case.inp, case.idx),)
               + pc.subtraction_bwd(case.g_full, case.idx, case.n))
    xa, xb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def run():
        xa.grad = xb.grad = None
        out = pointops2.subtraction(xa, xb, idx)
        out.backward(g)
        return out.detach(), xa.grad.clone(), xb.grad.clone()
    out, ga, gb = twice(run)
    assert same(out, want[0]) and same(ga, want[1]) and same(gb, want[2])
    o = torch.full_like(out, 9.0)
    r1, r2 = torch.full_like(ga, 9.0), torch.full_like(gb, 9.0)
    pointops2_cuda.subtraction_forward_cuda(case.m, case.nsample, case.c, a, b, idx, o)
    pointops2_cuda.subtraction_backward_cuda(case.m, case.nsample, case.c, idx, g, r1, r2)
    assert same(o, want[0]) and same(r1, want[1]) and same(r2, want[2])


@pytest.mark.parametrize("case", SQUARE_CASES, ids=[c.name for c in SQUARE_CASES])
def test_aggregation_pair(native_lib, case):
    """w_c in {1, 4, 5, c}: one of them does not divide c, and may exceed it."""
    from doda_amd import pointops2, pointops2_cuda
    assert any(case.c % w_c for w_c in case.w_cs)
    inp, position, idx, g = d(case.inp), d(case.position), d(case.idx), d(case.g_rows)
    for w_c in case.w_cs:
        wt = case.weight(w_c)
        want = ref(("aggregation", case.name, w_c), lambda: (pc.aggregation_fwd(case.inp, case.position, wt, case.idx),)
                   + pc.aggregation_bwd(case.inp, case.position, wt, case.idx, case.g_rows))
        w = d(wt)
        x, p, ww = (t.clone().requires_grad_(True) for t in (inp, position, w))

        def run():
            x.grad = p.grad = ww.grad = None
            out = pointops2.aggregation(x, p, ww, idx)
            out.backward(g)
            return out.detach(), x.grad.clone(), p.grad.clone(), ww.grad.clone()
        got = twice(run)
        for t, wanted, what in zip(got, want, ("out", "d_input", "d_position", "d_weight")):
            assert same(t, wanted), (w_c, what)
        if w_c == case.w_cs[-1]:
            raw = [torch.full_like(t, 9.0) for t in got]
            pointops2_cuda.aggregation_forward_cuda(case.m, case.nsample, case.c, w_c, inp, position, w, idx, raw[0])
            pointops2_cuda.aggregation_backward_cuda(case.m, case.nsample, case.c, w_c, inp, position, w, idx, g, *raw[1:])
            for t, wanted in zip(raw, want):
                assert same(t, wanted), w_c


# ---- autograd wiring -----------------------------------------------------------------------------------------------------------------
def test_autograd_chain_shares_one_transposed_index(native_lib):
    """aggregation(x, subtraction(x, y, idx), w, idx) -> interpolation2 -> backward(gradient=t), against the restatements chained by
    hand; the index by destination of the shared idx is built exactly once (the interpolation's own kNN idx needs a second one)."""
    from doda_amd import ops, pointops2
    rng = np.random.default_rng(3)
    n, ns, c, w_c, n_new = 500, 8, 12, 4, 650
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    new_xyz = rng.standard_normal((n_new, 3)).astype(np.float32)
    offset, new_offset = np.array([0, 200, n], np.int32), np.array([0, 300, n_new], np.int32)
    x_np, y_np = pc._mixed(rng, n, c), pc._mixed(rng, n, c)
    w_np, t_np = pc._mixed(rng, n, ns, w_c), pc._mixed(rng, n_new, c)
    d_xyz, d_new, d_off, d_noff = d(xyz), d(new_xyz), d(offset), d(new_offset)
    idx, _ = pointops2.knnquery(ns, d_xyz, None, d_off, d_off)
    idx_np = idx.cpu().numpy()
    x, y, w = (d(a).requires_grad_(True) for a in (x_np, y_np, w_np))
    before = ops.po_transpose_calls
    rel = pointops2.subtraction(x, y, idx)
    agg = pointops2.aggregation(x, rel, w, idx)
    out = pointops2.interpolation2(d_xyz, d_new, agg, d_off, d_noff, 3)
    assert ops.po_transpose_calls == before                                         # lazily: nothing is built in a forward
    out.backward(gradient=d(t_np))
    assert ops.po_transpose_calls == before + 2
    kidx, kw = pointops2._interpolation_weights(d_xyz, d_new, d_off, d_noff, 3)
    kidx_np, kw_np = kidx.cpu().numpy(), kw.cpu().numpy()

    rel_np = pc.subtraction_fwd(x_np, y_np, idx_np)
    agg_np = pc.aggregation_fwd(x_np, rel_np, w_np, idx_np)
    assert same(rel, rel_np) and same(agg, agg_np) and same(out, pc.interpolation_fwd(agg_np, kidx_np, kw_np))
    g_agg = pc.interpolation_bwd(t_np, kidx_np, kw_np, n)
    g_x_agg, g_rel, g_w = pc.aggregation_bwd(x_np, rel_np, w_np, idx_np, g_agg)
    g_x_sub, g_y = pc.subtraction_bwd(g_rel, idx_np, n)
    assert same(w.grad, g_w) and same(y.grad, g_y)
    # x receives two gradients; autograd adds them in one fp32 addition, in either order the same bits
    assert same(x.grad, g_x_agg + g_x_sub)

    # None where the reference has None, and the first interpolation form gives the same values
    out2 = pointops2.interpolation2(d_xyz, d_new, agg.detach().requires_grad_(True), d_off, d_noff, 3)
    assert [g is None for g in out2.grad_fn.apply(d(t_np))] == [True, True, False, True, True, True]
    before += 1                                                                     # (its own kNN idx is a new tensor)
    rel2 = pointops2.subtraction(x, y, idx)
    assert [g is None for g in rel2.grad_fn.apply(torch.ones_like(rel2))] == [False, False, True]
    grp, agg2 = pointops2.grouping(x, idx), pointops2.aggregation(x, rel2, w, idx)     # (alive while their nodes are called)
    assert [g is None for g in grp.grad_fn.apply(torch.ones(n, ns, c, device=dev()))] == [False, True]
    assert [g is None for g in agg2.grad_fn.apply(torch.ones(n, c, device=dev()))] == [False, False, False, True]
    assert ops.po_transpose_calls == before + 2                                     # all of them reused the remembered index
    assert same(pointops2.interpolation(d_xyz, d_new, agg.detach(), d_off, d_noff, 3), pc.interpolation_fwd(agg_np, kidx_np, kw_np))
    idx2 = idx.clone()
    idx2[0, 0] = 3                                                                  # a written-to idx is transposed afresh
    pointops2.grouping(x, idx2).backward(torch.ones(n, ns, c, device=dev()))
    assert ops.po_transpose_calls == before + 3


def test_queryandgroup_routes_gradients_through_grouping(native_lib):
    from doda_amd import pointops2
    rng = np.random.default_rng(8)
    n, m, ns, c = 300, 120, 5, 7
    xyz_np, new_np, feat_np = (rng.standard_normal(s).astype(np.float32) for s in ((n, 3), (m, 3), (n, c)))
    offset, new_offset = d(np.array([0, n], np.int32)), d(np.array([0, m], np.int32))
    xyz, new_xyz, feat = (d(a).requires_grad_(True) for a in (xyz_np, new_np, feat_np))
    out = pointops2.queryandgroup(ns, xyz, new_xyz, feat, None, offset, new_offset)
    idx, _ = pointops2.knnquery(ns, xyz.detach(), new_xyz.detach(), offset, new_offset)
    idx_np = idx.cpu().numpy()
    assert out.shape == (m, ns, 3 + c)
    assert same(out, np.concatenate((pc.grouping_fwd(xyz_np, idx_np) - new_np[:, None], pc.grouping_fwd(feat_np, idx_np)), -1))
    g = rng.standard_normal((m, ns, 3 + c)).astype(np.float32)
    out.backward(d(g))
    assert same(xyz.grad, pc.grouping_bwd(np.ascontiguousarray(g[..., :3]), idx_np, n))
    assert same(feat.grad, pc.grouping_bwd(np.ascontiguousarray(g[..., 3:]), idx_np, n))
    assert torch.allclose(new_xyz.grad, -d(g[..., :3]).sum(1))
    only = pointops2.queryandgroup(ns, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=False)
    assert same(only, pc.grouping_fwd(feat_np, idx_np))


def test_row_movers_give_the_same_bits_on_unaligned_arrays(native_lib):
    """The row movers (grouping and subtraction forward) and the per-destination sums take four channels per thread where c is a
    multiple of 4 and every array is 16-byte aligned, one otherwise: arrays that start 4 bytes past an aligned address (c = 32)
    take the other route and give the same bits."""
    from doda_amd import ops
    case = next(c for c in SQUARE_CASES if c.name == "c32_ns16")
    want_g = ref(("grouping_sq", case.name), lambda: pc.grouping_fwd(case.inp, case.idx))
    want_s = ref(("subtraction", case.name), lambda: (pc.subtraction_fwd(case.a, case.inp, case.idx),)
                 + pc.subtraction_bwd(case.g_full, case.idx, case.n))[0]

    def shifted(a):
        buf = torch.empty(a.size + 1, device=dev())
        view = buf[1:].view(a.shape)
        view.copy_(d(a))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    idx = d(case.idx)
    for inp, a, out in ((shifted(case.inp), shifted(case.a), shifted(want_s)), (d(case.inp), d(case.a), torch.empty_like(d(want_s)))):
        ops.po_grouping_fwd(inp, idx, out)
        assert same(out, want_g)
        ops.po_subtraction_fwd(a, inp, idx, out)
        assert same(out, want_s)
    # the per-destination sums likewise: four channels per thread, or one where the gradient is not 16-byte aligned
    want_b = ref(("grouping_bwd_sq", case.name), lambda: pc.grouping_bwd(case.g_full, case.idx, case.n))
    start, pos = ops.po_transpose(idx, case.n)
    for g_full, grad in ((shifted(case.g_full), shifted(want_b)), (d(case.g_full), torch.empty_like(d(want_b)))):
        ops.po_grouping_bwd(g_full.view(-1, case.c), start, pos, grad)
        assert same(grad, want_b)

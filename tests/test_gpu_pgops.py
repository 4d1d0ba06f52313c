"""GPU tests of the rest of PG_OP (include/doda_pgops.h, csrc/pgops.hip, doda_amd.ops / pg_op / pointgroup_ops) on the designed
inputs of tests/pgops_cases.py against its numpy restatements.

Everything is bit equality except sec_mean, whose kernel sums a segment's rounded quotients in another order than the index-order
restatement: it is held to |out - mean64| <= (len + 2) * 2^-24 * sum|x| / len per channel, the first-order bound of len rounded
quotients plus len - 1 rounded additions, which the restatement itself meets on every case (tests/test_pgops_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgops_cases as pc   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = pc.graph_cases()
_REF = {}


def dev():
    return torch.device("cuda:0")


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def graph_ref(g):
    """(root, size) of the undirected restatement, made once per graph."""
    if g.name not in _REF:
        _REF[g.name] = pc.components(g)
    return _REF[g.name]


def seg_ref(key, make):
    if key not in _REF:
        inp, offsets = make()
        val, arg = pc.roipool(inp, offsets)
        _REF[key] = (inp, offsets, pc.sec_min(inp, offsets), val, (val, arg))       # (sec_max is roipool's value)
    return _REF[key]


# ---- components and clustering --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GRAPHS, ids=[g.name for g in GRAPHS])
def test_components_and_clusters_equal_the_undirected_restatement(native_lib, g):
    """root and size bit for bit (the asymmetric and corrupt-range graphs included: the device route is the UNDIRECTED components),
    twice with identical bits; clusters at a threshold of 1, at a component's size (kept) and one above the largest (nothing
    survives), and at one above a middle size (that component dropped)."""
    from doda_amd import ops, pointgroup_ops
    want_root, want_size = graph_ref(g)
    label, idxs, sl = d(g.label), d(g.idxs), d(g.start_len)
    root, size = ops.pg_components(label, idxs, sl)
    assert root.dtype == torch.int32 and size.dtype == torch.int32
    assert torch.equal(root.cpu(), torch.from_numpy(want_root)) and torch.equal(size.cpu(), torch.from_numpy(want_size))
    root2, size2 = ops.pg_components(label, idxs, sl)
    assert torch.equal(root, root2) and torch.equal(size, size2)
    sizes = sorted(set(want_size[want_size > 0].tolist()))
    mid = sizes[len(sizes) // 2] if sizes else 1
    for threshold in sorted({1, mid, mid + 1, (sizes[-1] if sizes else 0) + 1}):
        want_idxs, want_offsets = pc.pack_clusters(pc.component_clusters(want_root, want_size, threshold))
        ci, co = pointgroup_ops.bfs_cluster(label, idxs, sl, threshold)
        assert ci.is_cuda and ci.dtype == torch.int32 and co.dtype == torch.int32 and ci.shape == (want_idxs.shape[0], 2)
        assert torch.equal(ci.cpu(), torch.from_numpy(want_idxs)) and torch.equal(co.cpu(), torch.from_numpy(want_offsets)), threshold
        if sizes:   # the thresholds do what they are there for: mid keeps the components of that size, mid + 1 drops them
            assert (threshold > sizes[-1]) == (want_idxs.shape[0] == 0) and (threshold <= mid) == (mid in want_size[want_idxs[:, 1]])
    ci2, co2 = pointgroup_ops.bfs_cluster(label, idxs, sl, 1)
    ci1, co1 = pointgroup_ops.BFSCluster.apply(label, idxs, sl, 1)
    assert torch.equal(ci1, ci2) and torch.equal(co1, co2)


def test_ballquery_then_cluster_equals_the_host_route(native_lib):
    """Two synthetic scenes: ball query on the device, then bfs_cluster with device tensors against the host route (the reference's
    sequential BFS) on the same tensors copied to the CPU — the same clusters as sets, in the same order.  The threshold keeps at
    least one cluster and drops at least one on the host route, so the comparison cannot pass on an empty result."""
    from doda_amd import pointgroup_ops, scene
    batch = scene.make_batch(2, 6000, 77)
    xyz = batch["locs_float"].to(dev()).contiguous()
    offsets = batch["offsets"].to(dev())
    n = xyz.shape[0]
    bidx = torch.repeat_interleave(torch.arange(2, device=dev()), (offsets[1:] - offsets[:-1]).long()).to(torch.int32)
    label = batch["labels"].to(torch.int32).to(dev())
    idx, start_len = pointgroup_ops.ballquery_batch_p(xyz, bidx, offsets, 0.04, 50)
    idx = idx.contiguous()
    assert start_len.shape == (n, 2) and idx.numel() > n
    every = pc.unpack_clusters(*(t.numpy() for t in pointgroup_ops.bfs_cluster(label.cpu(), idx.cpu(), start_len.cpu(), 1)))
    sizes = sorted(len(c) for c in every)
    threshold = sizes[len(sizes) // 2] + 1 if sizes[len(sizes) // 2] < sizes[-1] else sizes[-1]
    host = pc.unpack_clusters(*(t.numpy() for t in pointgroup_ops.bfs_cluster(label.cpu(), idx.cpu(), start_len.cpu(), threshold)))
    assert 1 <= len(host) < len(every), (len(host), len(every), threshold)
    ci, co = pointgroup_ops.bfs_cluster(label, idx, start_len, threshold)
    mine = pc.unpack_clusters(ci.cpu().numpy(), co.cpu().numpy())
    assert len(mine) == len(host) and all(m == sorted(h) for m, h in zip(mine, host))


# ---- segment pools -------------------------------------------------------------------------------------------------------------
def _seg_cases():
    cases = [("designed%d" % c, (lambda c=c: pc.seg_case(c))) for c in pc.SEG_CHANNELS]
    cases += [("long%d" % c, (lambda c=c: pc.seg_case_long(c))) for c in pc.SEG_CHANNELS]
    cases.append(("many", pc.seg_case_many))
    cases.append(("corrupt", pc.seg_case_corrupt))
    return cases


@pytest.mark.parametrize("name,make", _seg_cases(), ids=[n for n, _ in _seg_cases()])
def test_segment_pools_forward(native_lib, name, make):
    """sec_min / sec_max / roipool (values and arg-max) bit for bit; sec_mean inside its bound; twice the same bits.  The long
    cases run the kernels' 1024-thread workgroups, the others the 256-thread ones."""
    from doda_amd import _lib, ops, pointgroup_ops
    inp, offsets, want_min, want_max, (want_val, want_arg) = seg_ref(name, make)
    assert _lib.PG_LONG_SEGMENT == pc.LONG_SEGMENT
    assert name.startswith("long") == (inp.shape[0] >= pc.LONG_SEGMENT * (len(offsets) - 1))
    x, off = d(inp), d(offsets)
    ns, c = want_min.shape
    with np.errstate(all="ignore"):
        assert torch.equal(pointgroup_ops.sec_min(x, off).cpu(), torch.from_numpy(want_min))
        assert torch.equal(pointgroup_ops.sec_max(x, off).cpu(), torch.from_numpy(want_max))
        out = torch.full((ns, c), 7.0, device=dev())
        arg = torch.full((ns, c), 7, dtype=torch.int32, device=dev())
        ops.roipool_fp(x, off, out, arg, ns, c)
        assert torch.equal(out.cpu(), torch.from_numpy(want_val)) and torch.equal(arg.cpu(), torch.from_numpy(want_arg))
        assert torch.equal(pointgroup_ops.roipool(x, off), out) and torch.equal(pointgroup_ops.SecMax.apply(x, off), out)
        mean = pointgroup_ops.sec_mean(x, off)
        worst = pc.check_sec_mean(mean.cpu().numpy(), inp, offsets)
        print("sec_mean %s: worst error / bound = %.3f" % (name, worst))
        assert torch.equal(mean.view(torch.int32), pointgroup_ops.sec_mean(x, off).view(torch.int32))


@pytest.mark.parametrize("kind", ("designed", "long"))
@pytest.mark.parametrize("c", pc.SEG_CHANNELS)
def test_segment_pools_backward_through_autograd(native_lib, c, kind):
    """roipool and sec_mean gradients equal to the restatement; rows outside every segment stay zero; sec_min / sec_max and the
    offsets get none."""
    from doda_amd import pointgroup_ops
    make = pc.seg_case if kind == "designed" else pc.seg_case_long
    inp, offsets, _, _, (_, want_arg) = seg_ref("%s%d" % (kind, c), lambda: make(c))
    rng = np.random.default_rng(c)
    d_out = rng.standard_normal((len(offsets) - 1, c)).astype(np.float32)
    off = d(offsets)
    for fn, want in ((pointgroup_ops.roipool, pc.roipool_bp(d_out, want_arg, inp.shape[0])),
                     (pointgroup_ops.sec_mean, pc.sec_mean_bp(d_out, offsets, inp.shape[0]))):
        x = d(inp).requires_grad_(True)
        fn(x, off).backward(d(d_out))
        assert torch.equal(x.grad.cpu(), torch.from_numpy(want)), fn.__name__
        assert (x.grad[:pc.SEG_LEAD] == 0).all() and (x.grad[-pc.SEG_TAIL:] == 0).all()
    x = d(inp).requires_grad_(True)
    assert not pointgroup_ops.sec_min(x, off).requires_grad and not pointgroup_ops.sec_max(x, off).requires_grad


def test_backward_kernels_leave_other_rows_alone(native_lib):
    """roipool_bp with an arg-max of -1 (or any row outside the array) writes nothing and ADDS elsewhere; sec_mean_bp leaves rows
    outside every segment as they were; 33000 one-row segments (past a 32768-block grid) all get their gradient."""
    from doda_amd import ops, pg_op
    c = 5
    d_feats = torch.full((6, c), 2.0, device=dev())
    maxidx = torch.tensor([[-1] * c, [3, 3, 6, -7, 0], [4] * c], dtype=torch.int32, device=dev())
    d_out = torch.arange(3 * c, dtype=torch.float32, device=dev()).reshape(3, c) + 1
    off = torch.tensor([0, 0, 4, 6], dtype=torch.int32, device=dev())
    pg_op.roipool_bp(d_feats, off, maxidx, d_out, 3, c)
    want = np.full((6, c), 2.0, dtype=np.float32) + pc.roipool_bp(d_out.cpu().numpy(), maxidx.cpu().numpy(), 6)
    assert torch.equal(d_feats.cpu(), torch.from_numpy(want)) and want[3, 0] == 8.0 and want.sum() == 60 + 6 + 7 + 10 + 11 + 12 + 13 + 14 + 15
    d_inp = torch.full((8, c), -3.0, device=dev())
    off = torch.tensor([1, 3, 3, 6], dtype=torch.int32, device=dev())
    pg_op.sec_mean_bp(d_inp, off, d_out, 3, c)
    want = np.full((8, c), -3.0, dtype=np.float32)
    want[1:3], want[3:6] = d_out[0].cpu().numpy() / np.float32(2), d_out[2].cpu().numpy() / np.float32(3)
    assert torch.equal(d_inp.cpu(), torch.from_numpy(want))
    inp, offsets = pc.seg_case_many()
    g = d(inp)
    d_inp = torch.zeros_like(g)
    ops.sec_mean_bp(d_inp, d(offsets), g, inp.shape[0], inp.shape[1])
    assert torch.equal(d_inp, g)


# ---- proposal IoU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_instance", pc.IOU_INSTANCES + (8193,))
def test_get_iou_equals_the_formula(native_lib, n_instance):
    """Bit for bit against float32(float64(float32(inter)) / (float64(float32(union)) + 1e-5)); 8193 instances is one past the
    histogram's LDS budget (the workspace route)."""
    from doda_amd import _lib, pointgroup_ops
    assert _lib.PG_IOU_LDS_INSTANCES == 8192
    idx, offset, labels, pointnum = pc.iou_case(n_instance)
    want = pc.get_iou(idx, offset, labels, pointnum)
    args = (d(idx), d(offset), d(labels), d(pointnum))
    iou = pointgroup_ops.get_iou(*args)
    assert iou.dtype == torch.float32 and torch.equal(iou.cpu(), torch.from_numpy(want))
    assert torch.equal(iou, pointgroup_ops.GetIoU.apply(*args))
    assert (want[2] == 0).all() and want[5, n_instance - 1] > 0.99 and np.count_nonzero(want[5]) == 1


# ---- the drop-in module ------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "doda_amd", "shims"))
import torch
import PG_OP
dev = torch.device("cuda:0")
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
label, idxs, start_len = i32([0, 0, 1, 0]), i32([1, 0, 3, 3, 1]), i32([[0, 1], [1, 2], [3, 0], [3, 2]])
for lab, ix, sl in ((label, idxs, start_len), (label.cpu(), idxs.cpu(), start_len.cpu())):
    ci, co = lab.new(), lab.new()
    PG_OP.bfs_cluster(lab, ix, sl, ci, co, 4, 2)
    assert ci.tolist() == [[0, 0], [0, 1], [0, 3]] and co.tolist() == [0, 3] and ci.device == lab.device, (ci, co)
feats = torch.tensor([[1., 5.], [3., 5.], [2., -1.], [0., 7.]], device=dev)
off = i32([0, 2, 2, 4])
out, arg = torch.cuda.FloatTensor(3, 2).zero_(), torch.cuda.IntTensor(3, 2).zero_()
PG_OP.roipool_fp(feats, off, out, arg, 3, 2)
inf = float("inf")
assert out.tolist() == [[3., 5.], [-inf, -inf], [2., 7.]] and arg.tolist() == [[1, 0], [-1, -1], [2, 3]], (out, arg)
d_feats = torch.cuda.FloatTensor(4, 2).zero_()
PG_OP.roipool_bp(d_feats, off, arg, torch.ones(3, 2, device=dev), 3, 2)
assert d_feats.tolist() == [[0., 1.], [1., 0.], [1., 0.], [0., 1.]], d_feats
PG_OP.sec_mean(feats, off, out, 3, 2)
assert out.tolist() == [[2., 5.], [0., 0.], [1., 3.]], out
PG_OP.sec_min(feats, off, out, 3, 2)
assert out.tolist() == [[1., 5.], [inf, inf], [0., -1.]], out
PG_OP.sec_max(feats, off, out, 3, 2)
assert out.tolist() == [[3., 5.], [-inf, -inf], [2., 7.]], out
d_inp = torch.cuda.FloatTensor(4, 2).zero_()
PG_OP.sec_mean_bp(d_inp, off, torch.tensor([[3., 6.], [1., 1.], [2., 4.]], device=dev), 3, 2)
assert d_inp.tolist() == [[1.5, 3.], [1.5, 3.], [1., 2.], [1., 2.]], d_inp
inst = torch.tensor([0, 0, 1, -100], device=dev)
iou = torch.cuda.FloatTensor(2, 2).zero_()
PG_OP.get_iou(i32([0, 1, 2, 3]), i32([0, 3, 4]), inst, i32([2, 1]), iou, 2, 2)
want = [[2.0 / (3.0 + 1e-5), 1.0 / (3.0 + 1e-5)], [0.0, 0.0]]
assert iou.tolist() == torch.tensor(want, dtype=torch.float64).float().tolist(), iou
print("PG_OP complete")
"""


def test_shim_module_runs_all_eight_functions(native_lib):
    """`import PG_OP` from doda_amd/shims in a fresh process, DODA_NO_EXT=1 (through doda_amd.ops alone): each of the eight
    functions with the reference's positional arguments on a tiny case."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DODA_NO_EXT="1"))
    assert r.returncode == 0 and "PG_OP complete" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]

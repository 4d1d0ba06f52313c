"""GPU tests of the rest of the spconv surface (include/doda_spconv.h, csrc/rulebook.hip, csrc/maxpool.hip, csrc/spconv_dense.hip,
doda_amd.spconv): the transposed rulebook bit for bit against the serial restatement, SparseConvTranspose3d against fp64
F.conv_transpose3d autograd, bf16 max pooling bit for bit on designed ties, dense() / from_dense() against the torch expressions,
and a small network end to end against the same graph of dense torch ops.  Restatements and inputs: tests/spconv_cases.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spconv_cases as cases

pytestmark = pytest.mark.gpu

BF16_TOL = 2.0 ** -7          # the project's bf16 layer tolerance
SETS = cases.voxel_sets()


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


@functools.lru_cache(maxsize=None)
def restated_rulebook(voxels, geometry):
    idx, shape, _ = SETS[voxels]
    return cases.deconv_rulebook(idx, shape, *cases.GEOMETRIES[geometry])


# ------------------------------------------------------------------------------------------------ 1. the transposed rulebook
@pytest.mark.parametrize("geometry", list(cases.GEOMETRIES))
@pytest.mark.parametrize("voxels", list(SETS))
def test_transposed_rulebook_is_the_serial_scan_bit_for_bit(native_lib, voxels, geometry):
    from doda_amd import ops
    idx, shape, batch = SETS[voxels]
    ref = restated_rulebook(voxels, geometry)
    di = torch.from_numpy(idx).to(dev())
    builds = [ops.rulebook_deconv(di, shape, batch, *cases.GEOMETRIES[geometry]) for _ in range(2)]
    for got in builds:
        assert got[3] == ref[3]
        for g, r in zip(got[:3], ref[:3]):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), r)
    if geometry == "k3s1p1 grows":
        assert builds[0][0].shape[0] > idx.shape[0]
    if voxels == "eight corners" and geometry == "k3s1p1 grows":
        assert (ref[2] < 0).sum(0).min() > 0          # every corner drops positions, low side and high side
    if voxels == "2000 voxels":
        assert idx.shape[0] > 256 and idx.shape[0] % 256 != 0


# ------------------------------------------------------------------------------------------------ 2. the layer
def _layer_reference(x, w, b, idx, shape, batch, out_idx, out_shape, s, p, gy):
    """fp64 conv_transpose3d autograd sampled at the layer's indices; (y, dx, dW, dbias)"""
    x, w, b = (v.clone().requires_grad_(True) for v in (x, w, b))
    y = cases.sample(cases.conv_transpose_dense(cases.scatter_dense(x, idx, shape, batch), w, s, p, 1, 0, out_shape), out_idx) + b
    (y * gy).sum().backward()
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("geometry", [(2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize("cin,cout,dtype", [(4, 8, torch.float32), (16, 16, torch.float32), (16, 16, torch.bfloat16),
                                            (32, 16, torch.bfloat16)])
def test_transposed_layer_is_conv_transpose3d(native_lib, cin, cout, dtype, geometry):
    from doda_amd import spconv
    k, s, p = geometry
    idx, shape, batch = SETS["batch of 2"]
    g = torch.Generator().manual_seed(cin + 7 * k)
    conv = spconv.SparseConvTranspose3d(cin, cout, k, stride=s, padding=p, indice_key="up").to(dev())
    x = torch.randn(idx.shape[0], cin, generator=g).to(dtype)
    xt = x.to(dev()).requires_grad_(True)
    t = spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev()), shape, batch)
    out = conv(t)
    data = t.indice_dict["up"]
    assert data.kind == "transpose" and out.indices is data.outids and out.spatial_shape == data.out_spatial_shape
    assert out.spatial_shape == spconv.ops.get_deconv_output_size(shape, [k] * 3, [s] * 3, [p] * 3, [1] * 3, [0] * 3)
    assert out.features.dtype == dtype and out.features.shape == (data.outids.shape[0], cout)
    gy = torch.randn(out.features.shape, generator=g).to(dtype)
    out.features.backward(gy.to(dev()))
    # the reference on the operands as the kernels see them: bf16 features mean bf16-rounded weights (and bias)
    rnd = (lambda v: v.detach().cpu().to(dtype).double())
    ref = _layer_reference(x.double(), rnd(conv.weight), rnd(conv.bias), idx, shape, batch, data.outids.cpu().numpy(),
                           out.spatial_shape, s, p, gy.double())
    tol = 1e-4 if dtype == torch.float32 else BF16_TOL
    errs = [rel_err(out.features.detach().float().cpu(), ref[0]), rel_err(xt.grad.float().cpu(), ref[1]),
            rel_err(conv.weight.grad.cpu(), ref[2]), rel_err(conv.bias.grad.cpu(), ref[3])]
    print("transposed layer", cin, cout, dtype, geometry, errs)
    assert errs[0] < tol and errs[1] < tol and errs[3] < tol, errs
    assert errs[2] < (1e-4 if dtype == torch.float32 else 3e-3), errs
    # a second layer under the same key reuses the cached rulebook object: nothing is built again
    conv2 = spconv.SparseConvTranspose3d(cin, cout, k, stride=s, padding=p, bias=False, indice_key="up").to(dev())
    out2 = conv2(t)
    assert t.indice_dict["up"] is data and out2.indices is data.outids and len(t.indice_dict) == 1


@pytest.mark.parametrize("geometry", ["k2s2 up-sampling", "k3s2p1 outpad1"])
def test_get_indice_pairs_transpose_lists_are_the_tables(native_lib, geometry):
    from doda_amd import spconv
    idx, shape, batch = SETS["batch of 2"]
    k, s, p, d, op = cases.GEOMETRIES[geometry]
    outids, pairs, num = spconv.ops.get_indice_pairs(torch.from_numpy(idx).to(dev()), batch, shape, k, s, p, d, out_padding=op,
                                                     transpose=True)
    ref = restated_rulebook("batch of 2", geometry)
    assert np.array_equal(outids.cpu().numpy(), ref[0])
    pairs, num = pairs.cpu().numpy(), num.cpu().numpy()
    for o in range(ref[2].shape[0]):
        j = np.nonzero(ref[2][o] >= 0)[0]
        assert num[o] == j.size and np.array_equal(pairs[0, o, :j.size], j) and np.array_equal(pairs[1, o, :j.size], ref[2][o, j])
        assert (pairs[:, o, j.size:] == -1).all()


# ------------------------------------------------------------------------------------------------ 3. max pooling
POOLS = {(2, 2, 0): "2000 voxels", (3, 2, 1): "batch of 2"}      # geometry -> voxel set (k2 s2 on 33 x 17 x 9 leaves rows unreached)


@functools.lru_cache(maxsize=None)
def _pool_rulebook(geometry):
    from doda_amd import spconv
    idx, shape, batch = SETS[POOLS[geometry]]
    k, s, p = geometry
    return spconv.ops.build_down2(torch.from_numpy(idx).to(dev()), batch, shape, k, s, p, 1)


@pytest.mark.parametrize("c", [1, 8, 20])
@pytest.mark.parametrize("geometry", list(POOLS))
def test_bf16_maxpool_is_the_restatement_bit_for_bit(native_lib, geometry, c):
    from doda_amd import ops, spconv
    idx, shape, batch = SETS[POOLS[geometry]]
    data = _pool_rulebook(geometry)
    tbl, tbl_rev = data.tbl.cpu().numpy(), data.tbl_rev.cpu().numpy()
    x, dy = cases.pool_inputs(11 + c, tbl, idx.shape[0], c)
    y_ref = cases.maxpool_fwd(x, tbl)
    dx_ref = cases.maxpool_bwd(x, y_ref, dy, tbl_rev)
    assert (y_ref == 0).any() and (y_ref > 0).any() and x.min() < 0
    winners = np.zeros(y_ref.shape, dtype=np.int32)           # inputs equal to their output's value, per (output, channel)
    for o in range(tbl.shape[0]):
        t = np.nonzero(tbl[o] >= 0)[0]
        winners[t] += x[tbl[o, t]] == y_ref[t]
    assert ((winners >= 2) & (y_ref > 0)).any()               # the designed ties: two inputs receive the same dy
    k, s, p = geometry
    pool = spconv.SparseMaxPool3d(k, s, p, indice_key="pool")
    xt = torch.from_numpy(x).bfloat16().to(dev()).requires_grad_(True)
    t = spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev()), shape, batch)
    t.indice_dict["pool"] = data
    out = pool(t)
    assert out.features.dtype == torch.bfloat16 and out.indices is data.outids
    assert torch.equal(bits(out.features), bits(torch.from_numpy(y_ref).bfloat16()))
    dyt = torch.from_numpy(dy).bfloat16().to(dev())
    out.features.backward(dyt)
    want = bits(torch.from_numpy(dx_ref).bfloat16())
    assert torch.equal(bits(xt.grad), want)
    # twice the same bits, and every row is written: a NaN-filled dx comes back with zeros where no output reaches
    nan = torch.full_like(xt.detach(), float("nan"))
    again = ops.maxpool_bwd_rows(xt.detach(), out.features.detach(), dyt, data.tbl_rev, dx=nan)
    assert again is nan and torch.equal(bits(again), want)
    unreached = (tbl_rev < 0).all(0)
    if geometry == (2, 2, 0):
        assert unreached.any()
    assert (again.float().cpu().numpy()[unreached] == 0).all()
    # the element-size entry points in fp32 give the same values
    y32 = ops.maxpool_fwd_rows(torch.from_numpy(x).to(dev()), data.tbl, data.outids.shape[0])
    dx32 = ops.maxpool_bwd_rows(torch.from_numpy(x).to(dev()), y32, torch.from_numpy(dy).to(dev()), data.tbl_rev)
    assert np.array_equal(y32.cpu().numpy(), y_ref) and np.array_equal(dx32.cpu().numpy(), dx_ref)


def test_fp32_maxpool_module_still_equals_the_oracle(native_lib, oracle):
    from doda_amd import spconv
    idx, shape, batch = SETS["batch of 2"]
    x = np.random.default_rng(2).standard_normal((idx.shape[0], 8)).astype(np.float32)
    oi, pairs, pn, _ = oracle.indice_pairs_conv(idx, batch, shape, 2, 2, 0, 1)
    ref = oracle.indice_maxpool(torch.from_numpy(x), pairs, pn, oi.shape[0])
    xt = torch.from_numpy(x).to(dev()).requires_grad_(True)
    out = spconv.SparseMaxPool3d(2, 2)(spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev()), shape, batch))
    assert out.features.dtype == torch.float32 and np.array_equal(out.features.detach().cpu().numpy(), ref.numpy())
    out.features.sum().backward()
    g = xt.grad.cpu().numpy()
    assert g.min() >= 0 and abs(g.sum() - (ref.numpy() > 0).sum()) < 1e-3


# ------------------------------------------------------------------------------------------------ 4. dense
@pytest.mark.parametrize("shape", [[9, 7, 5], [33, 17, 9]])
@pytest.mark.parametrize("c", [1, 3, 16, 20])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dense_and_from_dense_are_the_torch_expressions(native_lib, dtype, c, shape):
    from doda_amd import spconv
    from tests.util import random_voxels
    batch = 2
    idx = random_voxels(c + shape[0], 2000 if shape[0] == 33 else 150, batch, shape)
    g = torch.Generator().manual_seed(c)
    feats = torch.randn(idx.shape[0], c, generator=g).to(dtype)
    feats[5] = 0                                           # an all-zero row: kept by dense(), dropped by from_dense()
    if c > 1:
        feats[6, 0] = -0.0                                 # (a sign bit alone does not make a cell active)
    di = torch.from_numpy(idx).to(dev())
    for channels_first in (True, False):
        ft = feats.to(dev()).requires_grad_(True)
        t = spconv.SparseConvTensor(ft, di, shape, batch)
        got = t.dense(channels_first)
        want = cases.dense_expression(feats.to(dev()), di, shape, batch, channels_first)
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(bits(got), bits(want))
        grad = torch.randn(want.shape, generator=g).to(dtype).to(dev())
        got.backward(grad)
        cl = grad.permute(0, 2, 3, 4, 1) if channels_first else grad
        li = di.long()
        assert torch.equal(bits(ft.grad), bits(cl[li[:, 0], li[:, 1], li[:, 2], li[:, 3]]))
    # M = 0: all zeros
    empty = spconv.SparseConvTensor(torch.zeros(0, c, dtype=dtype, device=dev()), di[:0], shape, batch)
    assert float(empty.dense().float().abs().max()) == 0 and empty.dense().shape == (batch, c, *shape)
    # from_dense(dense(False)): the row-major sorted voxels come back, without the zeroed row
    vol = spconv.SparseConvTensor(feats.to(dev()), di, shape, batch).dense(False).detach().requires_grad_(True)
    back = spconv.SparseConvTensor.from_dense(vol)
    order = cases.row_major_order(idx, shape)
    order = order[order != 5]
    assert back.indices.dtype == torch.int32 and np.array_equal(back.indices.cpu().numpy(), idx[order])
    assert torch.equal(bits(back.features), bits(feats[torch.from_numpy(order)]))
    assert back.spatial_shape == shape and back.batch_size == batch
    ref_idx, ref_feats = cases.from_dense(vol.detach())
    assert torch.equal(back.indices, ref_idx) and torch.equal(bits(back.features), bits(ref_feats))
    # a gradient flows to the active cells of the dense input only
    gr = torch.randn(back.features.shape, generator=g).to(dtype).to(dev())
    back.features.backward(gr)
    assert torch.equal(bits(vol.grad), bits(cases.dense_expression(gr, back.indices, shape, batch, False)))
    assert not back.indices.requires_grad


# ------------------------------------------------------------------------------------------------ 5. end to end
def _stored(v, dtype):
    """v as the sparse graph stores it between layers: rounded to dtype, gradient passed straight through"""
    return v if dtype == torch.float32 else v + (v.detach().to(dtype).double() - v.detach())


def _dense_graph(x, ws, idx, shape, batch, dtype):
    """SubM(3->16) -> max pool k2 s2 -> SubM(16->16) -> transposed conv k2 s2 -> dense, as dense torch ops in fp64.  Only active
    sites carry values; the pool starts at 0 (upstream's clamp) and sends its gradient to every input equal to the maximum."""
    occ = cases.scatter_dense(torch.ones(idx.shape[0], 1, dtype=torch.float64), idx, shape, batch)
    h = _stored(F.conv3d(cases.scatter_dense(x, idx, shape, batch), ws[0].permute(4, 3, 0, 1, 2), padding=1) * occ, dtype)
    cand = torch.stack([torch.where(occ[:, :, a::2, b::2, c::2] > 0, h[:, :, a::2, b::2, c::2], torch.tensor(-np.inf, dtype=torch.float64))
                        for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    occ2 = F.max_pool3d(occ, 2)
    top = cand.max(0).values.clamp(min=0).detach()
    hit = (cand == top) & torch.isfinite(cand)
    safe = torch.where(hit, cand, torch.zeros_like(cand))
    pooled = (top + (safe - safe.detach()).sum(0)) * occ2
    h2 = _stored(F.conv3d(pooled, ws[1].permute(4, 3, 0, 1, 2), padding=1) * occ2, dtype)
    return _stored(F.conv_transpose3d(h2, ws[2].permute(3, 4, 0, 1, 2), stride=2), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_network_end_to_end_against_dense_torch(native_lib, dtype):
    """The tolerances of the layer test.  The dense graph rounds each layer's output to the feature dtype where the sparse graph
    stores it (bf16 rows between layers), so both sides pool over the same candidates; everything else is fp64."""
    from doda_amd import spconv
    idx, shape, batch = SETS["batch of 2"]
    torch.manual_seed(3)
    net = spconv.SparseSequential(spconv.SubMConv3d(3, 16, 3, padding=1, bias=False, indice_key="subm1"),
                                  spconv.SparseMaxPool3d(2, 2),
                                  spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="subm2"),
                                  spconv.SparseConvTranspose3d(16, 16, 2, 2, bias=False),
                                  spconv.ToDense()).to(dev())
    g = torch.Generator().manual_seed(4)
    x = torch.randn(idx.shape[0], 3, generator=g).to(dtype)
    xt = x.to(dev()).requires_grad_(True)
    out = net(spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev()), shape, batch))
    assert out.shape == (batch, 16, *shape) and out.dtype == dtype
    gy = torch.randn(out.shape, generator=g).to(dtype)
    out.backward(gy.to(dev()))
    convs = [net[0], net[2], net[3]]
    ws = [m.weight.detach().cpu().to(dtype).double().requires_grad_(True) for m in convs]
    xr = x.double().requires_grad_(True)
    ref = _dense_graph(xr, ws, idx, shape, batch, dtype)
    (ref * gy.double()).sum().backward()
    tol = 1e-4 if dtype == torch.float32 else BF16_TOL
    wtol = 1e-4 if dtype == torch.float32 else 3e-3
    errs = [rel_err(out.detach().float().cpu(), ref.detach()), rel_err(xt.grad.float().cpu(), xr.grad)]
    errs += [rel_err(m.weight.grad.cpu(), w.grad) for m, w in zip(convs, ws)]
    print("end to end", dtype, errs)
    assert errs[0] < tol and errs[1] < tol, errs
    assert max(errs[2:]) < wtol, errs

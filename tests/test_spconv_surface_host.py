"""The rest of the spconv surface, host side (no GPU): the serial transposed-rulebook restatement against fp64 F.conv_transpose3d,
get_deconv_output_size on hand-worked cases, the from_dense restatement against to_sparse, the plain modules on CPU tensors, the
max-pool restatement's designed ties, and the argument errors of include/doda_spconv.h as statuses.  (The header against its
record in doda_amd._lib.ABIS: tests/test_abi_host.py runs over every header under include/, this one included.)"""
import os

import numpy as np
import pytest
import torch

from tests import abi_header, spconv_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DODA_ERR_INVALID, DODA_ERR_UNSUPPORTED, DODA_ERR_WORKSPACE = -1, -4, -5      # include/doda_hip.h


@pytest.mark.parametrize("geometry", list(cases.GEOMETRIES))
@pytest.mark.parametrize("voxels", ["batch of 2", "eight corners", "one voxel"])
def test_serial_transposed_rulebook_is_conv_transpose3d(geometry, voxels):
    k, s, p, d, op = cases.GEOMETRIES[geometry]
    idx, shape, batch = cases.voxel_sets()[voxels]
    out_idx, tbl, tbl_rev, out_shape = cases.deconv_rulebook(idx, shape, k, s, p, d, op)
    kk = cases.triple(k)
    K = kk[0] * kk[1] * kk[2]
    assert tbl.shape == (K, out_idx.shape[0]) and tbl_rev.shape == (K, idx.shape[0])
    # the output set is the support of conv_transpose3d(occupancy, ones) on the upstream shape
    occ = cases.scatter_dense(torch.ones(idx.shape[0], 1, dtype=torch.float64), idx, shape, batch)
    reach = cases.conv_transpose_dense(occ, torch.ones(*kk, 1, 1, dtype=torch.float64), s, p, d, op, out_shape)
    support = (reach[:, 0] > 0).nonzero().numpy()
    assert len({tuple(r) for r in out_idx.tolist()}) == out_idx.shape[0]
    assert sorted(map(tuple, out_idx.tolist())) == sorted(map(tuple, support.tolist()))
    assert (reach[:, 0].numpy()[tuple(out_idx.T.astype(np.int64))] == (tbl >= 0).sum(0)).all()       # inputs per output
    # the values: sum over offsets of x[tbl[o]] @ W[o] against the dense result sampled at the outputs
    g = torch.Generator().manual_seed(5)
    x = torch.randn(idx.shape[0], 3, generator=g, dtype=torch.float64)
    w = torch.randn(*kk, 3, 5, generator=g, dtype=torch.float64)
    y = torch.zeros(out_idx.shape[0], 5, dtype=torch.float64)
    for o in range(K):
        t = np.nonzero(tbl[o] >= 0)[0]
        y[t] += x[tbl[o, t]] @ w.reshape(K, 3, 5)[o]
    ref = cases.sample(cases.conv_transpose_dense(cases.scatter_dense(x, idx, shape, batch), w, s, p, d, op, out_shape), out_idx)
    assert float((y - ref).abs().max()) < 1e-12
    # tbl and tbl_rev describe the same triples
    for o in range(K):
        j = np.nonzero(tbl_rev[o] >= 0)[0]
        assert (tbl[o, tbl_rev[o, j]] == j).all() and (tbl[o] >= 0).sum() == j.size


def test_first_touch_order_of_a_hand_worked_case():
    """One voxel at (1, 1, 1), k2 s2: its eight outputs from the upper bound (3, 3, 3) downwards, last axis fastest, and the offset
    index of q is the row-major index of (q - lower)."""
    out_idx, tbl, tbl_rev, out_shape = cases.deconv_rulebook(np.array([[0, 1, 1, 1]]), [2, 2, 2], 2, 2, 0, 1, 0)
    assert out_shape == [4, 4, 4]
    assert out_idx.tolist() == [[0, 3, 3, 3], [0, 3, 3, 2], [0, 3, 2, 3], [0, 3, 2, 2], [0, 2, 3, 3], [0, 2, 3, 2], [0, 2, 2, 3], [0, 2, 2, 2]]
    assert tbl_rev[:, 0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]


def test_get_deconv_output_size_hand_worked():
    from doda_amd.spconv import ops
    f = ops.get_deconv_output_size
    assert f([5, 6, 7], [2, 2, 2], [2, 2, 2], [0, 0, 0], [1, 1, 1], [0, 0, 0]) == [10, 12, 14]
    assert f([5, 6, 7], [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0]) == [5, 6, 7]
    assert f([5, 6, 7], [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], [0, 0, 0]) == [9, 11, 13]
    assert f([5, 6, 7], [3, 3, 3], [2, 2, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1]) == [10, 12, 14]
    assert f([4, 4, 4], [1, 3, 2], [1, 2, 2], [0, 1, 0], [1, 1, 1], [0, 1, 0]) == [4, 8, 8]
    assert f([4, 4, 4], [3, 3, 3], [1, 1, 1], [0, 0, 0], [2, 2, 2], [0, 0, 0]) == [6, 6, 6]      # dilation is ignored
    assert f([4, 4, 4], [3, 3, 3], [1, 1, 1], [0, 0, 0], [2, 2, 2], [0, 0, 0]) == cases.deconv_output_size(
        [4, 4, 4], [3, 3, 3], [1, 1, 1], [0, 0, 0], [2, 2, 2], [0, 0, 0])
    assert "[MEM]" in f.__doc__


def test_from_dense_is_to_sparse_order_on_cpu():
    from doda_amd import spconv
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 4, 3, 2, generator=g) * (torch.rand(2, 5, 4, 3, 1, generator=g) < 0.3)
    x[1, 2, 3, 1] = torch.tensor([0.0, -0.0])                                   # all-zero features: no voxel
    x[0, 0, 0, 0] = torch.tensor([0.0, 2.0])                                    # one non-zero channel is enough
    sp = x.to_sparse(4).coalesce()
    for idx, feats in (cases.from_dense(x), (lambda t: (t.indices, t.features))(spconv.SparseConvTensor.from_dense(x))):
        assert idx.dtype == torch.int32 and torch.equal(idx.long(), sp.indices().t())
        assert torch.equal(feats, sp.values())
        assert not (idx.long() == torch.tensor([1, 2, 3, 1])).all(1).any() and (idx.long() == 0).all(1).any()
    t = spconv.SparseConvTensor.from_dense(x)
    assert t.spatial_shape == [5, 4, 3] and t.batch_size == 2
    assert torch.equal(t.dense(False), x) and torch.equal(t.dense(), x.permute(0, 4, 1, 2, 3))
    assert torch.equal(t.dense(), cases.dense_expression(t.features, t.indices, t.spatial_shape, 2))


def _tensor(seed, c, m=20, shape=(6, 5, 4)):
    from doda_amd import spconv
    from tests.util import random_voxels
    idx = torch.from_numpy(random_voxels(seed, m, 2, list(shape)))
    feats = torch.randn(idx.shape[0], c, generator=torch.Generator().manual_seed(seed))
    return spconv.SparseConvTensor(feats, idx, list(shape), 2, grid=torch.zeros(1))


def test_plain_modules_on_cpu_tensors():
    from doda_amd import spconv
    from doda_amd.shims import spconv as shim
    a = _tensor(1, 3)
    b = a.header(a.features * 2 + 1)
    c = a.header(torch.ones(a.features.shape[0], 2))
    added = spconv.AddTable()([a, b, c.header(a.features)])
    assert torch.equal(added.features, a.features + b.features + a.features) and added.indices is a.indices
    assert added.indice_dict is a.indice_dict and added is not a
    joined = spconv.JoinTable()([a, c])
    assert torch.equal(joined.features, torch.cat([a.features, c.features], 1)) and joined.spatial_shape == a.spatial_shape
    table = spconv.ConcatTable()
    table.add(spconv.Identity()).add(spconv.SparseSequential(torch.nn.ReLU())).add(spconv.Identity())
    outs = table(a.header(a.features))
    assert isinstance(outs, list) and len(outs) == 3 == len(list(table.children()))
    assert spconv.Identity()(a) is a
    dense = spconv.ToDense()(a)
    assert torch.equal(dense, a.dense()) and dense.shape == (2, 3, 6, 5, 4)
    assert a.grid is not None and spconv.RemoveGrid()(a) is a and a.grid is None
    # a branch-and-join block and a dense head in one SparseSequential
    net = spconv.SparseSequential(spconv.ConcatTable().add(spconv.Identity()).add(spconv.Identity()), spconv.AddTable(),
                                  spconv.ToDense(), torch.nn.Conv3d(3, 2, 1))
    a = _tensor(1, 3)
    assert net(a).shape == (2, 2, 6, 5, 4)
    for name in ("SparseConvTranspose3d", "ToDense", "RemoveGrid", "Identity", "ConcatTable", "AddTable", "JoinTable"):
        assert getattr(shim, name) is getattr(spconv, name) and name in spconv.__all__


def test_transposed_layer_surface():
    from doda_amd import spconv
    conv = spconv.SparseConvTranspose3d(4, 8, (1, 3, 2), stride=(1, 2, 2), padding=(0, 1, 0), bias=True, indice_key="up")
    assert conv.transposed and not conv.subm and not conv.inverse and conv.output_padding == [0, 0, 0]
    assert tuple(conv.weight.shape) == (1, 3, 2, 4, 8) and tuple(conv.bias.shape) == (8,)
    assert spconv.SparseConvolution(3, 4, 8, 2, 2, transposed=True, output_padding=1).output_padding == [1, 1, 1]
    with pytest.raises(NotImplementedError):
        spconv.SparseConvTranspose3d(4, 8, 2, 2, groups=2)
    with pytest.raises(NotImplementedError, match="27"):          # kernel volumes above 27 stay unsupported
        spconv.ops.build_transpose(torch.zeros((1, 4), dtype=torch.int32), 1, [8, 8, 8], 4, 2, 0, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(spconv.SparseConvTensor(torch.zeros(1, 4), torch.zeros((1, 4), dtype=torch.int32), [8, 8, 8], 1))
    # SparseInverseConv3d over a transposed layer's key is out of scope, and says so
    t = spconv.SparseConvTensor(torch.zeros(1, 8), torch.zeros((1, 4), dtype=torch.int32), [8, 8, 8], 1)
    t.indice_dict["up"] = spconv.IndiceData("transpose", t.indices, t.indices, [8, 8, 8], [8, 8, 8], None, None)
    with pytest.raises(NotImplementedError, match="SparseConvTranspose3d"):
        spconv.SparseInverseConv3d(8, 4, 2, indice_key="up")(t)
    from doda_amd.spconv import pool
    assert "volume of at most 27" in pool.__doc__


def test_maxpool_restatement_and_designed_ties():
    idx, shape, batch = cases.voxel_sets()["batch of 2"]
    # k2 s2 as a (degenerate) rulebook built here: output cell = input cell // 2
    cells = {}
    tbl_rev = np.full((8, idx.shape[0]), -1, dtype=np.int32)
    for j, (b, x, y, z) in enumerate(idx.tolist()):
        t = cells.setdefault((b, x // 2, y // 2, z // 2), len(cells))
        tbl_rev[(x % 2) * 4 + (y % 2) * 2 + (z % 2), j] = t
    tbl = np.full((8, len(cells)), -1, dtype=np.int32)
    for o in range(8):
        j = np.nonzero(tbl_rev[o] >= 0)[0]
        tbl[o, tbl_rev[o, j]] = j
    x, dy = cases.pool_inputs(7, tbl, idx.shape[0], 3)
    assert np.array_equal(x, torch.from_numpy(x).bfloat16().float().numpy()) and x.min() < 0 < x.max()     # exact in bf16
    y = cases.maxpool_fwd(x, tbl)
    assert y.min() == 0 and (y >= 0).all()                                                                  # the clamp at 0
    dx = cases.maxpool_bwd(x, y, dy, tbl_rev)
    ties = [t for t in range(tbl.shape[1]) if (tbl[:, t] >= 0).sum() >= 2 and (y[t] > 0).all()
            and sum(np.array_equal(x[j], y[t]) for j in tbl[:, t] if j >= 0) >= 2]
    assert ties
    for t in ties[:5]:
        js = [j for j in tbl[:, t] if j >= 0 and np.array_equal(x[j], y[t])]
        assert all(np.array_equal(dx[j], dy[t]) for j in js)
    # every unit of dy arrives once per input that equals its output's maximum
    hits = sum((x[tbl[o, t]] == y[t]) * dy[t] for o in range(8) for t in np.nonzero(tbl[o] >= 0)[0])
    assert float(dx.sum()) == float(np.asarray(hits, dtype=np.float64).sum())


def test_header_record_and_argument_errors(native_lib):
    from doda_amd import _lib
    abi = {a.header: a for a in _lib.ABIS}["doda_spconv.h"]
    with open(os.path.join(ROOT, "include", "doda_spconv.h")) as f:
        assert abi_header.compare(f.read(), abi) == []
    assert native_lib.doda_spconv_abi_version() == abi.version == 1 and len(abi.signatures) == 11
    assert (_lib.SPCONV_MAX_KERNEL_VOLUME, _lib.SPCONV_DENSE_CHUNK) == (27, 1024)
    import ctypes as C
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    out_shape = i3(0, 0, 0)
    lib = native_lib
    # statuses before anything launches (no device pointer is ever touched here)
    assert lib.doda_rulebook_deconv_workspace_bytes(10, 64) == 0 and lib.doda_rulebook_deconv_workspace_bytes(10, 27) > 0
    assert lib.doda_rulebook_deconv_assign(None, 5, i3(8, 8, 8), 1, i3(4, 4, 4), i3(2, 2, 2), i3(0, 0, 0), i3(1, 1, 1), i3(0, 0, 0),
                                           out_shape, 1, None, 0, None) == DODA_ERR_UNSUPPORTED                 # K = 64
    assert lib.doda_rulebook_deconv_assign(None, 5, i3(8, 8, 8), 1, i3(2, 2, 2), i3(2, 2, 2), i3(0, 0, 0), i3(1, 1, 1), i3(-1, 0, 0),
                                           out_shape, 1, None, 0, None) == DODA_ERR_INVALID                     # negative output_padding
    assert lib.doda_rulebook_deconv_assign(None, 5, i3(2, 2, 2), 1, i3(1, 1, 1), i3(1, 1, 1), i3(3, 3, 3), i3(1, 1, 1), i3(0, 0, 0),
                                           out_shape, 1, None, 0, None) == DODA_ERR_INVALID                     # output extent < 1
    assert lib.doda_rulebook_deconv_assign(None, 5, i3(8, 8, 8), 1, i3(2, 2, 2), i3(2, 2, 2), i3(0, 0, 0), i3(1, 1, 1), i3(0, 0, 0),
                                           out_shape, 1, None, 0, None) == DODA_ERR_INVALID                     # null indices, m > 0
    assert list(out_shape) == [16, 16, 16]
    assert lib.doda_rulebook_deconv_tables(None, 5, i3(8, 8, 8), 1, i3(2, 2, 2), i3(2, 2, 2), i3(0, 0, 0), i3(1, 1, 1), i3(0, 0, 0),
                                           9, None, None, 8, None, 5, None, 0, None) == DODA_ERR_INVALID        # ld_out < m_out
    assert lib.doda_maxpool_fwd(None, 0, 2, None, 0, 8, 0, 0, None, None) == DODA_ERR_INVALID
    assert lib.doda_maxpool_fwd(None, 8, 3, None, 4, 8, 4, 4, None, None) == DODA_ERR_UNSUPPORTED
    assert lib.doda_maxpool_fwd(None, 8, 2, None, 3, 8, 4, 4, None, None) == DODA_ERR_INVALID                   # ld < n_out
    assert lib.doda_maxpool_fwd(None, 8, 2, None, 0, 8, 4, 0, None, None) == 0                                  # nothing to do
    assert lib.doda_maxpool_bwd(None, None, None, 8, 8, None, 4, 8, 4, 4, None, None) == DODA_ERR_UNSUPPORTED
    assert lib.doda_maxpool_bwd(None, None, None, 8, 2, None, 4, 8, 4, 4, None, None) == DODA_ERR_INVALID
    assert lib.doda_dense_scatter(None, None, 0, 4, 2, 1, i3(2, 2, 2), 1, None, None) == DODA_ERR_INVALID      # null volume
    assert lib.doda_dense_scatter(None, None, 0, 4, 8, 1, i3(2, 2, 2), 1, 1, None) == DODA_ERR_UNSUPPORTED
    assert lib.doda_dense_gather(None, None, 0, 4, 2, 0, i3(2, 2, 2), 1, None, None) == DODA_ERR_INVALID       # batch < 1
    assert lib.doda_from_dense_workspace_bytes(1 << 31) == 0 and lib.doda_from_dense_workspace_bytes(2049) == 256
    assert lib.doda_from_dense_count(None, 4, 2, 1, i3(2, 2, 2), None, None, 0, None) == DODA_ERR_INVALID
    assert lib.doda_from_dense_count(None, 4, 2, 4, i3(1024, 1024, 1024), None, None, 0, None) == DODA_ERR_UNSUPPORTED
    assert lib.doda_from_dense_count(1, 4, 2, 1, i3(64, 64, 64), 1, 1, 16, None) == DODA_ERR_WORKSPACE
    assert lib.doda_from_dense_emit(None, 4, 2, 1, i3(2, 2, 2), -1, None, None, None, 0, None) == DODA_ERR_INVALID

"""Restatements of the entry points of include/doda_spconv.h, written from their semantics, and the designed inputs the host and GPU
tests share: the serial transposed-convolution rulebook (first-touch numbering of a scan over the inputs), indice max pooling with
upstream's clamp at 0 and its input-stationary gradient, the torch expression of SparseConvTensor.dense() as it stood before the
device route, and from_dense as `to_sparse` defines it.  Dense references use oracle/dense_ref.py's scatter_dense and sample."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.dense_ref import sample, scatter_dense  # noqa: F401  (re-exported for the tests)
from tests.util import random_voxels

# (kernel, stride, padding, dilation, output_padding) of the transposed-rulebook tests
GEOMETRIES = {
    "k2s2 up-sampling": (2, 2, 0, 1, 0),
    "k3s1p1 grows": (3, 1, 1, 1, 0),
    "k3s2p1 outpad1": (3, 2, 1, 1, 1),
    "k132 s122 p010": ((1, 3, 2), (1, 2, 2), (0, 1, 0), 1, 0),
    "k3 dilation2": (3, 1, 0, 2, 0),
}


def triple(v):
    return [int(x) for x in v] if isinstance(v, (tuple, list)) else [int(v)] * 3


def deconv_output_size(shape, k, s, p, d, op):
    return [(shape[a] - 1) * s[a] - 2 * p[a] + k[a] + op[a] for a in range(3)]


def deconv_rulebook(indices, shape, ksize, stride, padding, dilation, output_padding):
    """Serial scan: inputs ascending; each input's positions from the upper bound lower + (k - 1) * dilation downwards, last axis
    fastest; a position outside the output shape is dropped; the first touch of a cell numbers it.  Returns (out_indices [M_out, 4],
    tbl [K, M_out], tbl_rev [K, M_in], out_shape)."""
    k, s, p, d, op = (triple(v) for v in (ksize, stride, padding, dilation, output_padding))
    out_shape = deconv_output_size(shape, k, s, p, d, op)
    K = k[0] * k[1] * k[2]
    idx = np.asarray(indices).reshape(-1, 4)
    cell_to_out, out_indices, triples = {}, [], []
    for j, (b, *pos) in enumerate(idx.tolist()):
        lower = [pos[a] * s[a] - p[a] for a in range(3)]
        upper = [lower[a] + (k[a] - 1) * d[a] for a in range(3)]
        for c0 in range(k[0]):
            for c1 in range(k[1]):
                for c2 in range(k[2]):
                    q = [upper[a] - c * d[a] for a, c in enumerate((c0, c1, c2))]
                    if any(q[a] < 0 or q[a] > out_shape[a] - 1 for a in range(3)):
                        continue
                    off, mul = 0, 1
                    for a in (2, 1, 0):
                        off += mul * ((q[a] - lower[a]) // d[a])
                        mul *= k[a]
                    cell = (b, q[0], q[1], q[2])
                    t = cell_to_out.get(cell)
                    if t is None:
                        t = cell_to_out[cell] = len(out_indices)
                        out_indices.append(cell)
                    triples.append((off, j, t))
    tbl = np.full((K, len(out_indices)), -1, dtype=np.int32)
    tbl_rev = np.full((K, idx.shape[0]), -1, dtype=np.int32)
    for off, j, t in triples:
        assert tbl[off, t] == -1 and tbl_rev[off, j] == -1          # injective per offset: no entry is written twice
        tbl[off, t] = j
        tbl_rev[off, j] = t
    return np.asarray(out_indices, dtype=np.int32).reshape(-1, 4), tbl, tbl_rev, out_shape


def conv_transpose_dense(x_dense, weight, stride, padding, dilation, output_padding, out_shape):
    """F.conv_transpose3d of a dense [B, Cin, X, Y, Z] volume with a [k0, k1, k2, Cin, Cout] weight, on the window
    [padding, padding + out_shape) of the unpadded result (every cell p * stride + k * dilation): padding crops the low side,
    output_padding moves the high side, and the upstream shape ignores dilation where torch's does not.  Cells of the window
    beyond the unpadded result (nothing reaches them) are zero.  output_padding itself enters through out_shape only."""
    s, p, d = (triple(v) for v in (stride, padding, dilation))
    y = F.conv_transpose3d(x_dense, weight.permute(3, 4, 0, 1, 2), stride=s, padding=0, dilation=d)
    pad = []
    for a in (2, 1, 0):
        pad += [0, max(0, p[a] + out_shape[a] - y.shape[2 + a])]
    y = F.pad(y, pad)
    return y[:, :, p[0]:p[0] + out_shape[0], p[1]:p[1] + out_shape[1], p[2]:p[2] + out_shape[2]]


def voxel_sets():
    """name -> (indices int32 [M, 4], spatial shape, batch size)"""
    shape = [12, 10, 8]
    sets = {"batch of 2": (random_voxels(31, 300, 2, shape), shape, 2)}
    only1 = random_voxels(32, 150, 1, shape)
    only1[:, 0] = 1
    sets["item 0 empty"] = (only1, shape, 2)
    corners = np.array([[0, x, y, z] for x in (0, 11) for y in (0, 9) for z in (0, 7)], dtype=np.int32)
    sets["eight corners"] = (corners, shape, 1)
    sets["one voxel"] = (np.array([[0, 5, 4, 3]], dtype=np.int32), shape, 1)
    sets["2000 voxels"] = (random_voxels(33, 2000, 1, [33, 17, 9]), [33, 17, 9], 1)
    return sets


# ---------------------------------------------------------------------------------------------------------------------------
# max pooling
# ---------------------------------------------------------------------------------------------------------------------------
def maxpool_fwd(x, tbl):
    """x float32 [n_in, c], tbl [K, n_out]: out starts at 0 and is max-ed with every paired input."""
    y = np.zeros((tbl.shape[1], x.shape[1]), dtype=np.float32)
    for o in range(tbl.shape[0]):
        t = np.nonzero(tbl[o] >= 0)[0]
        y[t] = np.maximum(y[t], x[tbl[o, t]])
    return y


def maxpool_bwd(x, y, dy, tbl_rev):
    """dx[j] = sum over o (ascending, fp32) of dy[t] * [x[j] == y[t]], t = tbl_rev[o][j]; rows that reach no output stay 0."""
    dx = np.zeros_like(x, dtype=np.float32)
    for o in range(tbl_rev.shape[0]):
        j = np.nonzero(tbl_rev[o] >= 0)[0]
        t = tbl_rev[o, j]
        dx[j] = dx[j] + np.where(x[j] == y[t], dy[t], np.float32(0)).astype(np.float32)
    return dx


def pool_values(rng, shape):
    """Multiples of 2^-3 in [-16, 16]: exact in bf16, and every fp32 sum of at most 27 of them is exact."""
    return (rng.integers(-128, 129, size=shape) / 8.0).astype(np.float32)


def pool_inputs(seed, tbl, n_in, c):
    """(x, dy) of the value set above with designed ties: in every output with at least two inputs, the second input is set equal
    to the output's maximum in every channel, so both receive dy."""
    rng = np.random.default_rng(seed)
    x = pool_values(rng, (n_in, c))
    used = set()
    for t in range(tbl.shape[1]):
        js = [int(j) for j in tbl[:, t] if j >= 0]
        if len(js) >= 2 and not (used & set(js)):
            x[js[1]] = x[js].max(0)
            used.update(js)
    return x, pool_values(rng, (tbl.shape[1], c))


# ---------------------------------------------------------------------------------------------------------------------------
# dense volumes
# ---------------------------------------------------------------------------------------------------------------------------
def dense_expression(features, indices, spatial_shape, batch_size, channels_first=True):
    """SparseConvTensor.dense() as the torch expression it was before the device route: the bits every route must give."""
    idx = indices.long()
    shape = [batch_size] + list(spatial_shape) + [features.shape[1]]
    out = torch.zeros(shape, dtype=features.dtype, device=features.device)
    out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = features
    if not channels_first:
        return out
    return out.permute(0, 4, 1, 2, 3).contiguous()


def from_dense(x):
    """(indices int32 [M, 4], features [M, C]) of x [B, X, Y, Z, C]: the cells where any channel is non-zero, row-major."""
    mask = (x != 0).any(-1)
    return mask.nonzero().int(), x[mask]


def row_major_order(indices, spatial_shape):
    idx = np.asarray(indices).astype(np.int64)
    lin = ((idx[:, 0] * spatial_shape[0] + idx[:, 1]) * spatial_shape[1] + idx[:, 2]) * spatial_shape[2] + idx[:, 3]
    return np.argsort(lin, kind="stable")

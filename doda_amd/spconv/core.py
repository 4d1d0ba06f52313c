"""SparseConvTensor and the rulebook record kept in its indice_dict."""
import numpy as np
import torch

from .. import ops as _ops


import os as _os
_TRACE_PAIRS = _os.environ.get("DODA_TRACE_PAIRS", "0") == "1"


class IndiceData:
    """Rulebook of one indice_key.

    Behaves like spconv v1.2's 5-tuple `(outids, indices, indice_pairs, indice_pair_num,
    spatial_shape)` (unpacking and [i] indexing work), but the native record is the gather
    table(s) of include/doda_hip.h; the spconv-format pairs are materialised on first access.

    kind 'subm' : tbl = nbr int32 [27, M]
    kind 'down2': tbl = child int32 [8, M_out]; tbl_rev = par_off int32 [8, M_in]
                  (generic strided geometry: tbl int32 [K, M_out], tbl_rev int32 [K, M_in])
    kind 'transpose': the generic pair of a SparseConvTranspose3d, tbl int32 [K, M_out], tbl_rev int32 [K, M_in]
    """

    def __init__(self, kind, outids, indices, spatial_shape, out_spatial_shape, tbl, tbl_rev=None):
        self.kind = kind
        self.outids = outids
        self.indices = indices
        self.spatial_shape = spatial_shape
        self.out_spatial_shape = out_spatial_shape
        self.tbl = tbl
        self.tbl_rev = tbl_rev
        self._pairs = None
        self._wpairs = None   # (pairs int32 [2,K,n_in] without the -1 fill, pair_num) for the weight gradient

    def _export(self):
        if self._pairs is None:
            n_in = self.indices.shape[0]
            if self.kind == "subm":
                self._pairs = _ops.rulebook_pairs(self.tbl, n_in, flip=True)
            else:
                self._pairs = _ops.rulebook_pairs(self.tbl_rev, n_in, flip=False)
        return self._pairs

    def wgrad_lists(self, inverse=False):
        """(pair_in [K,ld], pair_out [K,ld], pair_num [K], seg [K,nt]) of the pair-list weight gradient
        (doda_spconv_wgrad_multi's pair-list kernel): list o pairs the row of the conv INPUT with the row of the conv
        OUTPUT under offset o, in ascending input row; seg is the lists' per-256-row prefix.  Exported
        once per rulebook (doda_rulebook_pairs without the -1 fill)."""
        if self._wpairs is None:
            n_in = self.indices.shape[0]
            if _TRACE_PAIRS:
                import sys
                import traceback
                sys.stderr.write("[doda] lazy pair-list export: kind %s, %d rows, inverse %s, from %s\n" % (
                    self.kind, n_in, inverse, " <- ".join("%s:%d" % (f.name, f.lineno) for f in reversed(traceback.extract_stack(limit=6)[:-1]))))
            if self.kind == "subm":
                self._wpairs = _ops.rulebook_pairs(self.tbl, n_in, flip=True, pad=False, with_seg=True)
            else:
                self._wpairs = _ops.rulebook_pairs(self.tbl_rev, n_in, flip=False, pad=False, with_seg=True)
        pairs, num, seg = self._wpairs
        # (the inverse convolution reads the same lists with the operand roles swapped; the segment prefix
        # belongs to the ascending list, whichever operand it indexes)
        return (pairs[1], pairs[0], num, seg) if inverse else (pairs[0], pairs[1], num, seg)

    @property
    def indice_pairs(self):
        return self._export()[0]

    @property
    def indice_pair_num(self):
        return self._export()[1]

    def _as_tuple(self):
        return (self.outids, self.indices, self.indice_pairs, self.indice_pair_num,
                self.spatial_shape)

    def __iter__(self):
        return iter(self._as_tuple())

    def __len__(self):
        return 5

    def __getitem__(self, i):
        return self._as_tuple()[i]


class IndiceDict(dict):
    """`SparseConvTensor.indice_dict`: indice_key -> IndiceData, shared by every tensor derived from one
    network input.  `pack_gen` is the weight-pack generation of the forward pass that owns the dictionary
    (doda_amd.spconv.conv: packed weight copies are refreshed once per forward pass); it lives in a slot,
    not under a key, so code that walks the rulebooks never meets it."""
    __slots__ = ("pack_gen",)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pack_gen = None


def dense_torch(features, indices, batch_size, spatial_shape, channels_first=True):
    """dense() as a torch expression: zeros, an indexed put in channels-last order, then the permutation."""
    idx = indices.long()
    shape = [batch_size] + list(spatial_shape) + [features.shape[1]]
    out = torch.zeros(shape, dtype=features.dtype, device=features.device)
    out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = features
    if not channels_first:
        return out
    ndim = len(spatial_shape)
    return out.permute(0, ndim + 1, *range(1, ndim + 1)).contiguous()


class _Dense(torch.autograd.Function):
    """rows -> volume by doda_dense_scatter; the gradient gathers the rows back (doda_dense_gather)."""

    @staticmethod
    def forward(ctx, features, indices, batch_size, spatial_shape, channels_first):
        ctx.args = (indices, channels_first)
        return _ops.dense_scatter(features.contiguous(), indices, batch_size, spatial_shape, channels_first)

    @staticmethod
    def backward(ctx, grad):
        indices, channels_first = ctx.args
        return _ops.dense_gather(grad.contiguous(), indices, channels_first), None, None, None, None


class _FromDense(torch.autograd.Function):
    """volume -> (rows, indices) by doda_from_dense_count / _emit; the gradient scatters the rows' gradient into a zero volume."""

    @staticmethod
    def forward(ctx, x):
        indices, rows = _ops.from_dense(x.contiguous())
        ctx.args = (indices, x.shape[0], tuple(x.shape[1:4]))
        ctx.mark_non_differentiable(indices)
        return rows, indices

    @staticmethod
    def backward(ctx, grad_rows, _grad_indices):
        indices, batch, shape = ctx.args
        return _ops.dense_scatter(grad_rows.contiguous(), indices, batch, shape, False)


class SparseConvTensor:
    """features [M,C] + indices int32 [M,4] (batch,x,y,z) + spatial_shape + batch_size.

    Mirrors spconv v1.2 SparseConvTensor as used at reference model/unet.py:94 and
    model/unet_block.py:33,89 (rw attributes features/indices/spatial_shape/batch_size,
    indice_dict shared along the network, grid carried but unused by the hash builders)."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features = features
        self.indices = indices
        # (a plain list of ints — what the conv modules pass along — skips the numpy round trip)
        self.spatial_shape = list(spatial_shape) if type(spatial_shape) is list else \
            [int(v) for v in np.asarray(spatial_shape).reshape(-1)]
        self.batch_size = int(batch_size)
        self.indice_dict = IndiceDict()
        self.grid = grid

    def header(self, features, indices=None, spatial_shape=None):
        """A tensor of the same forward pass over other features (behind a strided layer: other indices and shape) that shares the
        rulebooks, their weight-pack generation and the grid; also what a branch that must keep the incoming features takes, since
        SparseSequential re-binds `.features` on the object it is given (reference unet_block.py:33,89)."""
        out = SparseConvTensor(features, self.indices if indices is None else indices,
                               self.spatial_shape if spatial_shape is None else spatial_shape, self.batch_size, self.grid)
        out.indice_dict = self.indice_dict
        return out

    # BatchNorm statistics partials (sum y, sum y^2) that the producing convolution accumulated in its epilogue.  They belong to one
    # tensor object AND one version of it: `output.features += skip` (reference model/unet_block.py:36) edits the same object in
    # place.  (__dict__, not getattr with a default: a missing attribute on this path costs an exception per call.)
    def stats(self):
        """The epilogue statistics of the current `.features`: a tensor, the pair of a channel concatenation's halves, or None."""
        st = self.__dict__.get("_doda_stats")
        if st is None:
            return None
        feats = self.features
        return st[1] if (st[0] is feats and st[2] == feats._version) else None

    def set_stats(self, stats):
        feats = self.features
        self.__dict__["_doda_stats"] = (feats, stats, feats._version)

    def clear_stats(self):
        self.__dict__.pop("_doda_stats", None)

    @property
    def spatial_size(self):
        return int(np.prod(self.spatial_shape))

    def find_indice_pair(self, key):
        if key is None:
            return None
        return self.indice_dict.get(key)

    def dense(self, channels_first=True):
        """The dense volume [B, C, X, Y, Z] (channels_first) or [B, X, Y, Z, C]; the indices must be unique.  fp32 / bf16 device
        features with int32 indices: one native scatter straight into the requested layout (doda_dense_scatter), differentiable
        through the features; anything else: the torch expression, with the same bits."""
        feats = self.features
        if (feats.is_cuda and feats.dtype in (torch.float32, torch.bfloat16) and feats.dim() == 2 and feats.shape[1] > 0
                and self.indices.is_cuda and self.indices.dtype == torch.int32 and len(self.spatial_shape) == 3
                and self.batch_size > 0):
            return _Dense.apply(feats, self.indices, self.batch_size, tuple(self.spatial_shape), bool(channels_first))
        return dense_torch(feats, self.indices, self.batch_size, self.spatial_shape, channels_first)

    @classmethod
    def from_dense(cls, x):
        """The sparse tensor of a channels-last dense volume x [B, X, Y, Z, C]: a cell is active iff any channel is non-zero; rows
        in row-major (b, x, y, z) order (the coalesced order of x.to_sparse(4)), indices int32.  Device fp32 / bf16 volumes: flag,
        stable compaction and row copy on the device with one size read-back.  Not differentiable through the indices;
        differentiable through the features (a gather, whose gradient is the scatter)."""
        if x.dim() != 5:
            raise ValueError("from_dense expects [B, X, Y, Z, C], got %r" % (tuple(x.shape),))
        shape, batch = [int(v) for v in x.shape[1:4]], int(x.shape[0])
        if x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.numel() > 0:
            feats, indices = _FromDense.apply(x)
        else:
            mask = (x != 0).any(-1)
            indices = mask.nonzero().int()
            feats = x[mask]
        return cls(feats, indices, shape, batch)

    @property
    def sparity(self):
        return self.indices.shape[0] / max(self.spatial_size * self.batch_size, 1)

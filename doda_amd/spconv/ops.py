"""Rulebook construction at the level of spconv v1.2 `spconv.ops` (get_conv_output_size,
get_indice_pairs).  The geometries DODA instantiates — SubM with a cubic kernel of 1 or 3 and the
kernel-2 / stride-2 / padding-0 convolution (model/unet.py:36, model/unet_block.py:18-29,48,70,78) —
have dedicated native builders; any other kernel_size / stride / padding / dilation with a kernel
volume of at most 27 goes through the generic one (doda_rulebook_conv_*, doda_rulebook_subm_generic), and the transposed
convolution through the same builder's second enumeration (doda_rulebook_deconv_*, include/doda_spconv.h)."""
import os

import numpy as np

import torch

from .. import ops as _ops
from .._ext import ext as _ext
from .core import IndiceData


def _triple(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        out = [int(x) for x in v]
        if len(out) != 3:
            raise ValueError("expected 3 values, got %r" % (v,))
        return out
    return [int(v)] * 3


def get_conv_output_size(input_size, kernel_size, stride, padding, dilation):
    out = []
    for i in range(len(input_size)):
        size = (input_size[i] + 2 * padding[i] - dilation[i] * (kernel_size[i] - 1) - 1) // stride[i] + 1
        out.append(1 if kernel_size[i] == -1 else size)
    return out


def build_subm(indices, batch_size, spatial_shape, ksize):
    k = _triple(ksize)
    if any(v % 2 == 0 or v < 1 for v in k) or k[0] * k[1] * k[2] > 27:
        raise NotImplementedError("doda_amd SubMConv3d supports odd kernel sizes with volume <= 27, got %r" % (k,))
    if k[0] == k[1] == k[2]:
        tbl = _ops.rulebook_subm(indices, spatial_shape, batch_size, k[0])
    else:
        tbl = _ops.rulebook_subm_generic(indices, spatial_shape, batch_size, k)
    return IndiceData("subm", indices, indices, list(spatial_shape), list(spatial_shape), tbl)


def build_down2(indices, batch_size, spatial_shape, ksize, stride, padding, dilation):
    k, s, p, d = _triple(ksize), _triple(stride), _triple(padding), _triple(dilation)
    if k != [2, 2, 2] or s != [2, 2, 2] or p != [0, 0, 0] or d != [1, 1, 1]:
        if k[0] * k[1] * k[2] > 27:
            raise NotImplementedError("doda_amd SparseConv3d supports kernel volumes <= 27, got k=%r" % (k,))
        outids, tbl, tbl_rev, out_shape = _ops.rulebook_conv(indices, spatial_shape, batch_size, k, s, p, d)
        return IndiceData("down2", outids, indices, list(spatial_shape), out_shape, tbl, tbl_rev)
    outids, child, par_off, out_shape = _ops.rulebook_down2(indices, spatial_shape, batch_size)
    return IndiceData("down2", outids, indices, list(spatial_shape), out_shape, child, par_off)


def get_deconv_output_size(input_size, kernel_size, stride, padding, dilation, output_padding):
    """Output shape of a transposed convolution: (in - 1) * stride - 2 * padding + kernel_size + output_padding per axis.
    [MEM] upstream's spconv.ops.get_deconv_output_size, written from memory as in SURVEY §0 (spconv v1.2 is not vendored).  The
    formula ignores dilation: positions a dilated kernel would reach beyond it are dropped by the rulebook builder."""
    out = []
    for i in range(len(input_size)):
        if kernel_size[i] < 1:
            raise ValueError("a transposed convolution needs kernel_size >= 1, got %r" % (kernel_size,))
        out.append((input_size[i] - 1) * stride[i] - 2 * padding[i] + kernel_size[i] + output_padding[i])
    return out


def build_transpose(indices, batch_size, spatial_shape, ksize, stride, padding, dilation, output_padding):
    """Rulebook of SparseConvTranspose3d (doda_rulebook_deconv_*): kind 'transpose', tables in the generic strided layout —
    tbl [K, M_out] (the input row feeding output t through offset o), tbl_rev [K, M_in]."""
    k, s, p, d, op = _triple(ksize), _triple(stride), _triple(padding), _triple(dilation), _triple(output_padding)
    if k[0] * k[1] * k[2] > 27:
        raise NotImplementedError("doda_amd SparseConvTranspose3d supports kernel volumes <= 27, got k=%r" % (k,))
    outids, tbl, tbl_rev, out_shape = _ops.rulebook_deconv(indices, spatial_shape, batch_size, k, s, p, d, op)
    return IndiceData("transpose", outids, indices, list(spatial_shape), out_shape, tbl, tbl_rev)


def get_indice_pairs(indices, batch_size, spatial_shape, ksize=3, stride=1, padding=0, dilation=1,
                     out_padding=0, subm=False, transpose=False, grid=None, use_hash=False):
    """Upstream-shaped entry: returns (outids, indice_pairs [2,K,N], indice_pair_num [K])."""
    if subm:
        data = build_subm(indices, batch_size, spatial_shape, ksize)
    elif transpose:
        data = build_transpose(indices, batch_size, spatial_shape, ksize, stride, padding, dilation, out_padding)
    else:
        data = build_down2(indices, batch_size, spatial_shape, ksize, stride, padding, dilation)
    return data.outids, data.indice_pairs, data.indice_pair_num


TILE_MIN_ROWS = 32768    # finest-level rulebooks of at least this many rows get a tilebook (LDS-staged conv kernel)
TILE_KERNEL = os.environ.get("DODA_NO_TILE", "0") != "1"
# Safety valve: the tile kernel lives on the locality of the voxel order (raster-like scans: ~2-3 x 256 distinct
# neighbour rows per 256-row tile).  If more than TILE_OVERFLOW_MAX of a batch's finest-level tiles exceed the
# staging capacity (they are then served from the dense table inside the tile kernel, slower than the dense
# kernel itself), tilebooks are skipped for the next TILE_BACKOFF batches and probed again afterwards.
TILE_OVERFLOW_MAX = 0.25
TILE_BACKOFF = 64
_tile_state = {"skip": 0, "last": None}   # batches still to skip; (tiles, over 64-byte capacity, over list capacity)
# bf16 training: the SubM rulebooks of the coarser levels up to this one also get a tilebook, for the weight gradient only
# (48 .. 224 channels: csrc/spconv_wwide.hip).  Their overflow does not feed the backoff above: a coarse tile above the
# list capacity is served from the dense table inside that kernel.  0: none (DODA_WGRAD_TILE_LEVELS).
WGRAD_TILE_LEVELS = int(os.environ.get("DODA_WGRAD_TILE_LEVELS", "7"))
PAIRS_MIN_ROWS = 65536   # smaller rulebooks stay on the gather-table kernel: the list export (three launches
#                          per rulebook, issued by a host that is as busy as the GPU) would cost more than it saves
_NEVER, _NO_LIMIT = -1, 1 << 62


def level_policy(n_levels, with_pairs, n_tile_levels, tiles_on):
    """THE decision which SubM rulebook of a pyramid gets a tilebook and which gets pair lists: one (tile_lo, tile_hi,
    pairs_min) row per level, applied by whoever knows the level's row count m (the extension's build_pyramid after its
    read-back, the loop at the end of build_pyramid below).  A tilebook where tile_lo <= m < tile_hi; otherwise pair lists
    where m >= pairs_min; -1 = never.  Strided rulebooks get neither (their lists cost more than they saved).
      * the n_tile_levels finest levels (16 / 32 channels: rows of 32 or 64 bytes, what the tile kernels stage) take a
        tilebook from TILE_MIN_ROWS rows, unless tiles are off (tiles_on False: DODA_NO_TILE=1 or the overflow back-off);
      * bf16 training with tiles: the coarser levels below WGRAD_TILE_LEVELS take one for the weight gradient only
        (csrc/spconv_wwide.hip), whatever tiles_on says (their overflow is served inside the kernel), up to the size from
        which the rulebook gets lists instead — its layers then stay on the pair-list kernel;
      * lists (with_pairs) go to rulebooks of at least PAIRS_MIN_ROWS rows that got no tilebook: with one, every bf16 layer
        takes the tile weight gradient or falls back to the gather table."""
    pairs_min = PAIRS_MIN_ROWS if with_pairs else _NEVER
    wgrad_levels = WGRAD_TILE_LEVELS if (with_pairs and n_tile_levels > 0) else 0
    rows = []
    for k in range(n_levels):
        if k < n_tile_levels:
            tile = (TILE_MIN_ROWS, _NO_LIMIT) if tiles_on else (_NEVER, _NO_LIMIT)
        elif k < wgrad_levels:
            tile = (1, pairs_min)
        else:
            tile = (_NEVER, _NO_LIMIT)
        rows.append(tile + (pairs_min,))
    return rows


def build_pyramid(tensor, n_levels, subm_key="subm%d", down_key="spconv%d", first_level=1, with_pairs=False,
                  with_tiles=None):
    """Build every rulebook of an n-level U-Net up front and store it in `tensor.indice_dict`
    (SubM k3 under subm_key % i, k2s2 under down_key % i), so the convolutions find them cached.
    Rulebooks depend only on the voxel indices; building them before any feature kernel is queued
    means the size read-backs of the strided levels wait on an almost empty stream instead of
    stalling the host in the middle of the forward pass.  with_pairs: also export the pair lists of the SubM
    rulebooks that level_policy gives them to, for the pair-list weight gradient (training with bf16 features)."""
    indices, shape = tensor.indices, tensor.spatial_shape
    # with_tiles: number of finest levels that get a tilebook (True = 2: bf16 rows of 32 / 64 bytes at DODA's
    # widths; 1 for fp32 features); None follows with_pairs (bf16 training)
    n_tile_levels = (2 if with_pairs else 0) if with_tiles is None else (2 if with_tiles is True else int(with_tiles))
    if (_ext is not None and not tensor.indice_dict and indices.is_cuda and indices.dtype == torch.int32
            and indices.shape[0] > 0 and all(int(v) >= 2 for v in shape)):
        tiles_on = TILE_KERNEL and n_tile_levels > 0
        if tiles_on and _tile_state["skip"] > 0:
            _tile_state["skip"] -= 1
            tiles_on = False
        # (one call without the GIL: the builds, their six size read-backs and the tilebook's overflow counters)
        levels, nt, over64, over32 = _ext.build_pyramid_probe(indices, [int(v) for v in shape], int(tensor.batch_size),
                                                              level_policy(int(n_levels), with_pairs, n_tile_levels, tiles_on))
        if tiles_on and nt >= 0:
            _tile_state["last"] = (nt, over64, over32)
            if over32 > TILE_OVERFLOW_MAX * nt:
                _tile_state["skip"] = TILE_BACKOFF
                # this batch too: plain copies of the tables (no tilebook behind them) keep it on the dense kernels
                levels = [((lv[0].clone() if k < n_tile_levels and _ext.has_tilebook(lv[0]) else lv[0]),) + tuple(lv[1:])
                          for k, lv in enumerate(levels)]
        for k, (nbr, outids, child, par_off, oshape, sp, sn, sh) in enumerate(levels):   # sp, sn, sh: lists, counts, segments
            lvl = first_level + k
            data = tensor.indice_dict[subm_key % lvl] = IndiceData("subm", indices, indices, list(shape),
                                                                   list(shape), nbr)
            if sp is not None:
                data._wpairs = (sp, sn, sh)
            if k == len(levels) - 1:
                break
            tensor.indice_dict[down_key % lvl] = IndiceData("down2", outids, indices, list(shape), list(oshape), child, par_off)
            indices, shape = outids, list(oshape)
        return tensor.indice_dict
    # the module-by-module builders make no tilebook: the same policy with tiles off (a record found in place keeps what it has)
    policy = level_policy(int(n_levels), with_pairs, 0, False)
    for lvl, (_, _, pairs_min) in zip(range(first_level, first_level + n_levels), policy):
        key = subm_key % lvl
        if key not in tensor.indice_dict:
            tensor.indice_dict[key] = build_subm(indices, tensor.batch_size, shape, 3)
        if (0 <= pairs_min <= indices.shape[0]
                and not (_ext is not None and _ext.has_tilebook(tensor.indice_dict[key].tbl))):   # (tiled: no consumer)
            tensor.indice_dict[key].wgrad_lists()
        if lvl == first_level + n_levels - 1:
            break
        key = down_key % lvl
        data = tensor.indice_dict.get(key)
        if data is None:
            data = build_down2(indices, tensor.batch_size, shape, 2, 2, 0, 1)
            tensor.indice_dict[key] = data
        indices, shape = data.outids, data.out_spatial_shape
    return tensor.indice_dict

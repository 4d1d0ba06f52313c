"""ctypes binding of libdoda_hip.so: one record in ABIS per header under include/ (the core ABI and its companions) with the
header's signature table, its struct mirrors and its mirrored constants.  tests/test_abi_host.py holds every record to its header.

There is no fallback: if the shared library is missing or lacks a symbol, importing the product
path raises.  PyTorch is used only for device memory and streams; every signature below is
plain pointers + sizes.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdoda_hip.so")

c_i32, c_i64, c_f32, c_sz, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_void_p
c_i32p, c_i64p, c_u64p, c_f64p, c_f64 = C.POINTER(c_i32), C.POINTER(c_i64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_double

# What Python mirrors of one header: header = its file under include/; version_fn / version = its version function and the value
# expected of it (the header's DODA_..._ABI_VERSION); what = its name in the error message; signatures = name -> (restype,
# argtypes) of every function it declares; structs = C name -> ctypes.Structure mirror; constants = name -> value of the module-level
# ints that mirror its `#define DODA_<name>`; unmirrored = its structs that are never passed from Python.
Abi = collections.namedtuple("Abi", "header version_fn version what signatures structs constants unmirrored",
                             defaults=({}, {}, ()))
ABIS = []


def _named(*names):
    return {name: globals()[name] for name in names}


# ---- include/doda_hip.h: the core ABI ----------------------------------------------------------------------------------------
ABI_VERSION = 13
OPT_TILE_KERNEL, OPT_WLDS_KERNEL, OPT_WDMA_KERNEL, OPT_TILE_PIPELINE, OPT_TILE_DUAL, OPT_CONV_UP = 1, 2, 3, 4, 5, 6   # doda_set_option / doda_get_option
OPT_PRE_FWD_ROWS, OPT_PRE_BWD_ROWS = 7, 8   # (row thresholds of doda_layers_run's BatchNorm folding)
STATS_SLOTS = 8
WGRAD_ACCUMULATE = 1
CX_GEMM, CX_BNFWD, CX_BNBWD, CX_STATS = 1, 2, 3, 4
CX_F_BARRIER, CX_F_IDENTITY, CX_F_RELU, CX_F_TRAINING, CX_F_ACCUM = 1, 2, 4, 8, 16


class ConvEpilogue(C.Structure):   # doda_conv_epilogue (ABI 11)
    _fields_ = [("residual", c_vp), ("stats", c_vp), ("stats_rows_h", c_i32p), ("bn_x", c_vp), ("bn_mean", c_vp), ("bn_invstd", c_vp),
                ("bn_gamma", c_vp), ("bn_beta", c_vp), ("bn_relu", c_i32), ("tilebook_rows", c_i32), ("tilebook", c_vp),
                ("residual_bcast", c_i32), ("stats_totals", c_vp),
                ("x_ld", c_i32), ("y_ld", c_i32), ("residual_ld", c_i32), ("bn_x_ld", c_i32),   # ABI 11: row strides
                ("prologue", c_vp)]                                                             # ABI 11: doda_conv_prologue *


class WgradJob(C.Structure):   # doda_wgrad_job (ABI 2)
    _fields_ = [("a", c_vp), ("b", c_vp), ("tbl", c_vp), ("dw", c_vp), ("ca", c_i32), ("cb", c_i32), ("ld", c_i32), ("K", c_i32),
                ("n_rows", c_i32), ("elem_bytes", c_i32), ("pair_in", c_vp), ("pair_out", c_vp), ("pair_num", c_vp),
                ("pair_ld", c_i32), ("n_a", c_i32), ("flags", c_i32), ("reserved", c_i32), ("pair_seg", c_vp), ("pair_seg_nt", c_i32),
                ("reserved2", c_i32), ("tilebook", c_vp)]


class SgdTensor(C.Structure):   # doda_sgd_tensor
    _fields_ = [("p", c_vp), ("g", c_vp), ("buf", c_vp), ("n", c_i64), ("first_step", c_i32), ("reserved", c_i32)]


class CxOp(C.Structure):   # doda_cx_op
    _fields_ = [("kind", c_i32), ("flags", c_i32), ("rows", c_i32), ("rows_in", c_i32), ("c_in", c_i32), ("c_out", c_i32),
                ("K", c_i32), ("tbl_ld", c_i32), ("x_ld", c_i32), ("y_ld", c_i32), ("res_ld", c_i32), ("aux_ld", c_i32),
                ("y2_ld", c_i32), ("n_part", c_i32), ("c_split", c_i32), ("reserved", c_i32), ("eps", c_f32), ("momentum", c_f32),
                ("x", c_vp), ("w", c_vp), ("tbl", c_vp), ("y", c_vp), ("y2", c_vp), ("res", c_vp), ("aux", c_vp), ("stats", c_vp),
                ("stats_b", c_vp), ("gamma", c_vp), ("beta", c_vp), ("mean", c_vp), ("invstd", c_vp), ("running_mean", c_vp),
                ("running_var", c_vp), ("nbt", c_vp), ("dgamma", c_vp), ("dbeta", c_vp), ("tilebook", c_vp)]


# a descriptor of doda_spconv_pack_multi (the header describes it in words; doda_spconv_pack_desc_bytes() = its 48 bytes)
PACK_DESC = np.dtype([("w", "<u8"), ("out", "<u8"), ("K", "<i4"), ("kc", "<i4"), ("nc", "<i4"), ("layout", "<i4"), ("esz", "<i4"),
                      ("n_chunk", "<i4"), ("NB", "<i4"), ("pad", "<i4")])

ABIS.append(Abi("doda_hip.h", "doda_abi_version", ABI_VERSION, "ABI", {
    "doda_abi_version": (c_i32, []),
    "doda_strerror": (C.c_char_p, [c_i32]),
    "doda_voxelize_idx_h": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, C.POINTER(c_vp),
                                    C.POINTER(c_i32), C.POINTER(c_i32)]),
    "doda_voxelize_idx_fill_h": (c_i32, [c_vp, c_vp, c_vp, c_vp]),
    "doda_voxelize_idx_free_h": (None, [c_vp]),
    "doda_voxelize_idx_workspace_bytes": (c_sz, [c_i32]),
    "doda_voxelize_idx_assign": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_voxelize_idx_fill": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp,
                                       c_sz, c_vp]),
    "doda_voxelize_fp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_voxelize_bp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_voxelize_fp_rows": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    "doda_point_recover_fp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "doda_point_recover_bp": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "doda_rulebook_workspace_bytes": (c_sz, [c_i32]),
    "doda_rulebook_workspace_bytes_grid": (c_sz, [c_i32, c_i32, c_vp]),   # ABI 13
    "doda_rulebook_subm": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_sz, c_vp]),
    "doda_rulebook_down2_assign": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_sz, c_vp]),
    "doda_rulebook_down2_tables": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp]),
    "doda_rulebook_conv_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_rulebook_conv_assign": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_sz, c_vp]),
    "doda_rulebook_conv_tables": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp,
                                          c_i32, c_vp, c_i32, c_vp, c_sz, c_vp]),
    "doda_rulebook_subm_generic": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]),
    "doda_rulebook_pairs_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_rulebook_pairs": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_sz,
                                    c_vp]),
    "doda_spconv_gather_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32, c_i32]),
    "doda_spconv_pack_desc_bytes": (c_sz, []),
    "doda_spconv_pack_plan_h": (c_i32, [c_vp, c_i32, c_vp, C.POINTER(c_i32)]),
    "doda_spconv_pack_multi": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp]),
    "doda_rulebook_pairs_tile": (c_i32, []),
    "doda_spconv_wgrad_multi_workspace_bytes": (c_sz, [c_vp, c_i32]),
    "doda_spconv_wgrad_multi_desc_bytes": (c_sz, [c_i32]),
    "doda_spconv_wgrad_multi": (c_i32, [c_vp, c_i32, c_vp, c_sz, c_vp, c_sz, c_vp]),
    "doda_maxpool_fwd_f32": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "doda_maxpool_bwd_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "doda_cross_entropy_workspace_bytes": (c_sz, [c_i32]),
    "doda_seg_meters": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, C.c_int64, c_vp, c_vp]),
    "doda_cross_entropy_fwd": (c_i32, [c_vp, c_vp, c_i32, c_i32, C.c_int64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_cross_entropy_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, C.c_int64, c_vp, c_vp]),
    "doda_tilebook_tile": (c_i32, []),
    "doda_tilebook_umax": (c_i32, []),
    "doda_tilebook_bytes": (c_sz, [c_i32, c_i32]),
    "doda_tilebook_build": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_sz, c_vp]),
    "doda_set_option": (c_i32, [c_i32, c_i32]),
    "doda_get_option": (c_i32, [c_i32]),
    "doda_spconv_stats_capacity": (c_sz, [c_i32]),
    "doda_spconv_gather_ex": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32,
                                      c_i32, c_vp, c_sz, c_vp, c_vp]),
    "doda_bn_relu_fwd_stats": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_bn_relu_bwd_stats": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32,
                                          c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "doda_bn_relu_fwd_totals": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp,
                                        c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_bn_relu_bwd_totals": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32,
                                        c_vp, c_vp, c_vp, c_vp]),
    "doda_bn_relu_bwd_add": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp,
                                        c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_bn_relu_apply": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "doda_bn_fwd_final": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "doda_cast_colsum_blocks": (c_i32, [C.c_int64, c_i32]),
    "doda_cast_colsum_f32_bf16": (c_i32, [c_vp, C.c_int64, c_i32, c_vp, c_vp, c_i32, c_vp]),
    "doda_pad_channels": (c_i32, [c_vp, C.c_int64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "doda_sgd_multi_desc_bytes": (c_sz, [c_i32]),
    "doda_sgd_multi": (c_i32, [c_vp, c_i32, C.c_double, C.c_double, C.c_double, C.c_double, c_i32, c_i32, c_vp,
                               c_sz, c_vp]),
    "doda_bn_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_bn_relu_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                 c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_bn_relu_bwd": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp,
                                 c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_knnquery": (c_i32, [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "doda_knn_batch": (c_i32, [c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "doda_ballquery_workspace_bytes": (c_sz, [c_i32]),
    "doda_ballquery_batch_p": (c_i32, [c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       C.POINTER(c_i32), c_vp, c_sz, c_vp]),
    "doda_layers_run": (c_i32, [c_vp, c_i32, c_i32, C.POINTER(c_i32), c_vp]),
    "doda_head_ce_blocks": (c_i32, [c_i32]),
    "doda_head_dw_blocks": (c_i32, [c_i32]),
    "doda_head_dw_bf16": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp]),
    "doda_head_ce_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, C.c_int64, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "doda_head_ce_bwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, C.c_int64, c_vp, c_vp, c_vp, c_vp,
                                 c_vp, c_i32, c_vp]),
}, structs={"doda_conv_epilogue": ConvEpilogue, "doda_wgrad_job": WgradJob, "doda_sgd_tensor": SgdTensor, "doda_cx_op": CxOp},
    constants=_named("ABI_VERSION", "OPT_TILE_KERNEL", "OPT_WLDS_KERNEL", "OPT_WDMA_KERNEL", "OPT_TILE_PIPELINE", "OPT_TILE_DUAL",
                     "OPT_CONV_UP", "OPT_PRE_FWD_ROWS", "OPT_PRE_BWD_ROWS", "STATS_SLOTS", "WGRAD_ACCUMULATE", "CX_GEMM", "CX_BNFWD",
                     "CX_BNBWD", "CX_STATS", "CX_F_BARRIER", "CX_F_IDENTITY", "CX_F_RELU", "CX_F_TRAINING", "CX_F_ACCUM"),
    unmirrored=("doda_conv_prologue",)))   # (ConvEpilogue.prologue is always null from Python)
EXPORTED_SYMBOLS = tuple(ABIS[0].signatures)   # the core set

# ---- include/doda_selftrain.h: the self-training companion ABI (same library, as every companion below) -------------------------
ST_RADIX_BITS, ST_RADIX_LEVELS, ST_MAX_CLASSES = 8, 4, 32
ABIS.append(Abi("doda_selftrain.h", "doda_st_abi_version", 1, "self-training ABI", {
    "doda_st_abi_version": (c_i32, []),
    "doda_st_voxel_confidence": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "doda_st_point_store": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "doda_st_radix_hist": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "doda_st_label": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
}, constants=_named("ST_RADIX_BITS", "ST_RADIX_LEVELS", "ST_MAX_CLASSES")))

# ---- include/doda_mix.h: cuboid mixing ----------------------------------------------------------------------------------------
MIX_MAX_SEGMENTS, MIX_MAX_CUBOIDS, MIX_MAX_CLASSES, MIX_CHUNK, MIX_FIXED_BITS = 128, 32, 32, 1024, 28
ABIS.append(Abi("doda_mix.h", "doda_mix_abi_version", 1, "cuboid-mixing ABI", {
    "doda_mix_abi_version": (c_i32, []),
    "doda_mix_blocks": (c_i64, [c_i64p, c_i32]),
    "doda_mix_bounds": (c_i32, [c_vp, c_i32, c_i64p, c_i32, c_vp, c_vp, c_vp]),
    "doda_mix_classify": (c_i32, [c_vp, c_vp, c_i64p, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_mix_emit": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                              c_vp]),
    "doda_mix_extract": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
}, constants=_named("MIX_MAX_SEGMENTS", "MIX_MAX_CUBOIDS", "MIX_MAX_CLASSES", "MIX_CHUNK", "MIX_FIXED_BITS")))

# ---- include/doda_aug.h: the augmentation pipeline ----------------------------------------------------------------------------
AUG_MAX_SEGMENTS, AUG_CHUNK, AUG_MAX_GRID_CELLS = 64, 1024, 1 << 24
ABIS.append(Abi("doda_aug.h", "doda_aug_abi_version", 1, "augmentation ABI", {
    "doda_aug_abi_version": (c_i32, []),
    "doda_aug_blocks": (c_i64, [c_i64p, c_i32]),
    "doda_aug_affine": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp]),
    "doda_aug_blur": (c_i32, [c_vp, c_vp, c_i32p, c_i32, c_vp]),
    "doda_aug_displace": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_i32p, c_f64p, c_vp, c_vp, c_vp]),
    "doda_aug_crop": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "doda_aug_emit": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp, c_i32p, c_i64p, c_i32, c_vp,
                              c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
}, constants=_named("AUG_MAX_SEGMENTS", "AUG_CHUNK", "AUG_MAX_GRID_CELLS")))

# ---- include/doda_loss.h: the Lovasz-softmax loss ------------------------------------------------------------------------------
LOVASZ_MAX_CLASSES, LOVASZ_MAX_POINTS_PER_VOXEL = 32, 65535
ABIS.append(Abi("doda_loss.h", "doda_loss_abi_version", 1, "loss ABI", {
    "doda_loss_abi_version": (c_i32, []),
    "doda_lovasz_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_lovasz_blocks": (c_i32, [c_i32]),
    "doda_lovasz_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_sz,
                                c_vp]),
    "doda_lovasz_bwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
}, constants=_named("LOVASZ_MAX_CLASSES", "LOVASZ_MAX_POINTS_PER_VOXEL")))

# ---- include/doda_eval.h: full-cloud evaluation -------------------------------------------------------------------------------
EVAL_MAX_SCENES, EVAL_MAX_CELLS, EVAL_MAX_CLASSES = 32, 1 << 21, 32


class EvalScene(C.Structure):   # doda_eval_scene
    _fields_ = [("n_end", c_i32), ("m_end", c_i32), ("cell_base", c_i32), ("dims", c_i32 * 3), ("origin", c_f32 * 3),
                ("side", c_f32), ("inv_side", c_f32)]


ABIS.append(Abi("doda_eval.h", "doda_eval_abi_version", 1, "evaluation ABI", {
    "doda_eval_abi_version": (c_i32, []),
    "doda_eval_nn": (c_i32, [c_vp, c_vp, c_i64, c_vp, C.POINTER(EvalScene), c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "doda_eval_score_blocks": (c_i32, [c_i64]),
    "doda_eval_score": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp,
                                c_vp, c_i32, c_vp]),
}, structs={"doda_eval_scene": EvalScene}, constants=_named("EVAL_MAX_SCENES", "EVAL_MAX_CELLS", "EVAL_MAX_CLASSES")))

# ---- include/doda_subsample.h: the training subsample --------------------------------------------------------------------------
SUBSAMPLE_MAX_SEGMENTS, SUBSAMPLE_CHUNK = 64, 1024
ABIS.append(Abi("doda_subsample.h", "doda_subsample_abi_version", 1, "subsample ABI", {
    "doda_subsample_abi_version": (c_i32, []),
    "doda_subsample_workspace_bytes": (c_sz, [c_i64p, c_i32]),
    "doda_subsample_draw": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32p, c_u64p, C.c_uint32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                    c_vp, c_sz, c_vp]),
}, constants=_named("SUBSAMPLE_MAX_SEGMENTS", "SUBSAMPLE_CHUNK")))

# ---- include/doda_optim.h: the optimizer step ---------------------------------------------------------------------------------
OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2
OPTIM_TILE, OPTIM_NORM_BLOCKS = 2048, 512


class OptimTensor(C.Structure):   # doda_optim_tensor
    _fields_ = [("p", c_vp), ("g", c_vp), ("state1", c_vp), ("state2", c_vp), ("n", c_i64), ("bias_correction1", c_f64),
                ("bias_correction2_sqrt", c_f64), ("first_step", c_i32), ("reserved", c_i32)]


class OptimHyper(C.Structure):   # doda_optim_hyper
    _fields_ = [("lr", c_f64), ("beta1", c_f64), ("beta2", c_f64), ("eps", c_f64), ("weight_decay", c_f64), ("nesterov", c_i32),
                ("maximize", c_i32)]


ABIS.append(Abi("doda_optim.h", "doda_optim_abi_version", 1, "optimizer ABI", {
    "doda_optim_abi_version": (c_i32, []),
    "doda_optim_workspace_bytes": (c_sz, [c_i32]),
    "doda_optim_step": (c_i32, [C.POINTER(OptimTensor), c_i32, c_i32, C.POINTER(OptimHyper), c_f64, c_vp, c_vp, c_sz, c_vp]),
}, structs={"doda_optim_tensor": OptimTensor, "doda_optim_hyper": OptimHyper},
    constants=_named("OPTIM_SGD", "OPTIM_ADAM", "OPTIM_ADAMW", "OPTIM_TILE", "OPTIM_NORM_BLOCKS")))

# ---- include/doda_pgops.h: clustering, segment pools, proposal IoU -------------------------------------------------------------
PG_WAVE_LIST, PG_LONG_SEGMENT, PG_IOU_LDS_INSTANCES = 64, 2048, 8192
_PG_SEG = (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp])
ABIS.append(Abi("doda_pgops.h", "doda_pgops_abi_version", 1, "PG_OP ABI", {
    "doda_pgops_abi_version": (c_i32, []),
    "doda_pg_components": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "doda_pg_bfs_cluster_h": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32p, c_i32p]),
    "doda_pg_sec_mean": _PG_SEG,
    "doda_pg_sec_min": _PG_SEG,
    "doda_pg_sec_max": _PG_SEG,
    "doda_pg_roipool_fp": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "doda_pg_sec_mean_bp": _PG_SEG,
    "doda_pg_roipool_bp": _PG_SEG,
    "doda_pg_get_iou_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_pg_get_iou": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_sz, c_vp]),
}, constants=_named("PG_WAVE_LIST", "PG_LONG_SEGMENT", "PG_IOU_LDS_INSTANCES")))

# ---- include/doda_pointops.h: the rest of pointops2_cuda (sampling, grouping, interpolation, subtraction, aggregation) ----------
PO_WAVE_LIST, PO_FPS_BLOCK, PO_FPS_REG, PO_FPS_MAX_DIM = 64, 1024, 8, 8
ABIS.append(Abi("doda_pointops.h", "doda_pointops_abi_version", 1, "pointops ABI", {
    "doda_pointops_abi_version": (c_i32, []),
    "doda_po_transpose_workspace_bytes": (c_sz, [c_i32]),
    "doda_po_transpose": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_po_grouping_fwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_grouping_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_interpolation_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_interpolation_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_subtraction_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_subtraction_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_aggregation_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "doda_po_aggregation_bwd": (c_i32, [c_vp] * 10 + [c_i32] * 5 + [c_vp]),
    "doda_po_furthestsampling": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
}, constants=_named("PO_WAVE_LIST", "PO_FPS_BLOCK", "PO_FPS_REG", "PO_FPS_MAX_DIM")))

# ---- include/doda_vss.h: virtual scan simulation --------------------------------------------------------------------------------
VSS_MAX_SEGMENTS, VSS_CHUNK, VSS_MAX_GRID, VSS_EXHAUSTIVE, VSS_KEY_NONE = 64, 1024, 64, 1, 0x7fffffff
ABIS.append(Abi("doda_vss.h", "doda_vss_abi_version", 1, "virtual-scan ABI", {
    "doda_vss_abi_version": (c_i32, []),
    "doda_vss_blocks": (c_i64, [c_i64p, c_i32]),
    "doda_vss_bounds": (c_i32, [c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_vss_image": (c_i32, [c_vp, c_vp, c_i64p, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "doda_vss_view": (c_i32, [c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_vss_flip": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_vp, c_f64p, c_vp, c_vp, c_vp]),
    "doda_vss_extreme": (c_i32, [c_vp, c_vp, c_i32p, c_i32, c_vp, c_f64p, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "doda_vss_count": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_vp, c_vp]),
    "doda_vss_emit": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_vp, c_vp, c_i64p, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                              c_vp]),
}, constants=_named("VSS_MAX_SEGMENTS", "VSS_CHUNK", "VSS_MAX_GRID", "VSS_EXHAUSTIVE", "VSS_KEY_NONE")))

# ---- include/doda_spconv.h: transposed-conv rulebook, max pooling by element size, dense volume <-> rows -----------------------------
SPCONV_MAX_KERNEL_VOLUME, SPCONV_DENSE_CHUNK = 27, 1024
_SP_DENSE = (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp])
ABIS.append(Abi("doda_spconv.h", "doda_spconv_abi_version", 1, "spconv-surface ABI", {
    "doda_spconv_abi_version": (c_i32, []),
    "doda_rulebook_deconv_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_rulebook_deconv_assign": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_rulebook_deconv_tables": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32,
                                            c_vp, c_sz, c_vp]),
    "doda_maxpool_fwd": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "doda_maxpool_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "doda_dense_scatter": _SP_DENSE,
    "doda_dense_gather": _SP_DENSE,
    "doda_from_dense_workspace_bytes": (c_sz, [c_i64]),
    "doda_from_dense_count": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "doda_from_dense_emit": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
}, constants=_named("SPCONV_MAX_KERNEL_VOLUME", "SPCONV_DENSE_CHUNK")))

_lib = None


class DodaNativeError(RuntimeError):
    pass


def lib():
    """The loaded C-ABI library; raises DodaNativeError if it is not built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DodaNativeError(
                "libdoda_hip.so is not built (%s). Run `python -m doda_amd.build` "
                "(hipcc, gfx950). doda_amd has no CPU fallback for its native ops." % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for abi in ABIS:
            for name, (res, args) in abi.signatures.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as e:
                    raise DodaNativeError("libdoda_hip.so lacks symbol %s (stale build?)" % name) from e
                fn.restype = res
                fn.argtypes = args
            if getattr(handle, abi.version_fn)() != abi.version:
                raise DodaNativeError("libdoda_hip.so %s version mismatch" % abi.what)
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().doda_strerror(status).decode()
        raise DodaNativeError("%s failed: %s (%d)" % (what, msg, status))

"""ctypes binding of libdoda_hip.so (include/doda_hip.h and its companions include/doda_selftrain.h, include/doda_mix.h,
include/doda_aug.h, include/doda_loss.h, include/doda_eval.h, include/doda_subsample.h, include/doda_optim.h, include/doda_pgops.h,
include/doda_pointops.h).

There is no fallback: if the shared library is missing or lacks a symbol, importing the product
path raises.  PyTorch is used only for device memory and streams; every signature below is
plain pointers + sizes.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdoda_hip.so")

c_i32, c_i64, c_f32, c_sz, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_void_p

# name -> (restype, argtypes); mirrors include/doda_hip.h one to one
_SIGNATURES = {
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
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# name -> (restype, argtypes); mirrors include/doda_selftrain.h (the self-training companion ABI, same library)
SELFTRAIN_SIGNATURES = {
    "doda_st_abi_version": (c_i32, []),
    "doda_st_voxel_confidence": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "doda_st_point_store": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    "doda_st_radix_hist": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "doda_st_label": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
}
SELFTRAIN_SYMBOLS = tuple(SELFTRAIN_SIGNATURES)
ST_ABI_VERSION = 1  # include/doda_selftrain.h DODA_ST_ABI_VERSION
ST_RADIX_BITS, ST_RADIX_LEVELS, ST_MAX_CLASSES = 8, 4, 32

# name -> (restype, argtypes); mirrors include/doda_mix.h (the cuboid-mixing companion ABI, same library)
c_i64p = C.POINTER(c_i64)
MIX_SIGNATURES = {
    "doda_mix_abi_version": (c_i32, []),
    "doda_mix_blocks": (c_i64, [c_i64p, c_i32]),
    "doda_mix_bounds": (c_i32, [c_vp, c_i32, c_i64p, c_i32, c_vp, c_vp, c_vp]),
    "doda_mix_classify": (c_i32, [c_vp, c_vp, c_i64p, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "doda_mix_emit": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64,
                              c_vp]),
    "doda_mix_extract": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
}
MIX_SYMBOLS = tuple(MIX_SIGNATURES)
MIX_ABI_VERSION = 1  # include/doda_mix.h DODA_MIX_ABI_VERSION
MIX_MAX_SEGMENTS, MIX_MAX_CUBOIDS, MIX_MAX_CLASSES, MIX_CHUNK, MIX_FIXED_BITS = 128, 32, 32, 1024, 28

# name -> (restype, argtypes); mirrors include/doda_aug.h (the augmentation-pipeline companion ABI, same library)
c_i32p, c_f64p, c_f64 = C.POINTER(c_i32), C.POINTER(C.c_double), C.c_double
AUG_SIGNATURES = {
    "doda_aug_abi_version": (c_i32, []),
    "doda_aug_blocks": (c_i64, [c_i64p, c_i32]),
    "doda_aug_affine": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp]),
    "doda_aug_blur": (c_i32, [c_vp, c_vp, c_i32p, c_i32, c_vp]),
    "doda_aug_displace": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_i32p, c_f64p, c_vp, c_vp, c_vp]),
    "doda_aug_crop": (c_i32, [c_vp, c_i64p, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "doda_aug_emit": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp, c_i32p, c_i64p, c_i32, c_vp,
                              c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
}
AUG_SYMBOLS = tuple(AUG_SIGNATURES)
AUG_ABI_VERSION = 1  # include/doda_aug.h DODA_AUG_ABI_VERSION
AUG_MAX_SEGMENTS, AUG_CHUNK, AUG_MAX_GRID_CELLS = 64, 1024, 1 << 24

# name -> (restype, argtypes); mirrors include/doda_loss.h (the Lovasz-softmax companion ABI, same library)
LOSS_SIGNATURES = {
    "doda_loss_abi_version": (c_i32, []),
    "doda_lovasz_workspace_bytes": (c_sz, [c_i32, c_i32]),
    "doda_lovasz_blocks": (c_i32, [c_i32]),
    "doda_lovasz_fwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_sz,
                                c_vp]),
    "doda_lovasz_bwd": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
}
LOSS_SYMBOLS = tuple(LOSS_SIGNATURES)
LOSS_ABI_VERSION = 1  # include/doda_loss.h DODA_LOSS_ABI_VERSION
LOVASZ_MAX_CLASSES, LOVASZ_MAX_POINTS_PER_VOXEL = 32, 65535


# name -> (restype, argtypes); mirrors include/doda_eval.h (the full-cloud evaluation companion ABI, same library)
class EvalScene(C.Structure):   # doda_eval_scene
    _fields_ = [("n_end", c_i32), ("m_end", c_i32), ("cell_base", c_i32), ("dims", c_i32 * 3), ("origin", c_f32 * 3),
                ("side", c_f32), ("inv_side", c_f32)]


EVAL_SIGNATURES = {
    "doda_eval_abi_version": (c_i32, []),
    "doda_eval_nn": (c_i32, [c_vp, c_vp, c_i64, c_vp, C.POINTER(EvalScene), c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "doda_eval_score_blocks": (c_i32, [c_i64]),
    "doda_eval_score": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp,
                                c_vp, c_i32, c_vp]),
}
EVAL_SYMBOLS = tuple(EVAL_SIGNATURES)
EVAL_ABI_VERSION = 1  # include/doda_eval.h DODA_EVAL_ABI_VERSION
EVAL_MAX_SCENES, EVAL_MAX_CELLS, EVAL_MAX_CLASSES = 32, 1 << 21, 32

# name -> (restype, argtypes); mirrors include/doda_subsample.h (the training-subsample companion ABI, same library)
c_u64p = C.POINTER(C.c_uint64)
SUBSAMPLE_SIGNATURES = {
    "doda_subsample_abi_version": (c_i32, []),
    "doda_subsample_workspace_bytes": (c_sz, [c_i64p, c_i32]),
    "doda_subsample_draw": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i64p, c_i32, c_i32p, c_u64p, C.c_uint32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                    c_vp, c_sz, c_vp]),
}
SUBSAMPLE_SYMBOLS = tuple(SUBSAMPLE_SIGNATURES)
SUBSAMPLE_ABI_VERSION = 1  # include/doda_subsample.h DODA_SUBSAMPLE_ABI_VERSION
SUBSAMPLE_MAX_SEGMENTS, SUBSAMPLE_CHUNK = 64, 1024

# name -> (restype, argtypes); mirrors include/doda_optim.h (the optimizer-step companion ABI, same library)
class OptimTensor(C.Structure):   # doda_optim_tensor
    _fields_ = [("p", c_vp), ("g", c_vp), ("state1", c_vp), ("state2", c_vp), ("n", c_i64), ("bias_correction1", c_f64),
                ("bias_correction2_sqrt", c_f64), ("first_step", c_i32), ("reserved", c_i32)]


class OptimHyper(C.Structure):   # doda_optim_hyper
    _fields_ = [("lr", c_f64), ("beta1", c_f64), ("beta2", c_f64), ("eps", c_f64), ("weight_decay", c_f64), ("nesterov", c_i32),
                ("maximize", c_i32)]


OPTIM_SIGNATURES = {
    "doda_optim_abi_version": (c_i32, []),
    "doda_optim_workspace_bytes": (c_sz, [c_i32]),
    "doda_optim_step": (c_i32, [C.POINTER(OptimTensor), c_i32, c_i32, C.POINTER(OptimHyper), c_f64, c_vp, c_vp, c_sz, c_vp]),
}
OPTIM_SYMBOLS = tuple(OPTIM_SIGNATURES)
OPTIM_ABI_VERSION = 1  # include/doda_optim.h DODA_OPTIM_ABI_VERSION
OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2
OPTIM_TILE, OPTIM_NORM_BLOCKS = 2048, 512

# name -> (restype, argtypes); mirrors include/doda_pgops.h (the clustering / segment-pool / proposal-IoU companion ABI, same library)
_PG_SEG = (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp])
PGOPS_SIGNATURES = {
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
}
PGOPS_SYMBOLS = tuple(PGOPS_SIGNATURES)
PGOPS_ABI_VERSION = 1  # include/doda_pgops.h DODA_PGOPS_ABI_VERSION
PG_WAVE_LIST, PG_LONG_SEGMENT, PG_IOU_LDS_INSTANCES = 64, 2048, 8192

# name -> (restype, argtypes); mirrors include/doda_pointops.h (the rest of pointops2_cuda: sampling, grouping, interpolation,
# subtraction, aggregation; same library)
POINTOPS_SIGNATURES = {
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
}
POINTOPS_SYMBOLS = tuple(POINTOPS_SIGNATURES)
POINTOPS_ABI_VERSION = 1  # include/doda_pointops.h DODA_POINTOPS_ABI_VERSION
PO_WAVE_LIST, PO_FPS_BLOCK, PO_FPS_REG, PO_FPS_MAX_DIM = 64, 1024, 8, 8
OPT_TILE_KERNEL, OPT_WLDS_KERNEL, OPT_WDMA_KERNEL, OPT_TILE_PIPELINE, OPT_TILE_DUAL, OPT_CONV_UP = 1, 2, 3, 4, 5, 6   # doda_set_option / doda_get_option
OPT_PRE_FWD_ROWS, OPT_PRE_BWD_ROWS = 7, 8   # (row thresholds of doda_layers_run's BatchNorm folding)
ABI_VERSION = 12  # include/doda_hip.h DODA_ABI_VERSION

# the core ABI and its companions: (signature table, version symbol, expected version, name for the error)
_ABIS = ((_SIGNATURES, "doda_abi_version", ABI_VERSION, "ABI"),
         (SELFTRAIN_SIGNATURES, "doda_st_abi_version", ST_ABI_VERSION, "self-training ABI"),
         (MIX_SIGNATURES, "doda_mix_abi_version", MIX_ABI_VERSION, "cuboid-mixing ABI"),
         (AUG_SIGNATURES, "doda_aug_abi_version", AUG_ABI_VERSION, "augmentation ABI"),
         (LOSS_SIGNATURES, "doda_loss_abi_version", LOSS_ABI_VERSION, "loss ABI"),
         (EVAL_SIGNATURES, "doda_eval_abi_version", EVAL_ABI_VERSION, "evaluation ABI"),
         (SUBSAMPLE_SIGNATURES, "doda_subsample_abi_version", SUBSAMPLE_ABI_VERSION, "subsample ABI"),
         (OPTIM_SIGNATURES, "doda_optim_abi_version", OPTIM_ABI_VERSION, "optimizer ABI"),
         (PGOPS_SIGNATURES, "doda_pgops_abi_version", PGOPS_ABI_VERSION, "PG_OP ABI"),
         (POINTOPS_SIGNATURES, "doda_pointops_abi_version", POINTOPS_ABI_VERSION, "pointops ABI"))

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
        for table, version_fn, version, what in _ABIS:
            for name, (res, args) in table.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as e:
                    raise DodaNativeError("libdoda_hip.so lacks symbol %s (stale build?)" % name) from e
                fn.restype = res
                fn.argtypes = args
            if getattr(handle, version_fn)() != version:
                raise DodaNativeError("libdoda_hip.so %s version mismatch" % what)
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().doda_strerror(status).decode()
        raise DodaNativeError("%s failed: %s (%d)" % (what, msg, status))

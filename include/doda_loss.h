/*
 * doda_loss.h — companion C ABI of libdoda_hip.so: the Lovasz-softmax loss of OPTIMIZATION.loss: lovasz (reference
 * model/unet.py:109-111, util/loss_utils.py lovasz_softmax_with_logit, util/lovasz_loss.py lovasz_softmax with
 * classes='present') fused with the Linear head at VOXEL level.
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device
 * pointers + sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; the number
 * of present classes stays on the device (out[1]).  The core header's surface (ABI 12) and the other companions are unchanged;
 * this header carries its own version, DODA_LOSS_ABI_VERSION, and the same library exports all.
 *
 * All points of a voxel share the voxel's logits (model/unet.py:62-64), so for class c a voxel v contributes two error values:
 * 1 - p[v,c] for its nfg[v,c] valid points labelled c and p[v,c] for its other nvalid[v] - nfg[v,c] valid points.  The Lovasz
 * gradient of a run of tied errors telescopes to J(after the run) - J(before the run), J = 1 - (G - cumfg) / (G + cumbg), G = the
 * valid points labelled c.  Loss and gradient are therefore those of a WEIGHTED sort of 2 m items per class (voxel, fg | bg) with
 * integer weights; the [points, classes] matrix is never built.  Per class: a stable three-pass radix sort (10 bits each) of the
 * keys 0x3f800000 - bits(error) — errors lie in [0, 1], so their fp32 bit patterns order as integers below 2^30 —, exact integer
 * prefix sums of the weights in sorted order, J in fp64, the class loss sum error * (J_after - J_before) in fp64 in a fixed
 * order, loss = the mean over the classes with G > 0.  A repeated call returns the same bits.
 *
 * Deviation from the reference: when every point is ignored (or m = 0) the reference returns an empty [0, C] tensor that cannot
 * be back-propagated; here the loss is 0 and every gradient is 0.
 */
#ifndef DODA_LOSS_H
#define DODA_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_LOSS_ABI_VERSION 1

#define DODA_LOVASZ_MAX_CLASSES 32
#define DODA_LOVASZ_MAX_POINTS_PER_VOXEL 65535   /* v2p_ld - 1: the item weights are 16-bit */

int32_t doda_loss_abi_version(void);

/* Bytes of doda_lovasz_fwd's workspace for m voxels and n_cls classes (the two key / item buffers of the sort, the item weights,
 * the radix histograms and the per-tile partials); 0 when the sizes are outside the range (2 m n_cls must stay below 2^31). */
size_t doda_lovasz_workspace_bytes(int32_t m, int32_t n_cls);

/* Workgroups of doda_lovasz_bwd = rows of its db_partial. */
int32_t doda_lovasz_blocks(int32_t m);

/* The inputs of doda_head_ce_fwd: feats [m, 16] bf16 (elem_bytes 2) or fp32 (4); weight fp32 [n_cls, 16] (rounded to bf16 first for
 * bf16 features), bias fp32 [n_cls] or NULL, 2 <= n_cls <= DODA_LOVASZ_MAX_CLASSES; v2p int32 [m, v2p_ld] = (count, point ids ...);
 * labels int64 [points]; a point counts when its label is not ignore_index and lies in [0, n_cls).
 * out fp32 [2] = {loss, number of present classes}; pred int32 [m] (or NULL) = argmax_k z_v[k], bit-identical to doda_head_ce_fwd's;
 * gitem fp32 [m, n_cls, 2] (or NULL: forward only) = per (voxel, class) the Lovasz gradient J_after - J_before of its bg item
 * ([..., 0], error p) and its fg item ([..., 1], error 1 - p), the operand of doda_lovasz_bwd.
 * ws: doda_lovasz_workspace_bytes(m, n_cls) bytes, 256-byte aligned. */
int doda_lovasz_fwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias, int32_t n_cls,
                    const int32_t *v2p, int32_t v2p_ld, const int64_t *labels, int64_t ignore_index, float *out, int32_t *pred,
                    float *gitem, void *ws, size_t ws_bytes, doda_stream_t stream);

/* dL/dp[v,c] = (gitem[v,c,0] - gitem[v,c,1]) / out[1];  dz_v = grad[0] * p_v * (dp_v - <p_v, dp_v>)  (softmax recomputed from the
 * features with the forward's bits);  d_feats [m, 16] = dz W and dz [m, n_cls], both in the features' type and in the layout
 * doda_head_ce_bwd writes (dz: the operand of doda_head_dw_bf16);  dz_lo [m, n_cls] bf16 (bf16 features only; or NULL) =
 * bf16(dz_fp32 - dz): a second operand for doda_head_dw_bf16 whose result, added to the first, takes the rounding of dz out of
 * dW (up to 2^-8 of a contribution, which shows where few voxels carry a weight's gradient);  db_partial fp32 [n_blocks, n_cls] = per-workgroup column sums
 * of dz, n_blocks = doda_lovasz_blocks(m).  out[1] = 0 (nothing valid): every gradient is 0. */
int doda_lovasz_bwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias, int32_t n_cls,
                    const float *gitem, const float *out, const float *grad, void *d_feats, void *dz, void *dz_lo,
                    float *db_partial, int32_t n_blocks, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_LOSS_H */

/*
 * doda_aug.h — companion C ABI of libdoda_hip.so: the per-sample augmentation pipeline DATA_AUG.aug_list = [scene_aug, elastic,
 * crop] (reference dataset/augmentor/data_augmentor.py:171-230, dataset/augmentor/augmentor_utils.py:61-104,449-472).
 *
 * Same conventions as doda_hip.h / doda_mix.h (whose error codes and doda_strerror these entry points use): extern "C", plain
 * device pointers + sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises;
 * argument errors come back as statuses without a launch.  The core header's surface (ABI 12), doda_selftrain.h and doda_mix.h
 * (version 1 each) are unchanged; this header carries its own version, DODA_AUG_ABI_VERSION, and the same library exports all.
 *
 * Every kernel takes a BATCH OF SEGMENTS, as doda_mix.h does: the scenes of a batch concatenated into one array, with the
 * n_seg + 1 segment offsets given on the HOST (int64, offsets_h[0] = 0, non-decreasing, at most 2^31 - 1 points,
 * 1 <= n_seg <= DODA_AUG_MAX_SEGMENTS), validated before a launch and passed as launch arguments.  A segment is cut into
 * chunks of DODA_AUG_CHUNK points, one workgroup each; doda_aug_blocks() sizes the per-chunk scratch arrays.
 *
 * The coordinate path is fp64: `pos` fp64 [N][3] holds the reference's data_dict['xyz'] (voxel units) from the affine step to the
 * emit step.  Every random decision (the matrix, the grid shapes, the noise, the crop offsets) is made on the host
 * (doda_amd.aug) in the reference's arithmetic and draw order; the host reads back 48 bytes per segment after the affine and
 * after each displace call, and 4 bytes per segment after a crop call.
 */
#ifndef DODA_AUG_H
#define DODA_AUG_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_AUG_ABI_VERSION 1

#define DODA_AUG_MAX_SEGMENTS 64
#define DODA_AUG_CHUNK 1024             /* points per workgroup */
#define DODA_AUG_MAX_GRID_CELLS (1 << 24) /* cells of one noise grid (one of the three of a segment) */

int32_t doda_aug_abi_version(void);

/* Chunks (workgroups) of a batch of segments: sum over segments of ceil(points / DODA_AUG_CHUNK); -1 for invalid offsets. */
int64_t doda_aug_blocks(const int64_t *offsets_h, int32_t n_seg);

/* scene_aug's matmul and elastic's first line (augmentor_utils.py:103, data_augmentor.py:172): per point i of segment s
 *     mid = xyz[i] @ mat[s]        (fp64: (x0 * m0k + x1 * m1k) + x2 * m2k, the fp32 point widened)
 *     pos[i] = mid * scale
 * mat fp64 [n_seg][3][3] (row-major, device).  bounds fp64 [n_seg][2][3] = per segment (min pos, max pos), exact (abs(pos).max is
 * max(-min, max)); part: scratch fp64 [doda_aug_blocks][6].  An empty segment gets (+inf, -inf). */
int doda_aug_affine(const float *xyz, const int64_t *offsets_h, int32_t n_seg, const double *mat, double scale, double *pos,
                    double *part, double *bounds, doda_stream_t stream);

/* The six box blurs of augmentor_utils.py:62-73 over the noise grids of a batch.  Segment s owns three grids of
 * bb_h[s][0] x bb_h[s][1] x bb_h[s][2] fp32 cells (C order), contiguous from cell 3 * (sum of earlier segments' cells) of
 * `noise`; bb_h int32 [n_seg][3] on the HOST (a segment with bb = 0 0 0 has no grid).  Passes along axes 0, 1, 2, 0, 1, 2; per
 * pass out = (float)(((0 + (double)in[-1] * w) + (double)in[0] * w) + (double)in[+1] * w), w = (double)(1.f / 3.f), cells outside
 * the grid being 0 — scipy.ndimage.convolve(mode='constant') on fp32 input.  The result is in `noise`; tmp: scratch of the same
 * size. */
int doda_aug_blur(float *noise, float *tmp, const int32_t *bb_h, int32_t n_seg, doda_stream_t stream);

/* One elastic pass (augmentor_utils.py:74-80) on the segments with a grid (bb_h[s][0] > 0; the others are left alone and get no
 * bounds): pos[i] += g(pos[i]) * mag, g = the trilinear interpolation of the segment's three blurred grids on the axes
 * -(b-1) gran, ..., (b-1) gran (step 2 gran; 0 outside), evaluated as scipy's RegularGridInterpolator does (weights
 * ((1 * w0) * w1) * w2, corners summed with the last axis fastest).  gran_mag_h fp64 [n_seg][2] on the HOST.  bounds / part as
 * doda_aug_affine. */
int doda_aug_displace(double *pos, const int64_t *offsets_h, int32_t n_seg, const float *noise, const int32_t *bb_h,
                      const double *gran_mag_h, double *part, double *bounds, doda_stream_t stream);

/* One validity test of augmentor_utils.crop (:463 and :468-469) on the segments with par[s][9] != 0:
 *     q = (pos[i] - par[s][0..2]) + par[s][3..5]           (xyz - xyz.min(0), then + offset)
 *     t = all(q >= 0) && all(q < par[s][6..8])
 *     valid[i] = par[s][9] > 1 ? t : valid[i] && t          (2: the first test of a segment; 1: a further one)
 * par fp64 [n_seg][10] (device).  count int32 [n_seg], ADDED to (integer atomics; the caller zeroes it): valid points per tested
 * segment.  blk_cnt int32 [doda_aug_blocks]: valid points per chunk of the tested segments, written. */
int doda_aug_crop(const double *pos, const int64_t *offsets_h, int32_t n_seg, const double *par, uint8_t *valid, int32_t *count,
                  int32_t *blk_cnt, doda_stream_t stream);

/* The sample as the loader hands it on, valid points only and in their order (stable compaction): per segment s from output row
 * out_base_h[s] (int64 [n_seg], HOST)
 *     out_locs int32 [M][4]  = (batch0 + s, trunc((pos[i] - par[s][0..2]) + par[s][3..5]))        par fp64 [n_seg][10] as above
 *     out_float fp32 [M][3]  = (float)(feat_scale != 0 ? pos[i] / feat_scale : xyz[i] @ mat[s])   (elastic.apply_to_feat / not)
 *     out_labels int32 [M]   = labels[i];   out_mask1 / out_mask2 uint8 [M] = mask1[i] / mask2[i] (each pair NULL or not)
 * valid / blk_cnt: as doda_aug_crop left them, read for the segments with seg_valid_h[s] != 0 (int32 [n_seg], HOST); the other
 * segments are written whole; both may be NULL when no segment was tested.  top int32 [3], atomicMax'ed (the caller zeroes it):
 * the largest coordinate written + 1 per axis.  Rows at or beyond out_len are not written. */
int doda_aug_emit(const float *xyz, const double *pos, const int32_t *labels, const uint8_t *mask1, const uint8_t *mask2,
                  const int64_t *offsets_h, int32_t n_seg, const double *mat, double feat_scale, const double *par,
                  const uint8_t *valid, const int32_t *blk_cnt, const int32_t *seg_valid_h, const int64_t *out_base_h, int32_t batch0,
                  int32_t *out_locs, float *out_float, int32_t *out_labels, uint8_t *out_mask1, uint8_t *out_mask2, int32_t *top,
                  int64_t out_len, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_AUG_H */

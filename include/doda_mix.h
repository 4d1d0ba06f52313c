/*
 * doda_mix.h — companion C ABI of libdoda_hip.so: tail-aware cuboid mixing (TACM) of the self-training stage
 * (reference dataset/augmentor/augmentor_utils.py:255-445, dataset/mix_dataset.py:59-82).
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device
 * pointers + sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; argument
 * errors come back as statuses without a launch.  The core header's surface (ABI 12) and doda_selftrain.h (version 1) are
 * unchanged; this header carries its own version, DODA_MIX_ABI_VERSION, and the same library exports all three.
 *
 * Every kernel takes a BATCH OF SEGMENTS: the point clouds of a batch (its B target scenes and B source scenes, or a list of
 * queue cuboids) concatenated into one array, with the n_seg + 1 segment offsets given on the HOST (int64, offsets_h[0] = 0,
 * non-decreasing, at most 2^31 - 1 points, 1 <= n_seg <= DODA_MIX_MAX_SEGMENTS).  The offsets travel to the kernels as launch
 * arguments and are validated before a launch, so no kernel trusts a device-side table for its bounds.  A segment is cut into
 * chunks of DODA_MIX_CHUNK points, one workgroup each; doda_mix_blocks() is the number of chunks of a batch, which sizes the
 * per-chunk scratch arrays below.
 *
 * A batch of 2 B segments is mixed by a fixed handful of launches: bounds (2), classify (1), emit (1, plus 1 when queue
 * cuboids take part), extract (1, plus the bounds of the extracted cuboids), with two small host read-backs between them (the
 * bounds, 24 bytes per segment, and the per-cuboid statistics): the cuboid planes and the mixing plan are drawn on the host
 * (doda_amd.tacm.plan).
 */
#ifndef DODA_MIX_H
#define DODA_MIX_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_MIX_ABI_VERSION 1

#define DODA_MIX_MAX_SEGMENTS 128
#define DODA_MIX_MAX_CUBOIDS 32     /* split[0] * split[1] * split[2] */
#define DODA_MIX_MAX_CLASSES 32
#define DODA_MIX_CHUNK 1024         /* points per workgroup */
#define DODA_MIX_FIXED_BITS 28      /* coordinate sums: int64 sums of round(x * 2^28) — exact integer adds, any order */

int32_t doda_mix_abi_version(void);

/* Chunks (workgroups) of a batch of segments: sum over segments of ceil(points / DODA_MIX_CHUNK); -1 for offsets that are not
 * valid (see above). */
int64_t doda_mix_blocks(const int64_t *offsets_h, int32_t n_seg);

/* Replaces xyz.min(0), xyz.max(0) of augmentor_utils.py:259-260,424 (and _split[..., 0:3].max(0) of :326 for queue cuboids):
 * bounds fp32 [n_seg][2][3] = per segment (min xyz, max xyz), exact.  xyz: fp32 rows of `stride` floats (3, or 4 for the
 * (xyz, label) rows of queue cuboids).  part: scratch fp32 [doda_mix_blocks][6] (per-chunk partial results; a second tiny
 * launch combines them).  An empty segment gets (+inf, -inf). */
int doda_mix_bounds(const float *xyz, int32_t stride, const int64_t *offsets_h, int32_t n_seg, float *part, float *bounds,
                    doda_stream_t stream);

/* Replaces get_split_idx / xyz_idx_in_split (augmentor_utils.py:368-384,444-445) and the centring of :259-260.  Per point i of
 * segment s: x = xyz[i] - centre[s] (fp32 subtraction, as the reference's in-place one); cub[i] = the LAST cuboid q < n_cub with
 * (double)x < hi[s][q] && (double)x >= lo[s][q] on all three axes (planes fp64 [n_seg][n_cub][2][3]: hi, lo = hi - range, both
 * made by the host), or 255 when no cuboid holds it.  stats int64 [n_seg][n_cub + 1][3 + n_classes + 1], ADDED to: per (segment,
 * cuboid; row n_cub = points of no cuboid) the sums of round(x * 2^DODA_MIX_FIXED_BITS) per axis, then the histogram of the
 * labels (bin n_classes: labels outside [0, n_classes)).  blk_cnt int32 [doda_mix_blocks][n_cub + 1]: points per (chunk, cuboid),
 * written; doda_mix_emit / doda_mix_extract place their output rows with it.
 * 1 <= n_cub <= DODA_MIX_MAX_CUBOIDS, 1 <= n_classes <= DODA_MIX_MAX_CLASSES. */
int doda_mix_classify(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, const float *centre,
                      const double *planes, int32_t n_cub, int32_t n_classes, uint8_t *cub, int64_t *stats, int32_t *blk_cnt,
                      doda_stream_t stream);

/* Replaces the mixing loop and the concatenation of augmentor_utils.py:321-358 (with transform_xyz, :414-418).  Per segment s,
 * the points whose cuboid c has tab[s][c][0] != 0 are written, IN THEIR ORDER (stable compaction), to rows seg_tab[s][3] +
 * 0, 1, ... of the outputs:
 *     x = xyz[i] - centre[s]                       (fp32; skipped when centre is NULL)
 *     x = (float)((double)x + tab[s][c][1..3])     (the cuboid's move to its slot, :334 / :326)
 *     x = (float)((double)x + tab[s][c][4..6])     (-0.1 * the moved cuboid's mean, :416-417)
 *     x = (float)((double)x - seg_tab[s][0..2])    (the mean of the whole mixed sample, :352)
 * out_labels = labels[i] (or, labels NULL and stride 4, (int)xyz[i][3]); mask1 = seg_tab[s][4] != 0, mask2 = !mask1 (:357-358).
 * tab fp64 [n_seg][n_cub + 1][7] (column n_cub: the points of no cuboid), seg_tab fp64 [n_seg][5].
 * cub / blk_cnt: doda_mix_classify's outputs for the same xyz and offsets — or both NULL with n_cub = 0: every segment is one
 * cuboid, all of it written (queue cuboids).  Rows at or beyond out_len are not written. */
int doda_mix_emit(const float *xyz, int32_t stride, const int32_t *labels, const uint8_t *cub, const int32_t *blk_cnt,
                  const int64_t *offsets_h, int32_t n_seg, int32_t n_cub, const float *centre, const double *tab,
                  const double *seg_tab, float *out_xyz, int32_t *out_labels, uint8_t *mask1, uint8_t *mask2, int64_t out_len,
                  doda_stream_t stream);

/* Replaces np.concatenate((xyz[xyz_idx_s], label[xyz_idx_s].reshape(-1, 1)), axis=-1) of augmentor_utils.py:381: the centred,
 * unmixed points of cuboid c of segment s, in their order, as fp32 rows (x, y, z, label) from row ex_base[s][c] of out_rows on
 * (ex_base int64 [n_seg][n_cub + 1]; negative: the cuboid is not wanted).  Rows at or beyond out_len are not written. */
int doda_mix_extract(const float *xyz, const int32_t *labels, const uint8_t *cub, const int32_t *blk_cnt, const int64_t *offsets_h,
                     int32_t n_seg, int32_t n_cub, const float *centre, const int64_t *ex_base, float *out_rows, int64_t out_len,
                     doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_MIX_H */

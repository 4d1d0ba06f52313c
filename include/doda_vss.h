/*
 * doda_vss.h — companion C ABI of libdoda_hip.so: virtual scan simulation, DATA_AUG.aug_list's `vss` (reference
 * dataset/augmentor/augmentor_utils.py:108-251): per view a range mask, then open3d's hidden point removal — a point is kept iff
 * its spherical flip is a vertex of the convex hull of the flipped points and the camera — and at the end a uniform jitter.
 *
 * Same conventions as doda_aug.h / doda_mix.h (whose error codes and doda_strerror these entry points use): extern "C", plain
 * device pointers + sizes, an explicit HIP stream, an int status; nothing here allocates device memory or synchronises.  A batch
 * is SEGMENTS of one array: n_seg + 1 offsets on the HOST (int64, offsets_h[0] = 0, non-decreasing, at most 2^31 - 1 points,
 * 1 <= n_seg <= DODA_VSS_MAX_SEGMENTS), validated before a launch; a segment is cut into chunks of DODA_VSS_CHUNK points, one
 * workgroup each.  Inputs are fp32 xyz [N][3] (metres, z up) and int32 labels [N]; all geometry is fp64 in the reference's order
 * of operations.  No float atomics: every result is bit-reproducible.  The host (doda_amd.vss) draws every random number and
 * makes every decision from a few bytes per segment.
 *
 * The hull-vertex decision (doda_vss_extreme).  p_i is a vertex iff some direction u has u.(p_i - p_j) > 0 for every other
 * flipped point j and u.p_i > 0 (the camera is the origin).  With ph = p_i / |p_i| and (e1, e2) a basis of its tangent plane,
 * u = ph + t1 e1 + t2 e2 is no restriction, and the decision is the feasibility of the 2-D linear program
 *     -(E d_j) . t <= ph . d_j,   d_j = p_i - p_j,   for all j,
 * solved per query point by one wavefront with Seidel's incremental algorithm inside a box |t1|, |t2| <= half.  A point whose
 * flipped coordinates equal those of a point with a lower index is dropped (qhull reports one vertex per location).
 */
#ifndef DODA_VSS_H
#define DODA_VSS_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_VSS_ABI_VERSION 1

#define DODA_VSS_MAX_SEGMENTS 64
#define DODA_VSS_CHUNK 1024            /* points per workgroup */
#define DODA_VSS_MAX_GRID 64           /* direction cells per axis */
#define DODA_VSS_EXHAUSTIVE 1          /* doda_vss_extreme flag: every query against all points of its segment */
#define DODA_VSS_KEY_NONE 0x7fffffff   /* doda_vss_flip's key of a point outside the view */

int32_t doda_vss_abi_version(void);

/* Chunks (workgroups) of a batch of segments; -1 for invalid offsets. */
int64_t doda_vss_blocks(const int64_t *offsets_h, int32_t n_seg);

/* Per segment over the points with labels[i] != ignore_label: bounds fp32 [n_seg][2][3] = (min xyz, max xyz) ((+inf, -inf) when
 * there is none) and count int32 [n_seg], ADDED to (integer atomics; the caller zeroes it).  part: scratch fp32
 * [doda_vss_blocks][6]. */
int doda_vss_bounds(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                    float *part, float *bounds, int32_t *count, doda_stream_t stream);

/* The two occupancy planes of get_camera_candidate_locations (:178-198).  frame fp64 [n_seg][8] (device) per segment:
 * (c0, c1, c2, vmin0, vmin1, H, W, base); H = 0: the segment is skipped.  A point with labels[i] != ignore_label has the cell
 * (r, c) = trunc(((double)xyz - c) * 10 - vmin) + 1 of an H x W image; img[base + r * W + c] = 1 (a point), and
 * img[base + H * W + r * W + c] = 1 when its label is neither floor_label nor ceiling_label (ceiling_label < 0: no such class).
 * Cells outside the image are not written.  The caller zeroes img. */
int doda_vss_image(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                   int32_t floor_label, int32_t ceiling_label, const double *frame, uint8_t *img, int64_t img_len,
                   doda_stream_t stream);

/* The view-range mask of one (camera, interest point) pair per segment (:216-251).  view fp64 [n_seg][16] (device):
 *   [0..2] c (the frame: _xyz = (double)xyz - c)   [3..5] interest point   [6..8] camera_f = camera - interest
 *   [9] mode: < 0 the segment has no view (its mask is cleared), 0 constant z bounds (fixed, parallel), 1 perspective
 *   [10] camera_f[0]^2 + camera_f[1]^2   [11] z_upper   [12] z_lower   [13] sqrt([10])   [14] tan(pitch + a/2)   [15] tan(pitch - a/2)
 * With f = ((double)xyz - c) - interest:  mask = label != ignore && f0 * cam0 + f1 * cam1 <= [10] && f2 < zu && f2 > zl, where
 * (zu, zl) = ([11], [12]) in mode 0 and (([13] - (f0 * cam0 + f1 * cam1) / [13]) * [14 | 15]) + cam2 in mode 1.
 * mask uint8 [N] written; count int32 [n_seg] ADDED to (the caller zeroes it). */
int doda_vss_view(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                  const double *view, uint8_t *mask, int32_t *count, doda_stream_t stream);

/* The spherical flip of the masked points (open3d hidden_point_removal): q = f - camera_f, n = |q| (0 replaced by 1e-4),
 * flipped[i] = q + 2 * (radius - n) * q / n (fp64 [N][3]; rows outside the mask are not written), and the direction-cell key
 * key[i] = key_base + (c0 * G + c1) * G + c2, c = clamp(trunc((flipped / |flipped| + 1) * hinv), 0, G - 1); G = 0: key_base.
 * Points outside the mask get DODA_VSS_KEY_NONE.  grid_h fp64 [n_seg][4] on the HOST: (radius, hinv, G, key_base),
 * 0 <= G <= DODA_VSS_MAX_GRID. */
int doda_vss_flip(const float *xyz, const int64_t *offsets_h, int32_t n_seg, const double *view, const uint8_t *mask,
                  const double *grid_h, double *flipped, int32_t *key, doda_stream_t stream);

/* The vertex decision, one wavefront per query.  pts fp64 [M][3]: the flipped points of the batch's views SORTED by key (stably);
 * index int32 [M]: their point numbers; seg_begin_h int32 [n_seg + 1] (HOST): the rows of each segment; cell_start int32
 * (device): first row of every key, one past the largest key included (may be NULL with DODA_VSS_EXHAUSTIVE);
 * win_h fp64 [n_seg][4] (HOST): (G, hinv, half, key_base) as given to doda_vss_flip, half = the box of the windowed program
 * (G = 0 or half <= 0: the segment has no window and is decided exhaustively).  queries int32 [n_queries] rows of pts, or NULL
 * for all M rows.
 *   windowed: the constraints are the rows of the 3 x 3 x 3 cells around the query's.  Feasible in the box: state 1.
 *             Infeasible in the unbounded program (a box of 1e6): state 0.  Otherwise state 2 (undecided).
 *   exhaustive: all rows of the segment; state 1 or 0.
 * Either way a query visits its constraints in a fixed scattered order ((m * prime) mod their number), the same on every run.
 * state uint8 [M] is written at the query's row; selected uint8 [N]: selected[index[row]] = 1 for state 1 (never cleared). */
int doda_vss_extreme(const double *pts, const int32_t *index, const int32_t *seg_begin_h, int32_t n_seg, const int32_t *cell_start,
                     const double *win_h, const int32_t *queries, int64_t n_queries, int32_t flags, uint8_t *selected,
                     uint8_t *state, doda_stream_t stream);

/* selected uint8 [N] -> count int32 [n_seg] (ADDED to; the caller zeroes it) and blk_cnt int32 [doda_vss_blocks] (written). */
int doda_vss_count(const uint8_t *selected, const int64_t *offsets_h, int32_t n_seg, int32_t *count, int32_t *blk_cnt,
                   doda_stream_t stream);

/* The sample after vss: the selected points in their order (stable compaction over blk_cnt), per segment s from output row
 * out_base_h[s] (int64 [n_seg], HOST):
 *     out_xyz fp32 [M][3] = (float)((double)xyz[i] + noise[i])  (noise fp64 [N][3], or NULL: out_xyz = xyz[i])
 *     out_labels int32 [M] = labels[i];  out_index int32 [M] = i;  out_mask1 / out_mask2 uint8 [M] (each pair NULL or not)
 * Rows at or beyond out_len are not written. */
int doda_vss_emit(const float *xyz, const double *noise, const int32_t *labels, const uint8_t *mask1, const uint8_t *mask2,
                  const int64_t *offsets_h, int32_t n_seg, const uint8_t *selected, const int32_t *blk_cnt,
                  const int64_t *out_base_h, float *out_xyz, int32_t *out_labels, int32_t *out_index, uint8_t *out_mask1,
                  uint8_t *out_mask2, int64_t out_len, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_VSS_H */

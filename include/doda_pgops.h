/*
 * doda_pgops.h — companion C ABI of libdoda_hip.so: the rest of the reference's PG_OP module (lib/pointgroup_ops/src/
 * pointgroup_ops_api.cpp:6-26) — clustering (bfs_cluster), segment pools (sec_mean, sec_mean_bp, sec_min, sec_max, roipool_fp,
 * roipool_bp) and proposal IoU (get_iou).  With the core header's voxelize / point_recover / ballquery / knn entry points this
 * completes the 15 functions of that module.
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device pointers +
 * sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; sizes and null pointers are
 * checked on the host before anything launches (DODA_ERR_INVALID); a count of zero is DODA_OK with no launch.  The core header's
 * surface (ABI 12) and the other companions are unchanged; this header carries its own version, DODA_PGOPS_ABI_VERSION.
 *
 * Features are fp32, offsets and indices int32, instance_labels int64, as in the reference.  Every kernel is safe on corrupt
 * inputs: an offset pair with end < start is an empty segment, starts and ends are clamped to the array, and a neighbour or point
 * index outside [0, N) is skipped.
 *
 * Empty segment: mean 0, min +inf, max and roipool -inf, argmax -1 (what the reference's 1e50 constants become in float).
 */
#ifndef DODA_PGOPS_H
#define DODA_PGOPS_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_PGOPS_ABI_VERSION 1

#define DODA_PG_WAVE_LIST 64          /* neighbour lists longer than this are hooked by a whole wave, shorter ones by one lane */
#define DODA_PG_LONG_SEGMENT 2048     /* n_rows / n_seg from which the segment kernels run 1024-thread workgroups instead of 256 */
#define DODA_PG_IOU_LDS_INSTANCES 8192 /* most instances whose per-proposal histogram lives in LDS; above it: the workspace */

int32_t doda_pgops_abi_version(void);

/* Connected components of the graph  i -- j  for every j in i's neighbour list (ball_query_idxs[start .. start + len) with
 * (start, len) = start_len[i]) that has semantic_label[j] == semantic_label[i]; edges count as undirected, self entries and
 * duplicates are harmless.  root[i] (device int32 [n]): the smallest point index of i's component.  size[i] (device int32 [n]):
 * the component's point count where root[i] == i, 0 elsewhere.  Lock-free union-find in four launches (init, hook, flatten, count),
 * no host read-back, no float atomic: the outputs are a function of the inputs alone.
 * DODA_ERR_INVALID: n < 0, n_active < 0, a null semantic_label / start_len / root / size with n > 0, a null ball_query_idxs with
 * n_active > 0. */
int doda_pg_components(const int32_t *semantic_label, const int32_t *ball_query_idxs, const int32_t *start_len, int32_t n,
                       int32_t n_active, int32_t *root, int32_t *size, doda_stream_t stream);

/* HOST route (all pointers host memory, no GPU touched): the reference's sequential rule (bfs_cluster/bfs_cluster.cpp:28-86) —
 * seeds ascending, a queue, directed edges, a first-visit mark; a component of at least `threshold` points becomes a cluster.
 * cluster_idxs: int32 [n][2] capacity, rows (cluster id, point index) in the reference's order; cluster_offsets: int32 [n + 1]
 * capacity; *sum_npoint rows and *n_cluster + 1 offsets are written.  DODA_ERR_INVALID: n < 0, n_active < 0, a null out-parameter,
 * a null array that the sizes make necessary. */
int doda_pg_bfs_cluster_h(const int32_t *semantic_label, const int32_t *ball_query_idxs, const int32_t *start_len, int32_t n,
                          int32_t n_active, int32_t threshold, int32_t *cluster_idxs, int32_t *cluster_offsets,
                          int32_t *sum_npoint, int32_t *n_cluster);

/* Segment operators over inp [n_rows][c] and offsets [n_seg + 1]: segment s covers rows offsets[s] .. offsets[s + 1].
 * out [n_seg][c].  sec_mean sums the rounded quotients x / float(len); sec_min / sec_max / roipool_fp are bit-exact and order-free;
 * roipool's maxidx [n_seg][c] is the smallest row among the maxima (the reference's strict >; NaN never wins, nor does -inf).
 * Element offsets are 64-bit, so n_rows * c and n_seg * c may pass 2^31.  DODA_ERR_INVALID: n_rows, n_seg or c negative; with
 * n_seg > 0 and c > 0, a null offsets / out (/ maxidx) or a null inp with n_rows > 0.  n_seg == 0 or c == 0: DODA_OK, no launch. */
int doda_pg_sec_mean(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                     doda_stream_t stream);
int doda_pg_sec_min(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                    doda_stream_t stream);
int doda_pg_sec_max(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                    doda_stream_t stream);
int doda_pg_roipool_fp(const float *feats, const int32_t *offsets, float *out, int32_t *maxidx, int32_t n_rows, int32_t n_seg,
                       int32_t c, doda_stream_t stream);

/* d_inp[row][ch] = d_out[s][ch] / float(len) for the rows of every segment (one division); rows outside every segment are left
 * untouched.  Same argument rules as above. */
int doda_pg_sec_mean_bp(float *d_inp, const int32_t *offsets, const float *d_out, int32_t n_rows, int32_t n_seg, int32_t c,
                        doda_stream_t stream);

/* d_feats[maxidx[s][ch]][ch] += d_out[s][ch].  Segments are disjoint, so this is a plain add, not an atomic.  An argmax outside
 * [0, n_rows) — the -1 of an empty segment — is skipped (the reference writes out of bounds there: a deliberate fix). */
int doda_pg_roipool_bp(float *d_feats, const int32_t *maxidx, const float *d_out, int32_t n_rows, int32_t n_seg, int32_t c,
                       doda_stream_t stream);

/* Bytes of the device workspace of doda_pg_get_iou: 0 while n_instance <= DODA_PG_IOU_LDS_INSTANCES, else one int32 row of
 * n_instance counters per proposal. */
size_t doda_pg_get_iou_workspace_bytes(int32_t n_proposal, int32_t n_instance);

/* iou [n_proposal][n_instance] = float( double(float(inter)) / (double(float(p_total + inst_total - inter)) + 1e-5) ) with
 * inter = the number of i in the proposal's range of proposals_idx [sum_npoint] whose instance_labels[proposals_idx[i]] (int64
 * [n_points]) equals the instance; labels outside [0, n_instance) (-100 among them) match nothing.  One integer histogram per
 * proposal: O(proposal points + n_instance) work.  ws: 4-byte aligned device memory of at least the workspace bytes
 * (DODA_ERR_WORKSPACE), may be null when they are 0.  DODA_ERR_INVALID: a negative size, a null array that the sizes make
 * necessary. */
int doda_pg_get_iou(const int32_t *proposals_idx, const int32_t *proposals_offset, const int64_t *instance_labels,
                    const int32_t *instance_pointnum, float *iou, int32_t n_points, int32_t sum_npoint, int32_t n_instance,
                    int32_t n_proposal, void *ws, size_t ws_bytes, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_PGOPS_H */

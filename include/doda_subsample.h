/*
 * doda_subsample.h — companion C ABI of libdoda_hip.so: the random subsample of every training item under
 * DATA_PROCESSOR.downsampling_scale (reference dataset/s3dis.py:59-63, dataset/front3d.py:65, dataset/dataset.py:73-77: the first
 * int(n / ds) indices of a permutation, sorted).
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device
 * pointers + sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; argument
 * errors come back as statuses without a launch.  The core header's surface (ABI 12) and the other companions are unchanged; this
 * header carries its own version, DODA_SUBSAMPLE_ABI_VERSION, and the same library exports all of them.
 *
 * The scenes of a batch are SEGMENTS of one array: n_seg + 1 offsets given on the HOST (int64, offsets_h[0] = 0, non-decreasing,
 * at most 2^31 - 1 points, 1 <= n_seg <= DODA_SUBSAMPLE_MAX_SEGMENTS), validated before anything is launched and passed to the
 * kernels as launch arguments.  A segment is cut into chunks of DODA_SUBSAMPLE_CHUNK points, one workgroup each.
 *
 * The draw.  Point j of segment b has the 32-bit key  philox4x32_10(counter = (j, 0, 0, 0), key = seeds_h[b])[0] & key_mask
 * (Philox-4x32-10 of Random123; seeds_h[b] = key word 0 | key word 1 << 32).  Segment b keeps the k_h[b] points that are smallest
 * in the lexicographic order (key, j) and writes them in ascending j: with independent keys a uniformly random k_h[b]-subset,
 * sorted.  key_mask = 0xffffffff for a draw; smaller masks force equal keys (mask 0 keeps points 0 .. k - 1).
 *
 * How.  T_b, the k_b-th smallest key of segment b, is found by a radix select over the key — DODA_SUBSAMPLE_LEVELS passes of
 * DODA_SUBSAMPLE_RADIX_BITS bits, per-workgroup histograms added to per-segment counters, every pass resolving its digit on the
 * device from the counters of the pass before — then one pass counts, per chunk, the points below T_b and the points equal to T_b,
 * and one pass writes the kept points at  (kept in the earlier chunks) + (kept earlier in the chunk): a point with key == T_b is
 * kept iff fewer than r_b equal points precede it in its segment (r_b = k_b - points below T_b).  No key is stored, no atomic
 * decides an output row, nothing is read back; the output is a function of the arguments alone.
 */
#ifndef DODA_SUBSAMPLE_H
#define DODA_SUBSAMPLE_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_SUBSAMPLE_ABI_VERSION 1

#define DODA_SUBSAMPLE_MAX_SEGMENTS 64
#define DODA_SUBSAMPLE_CHUNK 1024       /* points per workgroup */
#define DODA_SUBSAMPLE_RADIX_BITS 8
#define DODA_SUBSAMPLE_LEVELS 4

int32_t doda_subsample_abi_version(void);

/* Bytes of the workspace of a draw over these segments (the per-segment digit counters, the thresholds and two counts per
 * chunk); 0 for offsets that are not valid (see above). */
size_t doda_subsample_workspace_bytes(const int64_t *offsets_h, int32_t n_seg);

/* The draw described above.  xyz fp32 [N][3], labels int32 [N]; extra_i32 int32 [N] and extra_u8 uint8 [N] are optional further
 * columns (NULL: none; an input column and its output come together).  k_h int32 [n_seg], 0 <= k_h[b] <= points of segment b;
 * seeds_h uint64 [n_seg].  Outputs, packed per segment from row sum(k_h[0 .. b - 1]) on: out_xyz [K][3] (bit copies of the kept
 * rows), out_labels [K], out_idx int32 [K] (the kept point's index INSIDE its segment), out_extra_i32 / out_extra_u8 [K];
 * K = sum(k_h).  No row at or beyond K is written.  ws: 4-byte aligned, ws_bytes at least the answer above (DODA_ERR_WORKSPACE);
 * the call zeroes what it needs on `stream`.  An empty segment and k_h[b] = 0 emit nothing; k_h[b] = points copies the segment. */
int doda_subsample_draw(const float *xyz, const int32_t *labels, const int32_t *extra_i32, const uint8_t *extra_u8,
                        const int64_t *offsets_h, int32_t n_seg, const int32_t *k_h, const uint64_t *seeds_h, uint32_t key_mask,
                        float *out_xyz, int32_t *out_labels, int32_t *out_idx, int32_t *out_extra_i32, uint8_t *out_extra_u8,
                        void *ws, size_t ws_bytes, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_SUBSAMPLE_H */

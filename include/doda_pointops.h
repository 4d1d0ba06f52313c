/*
 * doda_pointops.h — companion C ABI of libdoda_hip.so: the rest of the reference's pointops2_cuda module (lib/pointops2/src/
 * pointops_api.cpp:12-23) — furthest point sampling, grouping, interpolation, subtraction and aggregation, forward and backward.
 * With the core header's doda_knnquery this completes the 11 functions of that module.
 *
 * Same conventions as doda_pgops.h: extern "C", plain device pointers + sizes, an explicit HIP stream, an int status (the codes and
 * doda_strerror of doda_hip.h).  Nothing here allocates device memory or synchronises; sizes and null pointers are checked on the
 * host before anything launches (DODA_ERR_INVALID); a count of zero is DODA_OK with no launch.  Element offsets are 64-bit, so
 * rows * nsample * c may pass 2^31 (rows * nsample itself may not: positions are int32).  The core header's surface (ABI 12) and
 * the other companions are unchanged; this header carries its own version, DODA_POINTOPS_ABI_VERSION.
 *
 * Features are fp32, indices and offsets int32, as in the reference.
 *
 * ORDER.  Outputs are a function of the inputs alone: no float atomic anywhere.  Every product, sum and difference is rounded once
 * (no FMA contraction), every sum starts at +0 and adds its terms in the order stated at the entry point.  The reference's
 * backward kernels scatter with float atomicAdd, so their last bits depend on arrival order; here every scatter is a gather over the
 * index transposed by destination (doda_po_transpose), summed in ascending position.
 *
 * BOUNDS (a deliberate fix: the reference reads and writes out of bounds in each of these cases).  An index outside [0, n) reads as
 * 0 in a forward and contributes to no gradient of the indexed array; a segment whose end lies below its start is empty; offsets
 * and list ranges are clamped to their arrays.
 *
 * OVERWRITE.  The reference's kernels add into buffers that its wrappers zero first; these entry points write every element of
 * their outputs and read none of them.
 */
#ifndef DODA_POINTOPS_H
#define DODA_POINTOPS_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_POINTOPS_ABI_VERSION 1

#define DODA_PO_WAVE_LIST 64   /* transposed lists longer than this are sorted by a whole wave, shorter ones by one lane */
#define DODA_PO_FPS_BLOCK 1024 /* threads of the one workgroup that samples a segment */
#define DODA_PO_FPS_REG 8      /* points per thread whose coordinates and running distance stay in registers: a segment of up to
                                  DODA_PO_FPS_BLOCK * DODA_PO_FPS_REG points touches no memory inside the sampling loop */
#define DODA_PO_FPS_MAX_DIM 8

int32_t doda_pointops_abi_version(void);

/* The index by destination of idx [m][nsample] with values in [0, n):
 *   start int32 [n + 1]; pos int32 [m * nsample] capacity.  pos[start[j] .. start[j + 1]) are the flat positions
 *   p = row * nsample + i with idx[p] == j, ascending.  Entries outside [0, n) are dropped, so start[n] <= m * nsample and the
 *   tail of pos is left unwritten.
 * Counting and filling use integer atomics (order-free); every list is then sorted ascending: lists of up to DODA_PO_WAVE_LIST
 * entries by one lane, longer ones by one wave.
 * ws: 4-byte aligned device memory of at least doda_po_transpose_workspace_bytes(n) (DODA_ERR_WORKSPACE when smaller).
 * DODA_ERR_INVALID: m, nsample or n negative, m * nsample above INT32_MAX; with n > 0, a null start, a null or misaligned ws, or
 * a null idx / pos while m * nsample > 0.  n == 0: DODA_OK, nothing is written (start[0] included).  m * nsample == 0 with
 * n > 0: start[0 .. n] = 0. */
size_t doda_po_transpose_workspace_bytes(int32_t n);
int doda_po_transpose(const int32_t *idx, int32_t m, int32_t nsample, int32_t n, int32_t *start, int32_t *pos, void *ws,
                      size_t ws_bytes, doda_stream_t stream);

/* The backward entry points below take (start, pos) as doda_po_transpose wrote them for the same idx and destination count n;
 * `total` = m * nsample is the number of positions.  They too are safe on corrupt input: start is clamped to [0, total], a position
 * outside [0, total) is skipped.
 *
 * Argument errors of all of them (DODA_ERR_INVALID): a negative size; c < 1 where rows exist; a null pointer to an array that the
 * sizes make non-empty.  No output element to write: DODA_OK, no launch. */

/* out [m][nsample][c]:  out[r][i][:] = inp[idx[r][i]][:]      (inp [n][c]) */
int doda_po_grouping_fwd(const float *inp, const int32_t *idx, float *out, int32_t n, int32_t m, int32_t nsample, int32_t c,
                         doda_stream_t stream);
/* d_inp [n][c]:  d_inp[j][:] = sum over j's list, ascending p, of d_out[p][:]      (d_out [total][c]) */
int doda_po_grouping_bwd(const float *d_out, const int32_t *start, const int32_t *pos, float *d_inp, int32_t n, int32_t total,
                         int32_t c, doda_stream_t stream);

/* out [m][c]:  out[r][ch] = sum over i ascending of inp[idx[r][i]][ch] * w[r][i]      (inp [n][c], idx and w [m][k]) */
int doda_po_interpolation_fwd(const float *inp, const int32_t *idx, const float *w, float *out, int32_t n, int32_t m, int32_t k,
                              int32_t c, doda_stream_t stream);
/* d_inp [n][c]:  d_inp[j][ch] = sum over j's list, ascending p, of d_out[p / k][ch] * w[p]      (d_out [m][c], total = m * k) */
int doda_po_interpolation_bwd(const float *d_out, const float *w, const int32_t *start, const int32_t *pos, float *d_inp, int32_t n,
                              int32_t m, int32_t k, int32_t c, doda_stream_t stream);

/* out [m][nsample][c]:  out[r][i][ch] = a[r][ch] - b[idx[r][i]][ch]      (a [m][c], b [n][c]; the reference has m == n) */
int doda_po_subtraction_fwd(const float *a, const float *b, const int32_t *idx, float *out, int32_t n, int32_t m, int32_t nsample,
                            int32_t c, doda_stream_t stream);
/* d_a [m][c]:  d_a[r][ch] = sum over i ascending of d_out[r][i][ch]            (no scatter)
 * d_b [n][c]:  d_b[j][ch] = sum over j's list, ascending p, of (-d_out[p][ch]) */
int doda_po_subtraction_bwd(const float *d_out, const int32_t *start, const int32_t *pos, float *d_a, float *d_b, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, doda_stream_t stream);

/* out [m][c]:  out[r][ch] = sum over i ascending of (inp[idx[r][i]][ch] + position[r][i][ch]) * w[r][i][ch % w_c]
 * (inp [n][c], position [m][nsample][c], w [m][nsample][w_c]; any c >= 1 and w_c >= 1: w_c need not divide c) */
int doda_po_aggregation_fwd(const float *inp, const float *position, const float *w, const int32_t *idx, float *out, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, int32_t w_c, doda_stream_t stream);
/* With g = d_out [m][c]:
 * d_position [m][nsample][c]:  g[r][ch] * w[r][i][ch % w_c]
 * d_w [m][nsample][w_c]:       d_w[r][i][k] = sum over ch with ch % w_c == k, ascending, of g[r][ch] * (inp[idx[r][i]][ch] + position[r][i][ch])
 * d_inp [n][c]:                d_inp[j][ch] = sum over j's list, ascending p, of g[p / nsample][ch] * w[p][ch % w_c] */
int doda_po_aggregation_bwd(const float *inp, const float *position, const float *w, const int32_t *idx, const int32_t *start,
                            const int32_t *pos, const float *d_out, float *d_inp, float *d_position, float *d_w, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, int32_t w_c, doda_stream_t stream);

/* Furthest point sampling per batch segment.  xyz [n][dim], dim in 1 .. DODA_PO_FPS_MAX_DIM; offset and new_offset int32 [nbatch]
 * are END offsets (as doda_knnquery takes them): segment b covers points offset[b - 1] .. offset[b] (0 for b == 0) and fills
 * idx[new_offset[b - 1] .. new_offset[b]); idx int32 [m] capacity, output ranges clamped to it.  ws: n floats, the running
 * distances of the points that do not fit a workgroup's registers; initialised here, its contents on entry are not read.
 *
 * Per segment: the first sample is the segment's first point.  Each further sample is the point that maximises
 * t = min(previous running distance, d), d = ((0 + dx*dx) + dy*dy) + ... to the last sample over the dim coordinates, each
 * operation rounded (dim 3: the dist2 of the neighbour queries); t becomes the point's running distance, which starts at 1e10.
 * TIES GO TO THE LOWEST POINT INDEX.  The reference's winner among exact ties is the smallest bit-reversed thread id of a
 * power-of-two block sized by the largest segment of the batch, so it changes with the batch a cloud is sampled in and no caller
 * can rely on it; this rule is pinned instead.  A segment asked for more samples than it has points keeps sampling by the same
 * rule (repeats); a segment without points that is asked for samples gets -1.
 *
 * One workgroup of DODA_PO_FPS_BLOCK threads per segment, one barrier per sample.
 * DODA_ERR_INVALID: n, m or nbatch negative, dim outside 1 .. DODA_PO_FPS_MAX_DIM, a null offset / new_offset with nbatch > 0, a
 * null idx with m > 0, a null xyz or ws with n > 0.  nbatch == 0 or m == 0: DODA_OK, no launch. */
int doda_po_furthestsampling(const float *xyz, const int32_t *offset, const int32_t *new_offset, float *ws, int32_t *idx, int32_t n,
                             int32_t m, int32_t nbatch, int32_t dim, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_POINTOPS_H */

/*
 * doda_eval.h — companion C ABI of libdoda_hip.so: scoring a scene whose processed cloud is a SUBSET of its full cloud (reference
 * model/unet.py:135-145, test_model_fn with the `*_all` keys of dataset/s3dis.py:54-130: the network runs on a subsample, every
 * point of the full cloud takes the scores of its nearest processed point, loss and IoU are taken on the full cloud).
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device pointers +
 * sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises.  The core header's surface
 * (ABI 12) and the other companions are unchanged; this header carries its own version, DODA_EVAL_ABI_VERSION, and the same
 * library exports all.
 *
 * Nearest processed point.  The brute-force 1-nearest-neighbour query of the core header sweeps every processed point of the scene
 * per full point; here the processed points of every scene sit in a uniform grid of cells and a query walks the cells around its
 * own in shells of growing Chebyshev radius.  The answer is bit-identical to the brute force's for every query: the same distance
 * arithmetic (each operation rounded, no contraction), the lexicographic minimum of (distance, index) — what "the first strictly
 * smaller candidate in ascending index" amounts to — and a stopping rule that is conservative under fp32 rounding: after the cube
 * of radius r has been visited the search ends only when the best distance is strictly below a lower bound of the distance of
 * every point outside the cube, or when the cube covers the scene's whole grid.
 *
 * The cell table (built by the caller, doda_amd.ops.eval_table; per batch):
 *   scenes      per scene its END offsets, grid origin, cell side and its reciprocal, grid dimensions and first cell (host array);
 *   cell of a processed point p of scene s, per axis k:  clamp(floor((p[k] - origin[k]) * inv_side), 0, dims[k] - 1), fp32;
 *   cell id     cell_base + (cx * dims[1] + cy) * dims[2] + cz        (z runs fastest: a z-run of cells is one range of points);
 *   order       int32 [n]: the processed points sorted by cell id, STABLY (ascending index inside a cell);
 *   xyz_sorted  fp32 [n, 3]: xyz[order];
 *   cell_start  int32 [cells of all scenes + 1]: first position in `order` of every cell, the last entry = n.
 *
 * Scoring.  Every point of a voxel has its voxel's logits, so the [full points, classes] score matrix of the reference is never
 * built: per full point the voxel row is read through p2v[idx[i]] and the head is recomputed (16 n_cls fused multiply-adds).
 */
#ifndef DODA_EVAL_H
#define DODA_EVAL_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_EVAL_ABI_VERSION 1

#define DODA_EVAL_MAX_SCENES 32             /* scenes per call */
#define DODA_EVAL_MAX_CELLS (1 << 21)       /* cells of one scene's grid */
#define DODA_EVAL_MAX_CLASSES 32

typedef struct doda_eval_scene {
    int32_t n_end, m_end;      /* END offsets of the scene's processed points (xyz) and of its full points (new_xyz) */
    int32_t cell_base;         /* the scene's first entry in cell_start */
    int32_t dims[3];           /* cells per axis, each >= 1, their product <= DODA_EVAL_MAX_CELLS */
    float origin[3];           /* the grid's lower corner: the minimum of the scene's processed points */
    float side, inv_side;      /* cell side in metres (> 0) and the fp32 reciprocal the cells were assigned with */
} doda_eval_scene;

int32_t doda_eval_abi_version(void);

/* idx[q] / dist2[q] for every full point q < m: the processed point of q's scene with the smallest (dist2, index) and that squared
 * distance — bit-identical to the brute-force 1-nearest-neighbour query of the core header on (xyz, new_xyz, the scenes' offsets).
 * scenes_h: HOST array [nbatch] (copied into the launch); xyz_sorted, order, cell_start: the cell table above (device);
 * new_xyz fp32 [m, 3]; qorder int32 [m] or NULL: a permutation of the queries (thread t answers query qorder[t]; sorted by cell,
 * a wave walks the same cells) — the result does not depend on it.
 * n, m: 64-bit so that sizes past int32 come back as DODA_ERR_UNSUPPORTED; a scene with no processed point and a non-empty full
 * cloud, offsets that decrease or do not end at n / m, or a grid outside the limits: DODA_ERR_INVALID;
 * nbatch > DODA_EVAL_MAX_SCENES: DODA_ERR_UNSUPPORTED. */
int doda_eval_nn(const float *xyz_sorted, const int32_t *order, int64_t n, const int32_t *cell_start, const doda_eval_scene *scenes_h,
                 int32_t nbatch, const float *new_xyz, const int32_t *qorder, int64_t m, int32_t *idx, float *dist2,
                 doda_stream_t stream);

/* Workgroups of doda_eval_score = rows of its partial_ws. */
int32_t doda_eval_score_blocks(int64_t m);

/* Full-cloud scores without the score matrix.  feats [m_vox, c] bf16 (elem_bytes 2) or fp32 (4), c in {16, 32}; weight fp32
 * [n_cls, c] (rounded to bf16 first for bf16 features), bias fp32 [n_cls] or NULL, 2 <= n_cls <= DODA_EVAL_MAX_CLASSES; p2v int32
 * [n] (processed point -> voxel row); idx int32 [m] (full point -> processed point) or NULL = identity (then m == n); labels_all
 * int64 [m].  For full point i, v = p2v[idx[i]]:
 *   pred_all[i] (uint8 [m], or NULL) = argmax_k z_v[k], the bits of the voxel-level head's prediction elsewhere in the library;
 *   hist int64 [3][n_cls] (intersection, prediction area, target area) is ADDED to, over the valid points: label != ignore_index
 *   and 0 <= label < n_cls (integer atomics: exact, order-independent);
 *   out fp64 [2] = { sum over valid points of lse_v - z_v[label], number of valid points } (SET): per-workgroup fp64 partials in
 *   partial_ws fp64 [n_blocks][2], combined in a fixed order by a second launch — the same bits on every run.
 * A point whose idx / p2v entry is out of range is dropped (pred 0).  n_blocks = doda_eval_score_blocks(m). */
int doda_eval_score(const void *feats, int32_t m_vox, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                    int32_t n_cls, const int32_t *p2v, int64_t n, const int32_t *idx, const int64_t *labels_all, int64_t m,
                    int64_t ignore_index, uint8_t *pred_all, int64_t *hist, double *out, double *partial_ws, int32_t n_blocks,
                    doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_EVAL_H */

// Evaluation on a full cloud whose processed cloud is a subsample (include/doda_eval.h; reference model/unet.py:135-145):
// doda_eval_nn, the exact nearest processed point over a uniform grid, and doda_eval_score, predictions / class histograms /
// cross-entropy of the full cloud without the [full points, classes] score matrix.
//
// doda_eval_nn: ONE LANE PER QUERY, the queries handed out in cell order (qorder) so that the lanes of a wave walk the same cells and
// their candidate reads hit the same lines.  (One wave per query cell with the candidates staged in LDS shares more, but a shell of
// radius r around a cell holds a different point count for every cell and the queries outside the grid have no cell of their own;
// the per-lane walk needs no barrier and no staging and its divergence is bounded by the wave's spread of radii.)  Candidates are
// read from xyz_sorted — the cells of a z-run are one contiguous range — and `order` is read only where a candidate ties or wins.
#include "common.hpp"
#include "spconv_common.hpp"
#include "head_common.hpp"
#include "neighbors_common.hpp"
#include "../../include/doda_eval.h"

namespace {
constexpr int EV_BLOCK = 256;

struct EvalScenes {                                      // launch argument, validated on the host (eval_scenes)
    int32_t n;
    doda_eval_scene s[DODA_EVAL_MAX_SCENES];
};

// the cell coordinate along one axis: THE expression the table's builder assigns the processed points with (doda_amd.ops.eval_table:
// floor((x - origin) * inv_side) in fp32, clamped to the grid; NaN -> 0)
__device__ __forceinline__ int eval_cell(float x, float origin, float inv_side, int dim) {
    const float t = floorf(__fmul_rn(__fsub_rn(x, origin), inv_side));
    return t >= 0.f ? (t < (float)dim ? (int)t : dim - 1) : 0;
}

__global__ __launch_bounds__(EV_BLOCK) void eval_nn(EvalScenes sc, const float *__restrict__ cand, const int32_t *__restrict__ order,
                                                    const int32_t *__restrict__ cell_start, const float *__restrict__ new_xyz,
                                                    const int32_t *__restrict__ qorder, int m, int32_t *__restrict__ idx,
                                                    float *__restrict__ dist2) {
    __shared__ doda_eval_scene ss[DODA_EVAL_MAX_SCENES];
    {
        constexpr int WORDS = sizeof(doda_eval_scene) / 4;
        const int32_t *src = reinterpret_cast<const int32_t *>(&sc.s[0]);
        int32_t *dst = reinterpret_cast<int32_t *>(&ss[0]);
        for (int e = threadIdx.x; e < sc.n * WORDS; e += EV_BLOCK) dst[e] = src[e];
    }
    doda_sync();
    const int t = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (t >= m) return;                                  // (no barrier below)
    const int q = qorder ? qorder[t] : t;
    if ((unsigned)q >= (unsigned)m) return;              // (a qorder that is no permutation writes nothing out of bounds)
    int b = 0;
    while (b < sc.n - 1 && q >= ss[b].m_end) ++b;
    const doda_eval_scene &g = ss[b];
    const int start = b == 0 ? 0 : ss[b - 1].n_end, end = g.n_end;
    const float qx = new_xyz[q * 3LL], qy = new_xyz[q * 3LL + 1], qz = new_xyz[q * 3LL + 2];
    const float qv[3] = {qx, qy, qz};
    // the brute force's start state: nothing at or above 1e10 is ever taken, the index then stays the scene's first
    float best = 1e10f;
    int besti = start;
    const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = eval_cell(qv[k], g.origin[k], g.inv_side, g.dims[k]);
    // the radius at which the cube around (the clamped) c covers the whole grid: the search always ends there
    int rmax = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rmax = c[k] > rmax ? c[k] : rmax;
        rmax = g.dims[k] - 1 - c[k] > rmax ? g.dims[k] - 1 - c[k] : rmax;
    }
    // Rounding allowance of the stopping rule.  Let S bound the magnitude of every intermediate below and in eval_cell (|q|, |origin|,
    // the grid's extent).  A processed point p whose cell along axis k is >= h satisfies floor(fl(fl(p - o) * inv)) >= h; rounding is
    // monotone, so fl(p - o) * inv >= h (1 - 2^-24), inv = (1 / side)(1 + e), |e| <= 2^-24, hence p - o >= h side - 3 * 2^-24 S
    // (one more 2^-24 S for fl(p - o)); the mirrored bound holds for a cell <= l.  The face distance below takes three more rounded
    // operations (h * side, + o, - q), each within 2^-24 S.  Together under 7 * 2^-24 S; the allowance is 2^-20 S = 16 * 2^-24 S.
    // dist2_rn of a point at true distance >= d is >= d^2 (1 - 5 * 2^-24) (three differences, three squares, two sums: every factor
    // within 2^-24, all terms non-negative), and the square of the bound is one more rounding; the factor 1 - 2^-18 covers 64 of them.
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) S = fmaxf(S, fabsf(qv[k]) + fabsf(g.origin[k]) + (float)g.dims[k] * g.side);
    const float allowance = S * 9.5367431640625e-07f;    // 2^-20
    for (int r = 0;; ++r) {
        // the shell of Chebyshev radius r inside the grid: full z-runs where |dx| or |dy| is r, the two end cells elsewhere
        const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < nx - 1 ? c[0] + r : nx - 1;
        const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < ny - 1 ? c[1] + r : ny - 1;
        const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < nz - 1 ? c[2] + r : nz - 1;
        for (int x = x0; x <= x1; ++x) {
            const bool xe = x - c[0] == r || c[0] - x == r;
            for (int y = y0; y <= y1; ++y) {
                const int row = g.cell_base + (x * ny + y) * nz;
                const bool edge = xe || y - c[1] == r || c[1] - y == r;
                // up to two ranges of positions in `order`: [a0, a1) and [b0, b1)
                int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
                if (edge) {
                    a0 = cell_start[row + z0]; a1 = cell_start[row + z1 + 1];
                } else {
                    if (c[2] - r >= 0) { a0 = cell_start[row + c[2] - r]; a1 = cell_start[row + c[2] - r + 1]; }
                    if (c[2] + r <= nz - 1) { b0 = cell_start[row + c[2] + r]; b1 = cell_start[row + c[2] + r + 1]; }
                }
                // (positions stay inside the scene's own points whatever the table holds)
                a0 = a0 < start ? start : a0; a1 = a1 > end ? end : a1;
                b0 = b0 < start ? start : b0; b1 = b1 > end ? end : b1;
                for (int pass = 0; pass < 2; ++pass) {
                    const int j0 = pass ? b0 : a0, j1 = pass ? b1 : a1;
                    for (int j = j0; j < j1; ++j) {
                        const float d = dist2_rn(qx, qy, qz, cand[j * 3LL], cand[j * 3LL + 1], cand[j * 3LL + 2]);
                        if (d <= best) {                 // the lexicographic minimum of (d, index): cells come in no index order
                            const int i = order[j];
                            if (d < best || i < besti) { best = d; besti = i; }
                        }
                    }
                }
            }
        }
        if (r >= rmax) break;                            // the cube covers the grid: every point of the scene was a candidate
        // Lower bound of the distance from q to any point OUTSIDE the cube [c - r, c + r]: such a point has, along some axis, a cell
        // <= c - r - 1 (it then lies below the face origin + (c - r) side) or >= c + r + 1 (above origin + (c + r + 1) side).  A side
        // on which the cube reaches the grid's edge has no point beyond it.  A query outside the cube (its cell was clamped) makes a
        // face distance negative: no stop, the cube keeps growing.
        float gap = INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int lo = c[k] - r, hi = c[k] + r + 1;
            if (lo > 0) gap = fminf(gap, __fsub_rn(qv[k], __fadd_rn(g.origin[k], __fmul_rn((float)lo, g.side))));
            if (hi < g.dims[k]) gap = fminf(gap, __fsub_rn(__fadd_rn(g.origin[k], __fmul_rn((float)hi, g.side)), qv[k]));
        }
        gap -= allowance;
        if (gap > 0.f && best < __fmul_rn(__fmul_rn(gap, gap), 0.999996185302734375f)) break;     // 1 - 2^-18; STRICTLY below
    }
    idx[q] = besti;
    dist2[q] = best;
}

// ---- full-cloud scoring -------------------------------------------------------------------------------------------------------
// One thread per full point (grid-stride): the voxel row through p2v[idx[i]], the logits with hd_logits (the prediction's bits are
// head_ce_fwd's and st_voxel_conf's), integer class histograms in LDS flushed with integer atomics, the loss as per-thread fp64 sums
// reduced in a fixed order (butterfly, then the four waves in order) into the workgroup's row of `partial`.
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(HD_BLOCK, 4) void eval_score(const void *__restrict__ feats, int m_vox, const float *__restrict__ weight,
                                                       const float *__restrict__ bias, int n_cls, const int32_t *__restrict__ p2v, int n,
                                                       const int32_t *__restrict__ idx, const long long *__restrict__ labels, int m,
                                                       long long ignore_index, uint8_t *__restrict__ pred_all,
                                                       unsigned long long *__restrict__ hist, double *__restrict__ partial) {
    __shared__ float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    __shared__ unsigned h[3][HD_MAX_K];
    __shared__ double red[2][HD_BLOCK / 64];
    for (int e = threadIdx.x; e < 3 * HD_MAX_K; e += HD_BLOCK) (&h[0][0])[e] = 0u;
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);      // (ends with the barrier that also publishes the zeroed histograms)
    double loss = 0.0, cnt = 0.0;
#pragma unroll 1
    for (long long i = (long long)blockIdx.x * HD_BLOCK + threadIdx.x; i < m; i += (long long)gridDim.x * HD_BLOCK) {
        asm volatile("" ::: "memory");      // (the staged weights stay in LDS, as in head_ce_fwd)
        const int j = idx ? idx[i] : (int)i;
        const int v = (unsigned)j < (unsigned)n ? p2v[j] : -1;
        if ((unsigned)v >= (unsigned)m_vox) {
            if (pred_all) pred_all[i] = 0;
            continue;
        }
        float f[C], z[NK], mx;
        int arg;
        hd_load_row<ESZ, C>(feats, v, f);
        hd_logits<C, NK>(w, b, n_cls, f, z, mx, arg);
        if (pred_all) pred_all[i] = (uint8_t)arg;
        const long long lab = labels[i];
        if (lab == ignore_index || lab < 0 || lab >= n_cls) continue;
        float s = 0.f, zy = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            s += expf(z[k] - mx);           // (padding classes: exp(-inf) = 0)
            zy = (int)lab == k ? z[k] : zy;
        }
        loss += (double)((mx + logf(s)) - zy);
        cnt += 1.0;
        if (arg == (int)lab) atomicAdd(&h[0][arg], 1u);
        atomicAdd(&h[1][arg], 1u);
        atomicAdd(&h[2][(int)lab], 1u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { loss += __shfl_xor(loss, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = loss; red[1][threadIdx.x >> 6] = cnt; }
    doda_sync();
    if (threadIdx.x == 0) {
        double a = 0.0, c2 = 0.0;
        for (int q = 0; q < HD_BLOCK / 64; ++q) { a += red[0][q]; c2 += red[1][q]; }
        partial[2 * blockIdx.x] = a;
        partial[2 * blockIdx.x + 1] = c2;
    }
    for (int e = threadIdx.x; e < 3 * n_cls; e += HD_BLOCK) {
        const unsigned v = h[e / n_cls][e % n_cls];
        if (v) atomicAdd(hist + e, (unsigned long long)v);
    }
}

// out[0] = sum of the workgroups' loss sums, out[1] = valid points: strided per-thread sums, butterfly, the 16 waves in order
__global__ __launch_bounds__(1024) void eval_score_final(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
    __shared__ double red[2][16];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 1024) { a += partial[2 * k]; b += partial[2 * k + 1]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    doda_sync();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int q = 0; q < 16; ++q) { a += red[0][q]; b += red[1][q]; }
        out[0] = a;
        out[1] = b;
    }
}

int score_blocks(long long m) {
    long long nb = (m + HD_BLOCK * 4LL - 1) / (HD_BLOCK * 4LL);      // four points per thread: 1024 workgroups from 1 M points on
    if (nb > 2048) nb = 2048;
    return nb < 1 ? 1 : (int)nb;
}

// DODA_OK and *sc filled from the host array, or the status to return
int eval_scenes(const doda_eval_scene *scenes_h, int32_t nbatch, long long n, long long m, EvalScenes *sc) {
    if (!scenes_h || nbatch < 1) return DODA_ERR_INVALID;
    if (nbatch > DODA_EVAL_MAX_SCENES) return DODA_ERR_UNSUPPORTED;
    sc->n = nbatch;
    long long n_prev = 0, m_prev = 0, cells = 0;
    for (int k = 0; k < nbatch; ++k) {
        const doda_eval_scene &s = scenes_h[k];
        if (s.n_end < n_prev || s.m_end < m_prev) return DODA_ERR_INVALID;
        if (s.n_end == n_prev && s.m_end > m_prev) return DODA_ERR_INVALID;      // queries with nothing to be near to
        long long prod = 1;
        for (int a = 0; a < 3; ++a) {
            if (s.dims[a] < 1 || s.dims[a] > DODA_EVAL_MAX_CELLS) return DODA_ERR_INVALID;
            prod *= s.dims[a];
            if (!(s.origin[a] - s.origin[a] == 0.f)) return DODA_ERR_INVALID;   // finite
        }
        if (prod > DODA_EVAL_MAX_CELLS || s.cell_base != cells) return DODA_ERR_INVALID;
        if (!(s.side > 0.f) || !(s.inv_side > 0.f) || !(s.side - s.side == 0.f) || !(s.inv_side - s.inv_side == 0.f))
            return DODA_ERR_INVALID;
        cells += prod;
        n_prev = s.n_end;
        m_prev = s.m_end;
        sc->s[k] = s;
    }
    if (n_prev != n || m_prev != m || cells > 0x7fffffffLL - 1) return DODA_ERR_INVALID;
    return DODA_OK;
}
}  // namespace

extern "C" int32_t doda_eval_abi_version(void) { return DODA_EVAL_ABI_VERSION; }

extern "C" int doda_eval_nn(const float *xyz_sorted, const int32_t *order, int64_t n, const int32_t *cell_start,
                            const doda_eval_scene *scenes_h, int32_t nbatch, const float *new_xyz, const int32_t *qorder, int64_t m,
                            int32_t *idx, float *dist2, doda_stream_t stream) {
    if (n < 0 || m < 0) return DODA_ERR_INVALID;
    if (n > 0x7fffffffLL || m > 0x7fffffffLL) return DODA_ERR_UNSUPPORTED;      // index arithmetic in n and m is int32
    EvalScenes sc;
    const int st = eval_scenes(scenes_h, nbatch, n, m, &sc);
    if (st != DODA_OK) return st;
    if (m == 0) return DODA_OK;
    if (!xyz_sorted || !order || !cell_start || !new_xyz || !idx || !dist2) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(eval_nn, dim3(div_up(m, EV_BLOCK)), dim3(EV_BLOCK), 0, as_stream(stream), sc, xyz_sorted, order, cell_start,
                       new_xyz, qorder, (int)m, idx, dist2);
    return doda_check_launch();
}

extern "C" int32_t doda_eval_score_blocks(int64_t m) { return score_blocks(m > 0 ? m : 1); }

extern "C" int doda_eval_score(const void *feats, int32_t m_vox, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                               int32_t n_cls, const int32_t *p2v, int64_t n, const int32_t *idx, const int64_t *labels_all, int64_t m,
                               int64_t ignore_index, uint8_t *pred_all, int64_t *hist, double *out, double *partial_ws,
                               int32_t n_blocks, doda_stream_t stream) {
    if (n < 0 || m < 0 || !out || !hist) return DODA_ERR_INVALID;
    if (n > 0x7fffffffLL || m > 0x7fffffffLL) return DODA_ERR_UNSUPPORTED;
    if (hd_args_bad(m_vox, elem_bytes, 1, {weight, partial_ws}) || (!idx && m != n)) return DODA_ERR_INVALID;
    if ((c != 16 && c != 32) || n_cls < 2 || n_cls > DODA_EVAL_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    if (m == 0) { (void)hipMemsetAsync(out, 0, 2 * sizeof(double), s); return DODA_OK; }
    if (!feats || !p2v || !labels_all) return DODA_ERR_INVALID;
    if (n_blocks != score_blocks(m)) return DODA_ERR_WORKSPACE;
    if (c == 16)
        HD_DISPATCH(eval_score, 16, n_blocks, feats, m_vox, weight, bias, n_cls, p2v, (int)n, idx, (const long long *)labels_all, (int)m,
                    (long long)ignore_index, pred_all, (unsigned long long *)hist, partial_ws);
    else
        HD_DISPATCH(eval_score, 32, n_blocks, feats, m_vox, weight, bias, n_cls, p2v, (int)n, idx, (const long long *)labels_all, (int)m,
                    (long long)ignore_index, pred_all, (unsigned long long *)hist, partial_ws);
    hipLaunchKernelGGL(eval_score_final, dim3(1), dim3(1024), 0, s, (const double *)partial_ws, n_blocks, out);
    return doda_check_launch();
}

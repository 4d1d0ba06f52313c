// The per-sample augmentation pipeline DATA_AUG.aug_list = [scene_aug, elastic, crop] on the device (include/doda_aug.h).
//
// reference dataset/augmentor/data_augmentor.py:171-230 and augmentor_utils.py:61-104,449-472 run per sample in DataLoader workers:
// a 3x3 matmul, two elastic passes (scipy.ndimage.convolve x 6 on three random grids, scipy's RegularGridInterpolator per point), the
// subtraction of the minimum and the crop loop of boolean masks.  Here the scenes of a batch are SEGMENTS of one array
// (segments.hpp: chunks of DODA_AUG_CHUNK points, one workgroup each, the offsets as validated launch arguments), the coordinates
// live in an fp64 [N][3] array `pos` from the affine step to the emit step, and the host decides everything random from a few
// bytes per segment (doda_amd.aug).
//
// Precision: every coordinate operation is the reference's fp64 operation in the reference's order (the library is compiled with
// -ffp-contract=off), so a truncated voxel coordinate differs from the reference's only where BLAS's fused dot product or scipy's
// summation differs in the last bits AND the value sits on an integer.  The blur accumulates three taps in fp64 and rounds to fp32
// per pass, as scipy.ndimage does for fp32 input.
//
// Order and determinism: outputs keep the points' order by segments.hpp's stable compaction over blk_cnt, the per-chunk counts the
// crop pass stored.  Bounds are min / max (exact in any order); counts and the coordinate maximum are integer atomics.
#include "segments.hpp"
#include "../../include/doda_aug.h"

static_assert(DODA_AUG_CHUNK == SEG_CHUNK, "include/doda_aug.h promises the chunk size of segments.hpp");

namespace {
using AugSegs = Segs<DODA_AUG_MAX_SEGMENTS>;

struct AugGrids {                                        // launch argument: the noise grids of the segments
    int32_t bb[DODA_AUG_MAX_SEGMENTS][3];
    int32_t base[DODA_AUG_MAX_SEGMENTS + 1];             // first cell of segment s's three grids; base[n] = all cells
    double gran[DODA_AUG_MAX_SEGMENTS];
    double mag[DODA_AUG_MAX_SEGMENTS];
};

struct AugOut {                                          // launch argument of the emit kernel
    long long base[DODA_AUG_MAX_SEGMENTS];
    int32_t use_valid[DODA_AUG_MAX_SEGMENTS];
};

// bb_h [n_seg][3] -> g->bb / g->base; a segment has a grid (all three > 0, at least 2 per axis) or none (0 0 0)
int make_grids(const int32_t *bb_h, int32_t n_seg, AugGrids *g) {
    if (!bb_h || n_seg < 1) return DODA_ERR_INVALID;
    if (n_seg > DODA_AUG_MAX_SEGMENTS) return DODA_ERR_UNSUPPORTED;
    long long at = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int32_t *b = bb_h + 3 * s;
        g->base[s] = (int32_t)at;
        g->gran[s] = g->mag[s] = 0.0;
        for (int k = 0; k < 3; ++k) g->bb[s][k] = b[k];
        if (b[0] == 0 && b[1] == 0 && b[2] == 0) continue;
        if (b[0] < 2 || b[1] < 2 || b[2] < 2) return DODA_ERR_INVALID;
        const long long cells = (long long)b[0] * b[1] * b[2];
        if (b[0] > DODA_AUG_MAX_GRID_CELLS || b[1] > DODA_AUG_MAX_GRID_CELLS || (long long)b[0] * b[1] > DODA_AUG_MAX_GRID_CELLS ||
            cells > DODA_AUG_MAX_GRID_CELLS)
            return DODA_ERR_UNSUPPORTED;
        at += 3 * cells;
        if (at > 0x7fffffffLL) return DODA_ERR_UNSUPPORTED;
    }
    g->base[n_seg] = (int32_t)at;
    return DODA_OK;
}

// xyz[i] @ m (row-major 3x3), the fp32 point widened: (x0 * m0k + x1 * m1k) + x2 * m2k
__device__ __forceinline__ void point_matmul(const float *__restrict__ xyz, int i, const double *m, double out[3]) {
    const double x0 = (double)xyz[(size_t)i * 3], x1 = (double)xyz[(size_t)i * 3 + 1], x2 = (double)xyz[(size_t)i * 3 + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (x0 * m[k] + x1 * m[3 + k]) + x2 * m[6 + k];
}

__global__ __launch_bounds__(SEG_BLOCK) void aug_affine(const float *__restrict__ xyz, AugSegs s, const double *__restrict__ mat,
                                                      double scale, double *__restrict__ pos, double *__restrict__ part) {
    __shared__ double sh[SEG_WAVES][6];
    __shared__ double m[9];
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x < 9) m[threadIdx.x] = mat[ch.seg * 9 + threadIdx.x];
    doda_sync();
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        double p[3];
        point_matmul(xyz, i, m, p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = p[k] * scale;
            pos[(size_t)i * 3 + k] = v;
            lo[k] = fmin(lo[k], v);
            hi[k] = fmax(hi[k], v);
        }
    }
    doda_sync();
    block_minmax(lo, hi, sh, part + (size_t)blockIdx.x * 6);
}

// one workgroup per segment: its chunks' partial bounds -> bounds[seg] (with use_grids, a segment without a grid is left alone)
__global__ __launch_bounds__(SEG_BLOCK) void aug_bounds_final(AugSegs s, AugGrids g, int use_grids, const double *__restrict__ part,
                                                            double *__restrict__ bounds) {
    __shared__ double sh[SEG_WAVES][6];
    const int seg = blockIdx.x;
    if (use_grids && g.bb[seg][0] == 0) return;
    segment_minmax(s, seg, part, sh, bounds);
}

// one box pass along `axis` over every cell of every grid of the batch
__global__ __launch_bounds__(SEG_BLOCK) void aug_blur_pass(const float *__restrict__ in, float *__restrict__ out, AugGrids g, int n_seg,
                                                         int axis) {
    const int t = blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (t >= g.base[n_seg]) return;
    int seg = 0;
    for (int k = 1; k < n_seg; ++k)
        if (t >= g.base[k]) seg = k;                     // (a segment without a grid has base[k] == base[k + 1]: the later one wins)
    const int b0 = g.bb[seg][0], b1 = g.bb[seg][1], b2 = g.bb[seg][2];
    const int c = (t - g.base[seg]) % (b0 * b1 * b2);
    int idx, len, stride;
    if (axis == 0) { idx = c / (b1 * b2); len = b0; stride = b1 * b2; }
    else if (axis == 1) { idx = (c / b2) % b1; len = b1; stride = b2; }
    else { idx = c % b2; len = b2; stride = 1; }
    const double w = (double)(1.0f / 3.0f);
    double acc = 0.0;
    acc += (idx > 0 ? (double)in[t - stride] : 0.0) * w;
    acc += (double)in[t] * w;
    acc += (idx + 1 < len ? (double)in[t + stride] : 0.0) * w;
    out[t] = (float)acc;
}

// interval of x on the axis a0, a0 + step, ..., a0 + (b - 1) step: i in [0, b - 2] with axis[i] <= x < axis[i + 1] (the ends
// clamped), t = (x - axis[i]) / (axis[i + 1] - axis[i]); false when x lies outside the axis
__device__ __forceinline__ bool axis_interval(double x, double a0, double step, int b, int *i_out, double *t_out) {
    const double last = a0 + (double)(b - 1) * step;
    if (!(x >= a0) || !(x <= last)) return false;
    int i = (int)floor((x - a0) / step);
    i = i < 0 ? 0 : (i > b - 2 ? b - 2 : i);
    if (i > 0 && x < a0 + (double)i * step) --i;
    else if (i < b - 2 && x >= a0 + (double)(i + 1) * step) ++i;
    const double gi = a0 + (double)i * step, gn = a0 + (double)(i + 1) * step;
    *i_out = i;
    *t_out = (x - gi) / (gn - gi);
    return true;
}

__global__ __launch_bounds__(SEG_BLOCK) void aug_displace(double *__restrict__ pos, AugSegs s, const float *__restrict__ noise,
                                                        AugGrids g, double *__restrict__ part) {
    __shared__ double sh[SEG_WAVES][6];
    const Chunk ch = chunk_of_block(s);
    const int b0 = g.bb[ch.seg][0], b1 = g.bb[ch.seg][1], b2 = g.bb[ch.seg][2];
    if (b0 == 0) return;                                 // (uniform over the workgroup: no elastic pass for this segment)
    const double gran = g.gran[ch.seg], mag = g.mag[ch.seg], step = 2.0 * gran;
    const int bb[3] = {b0, b1, b2};
    const int cells = b0 * b1 * b2;
    const float *grid = noise + g.base[ch.seg];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        double x[3], t[3];
        int ix[3];
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = pos[(size_t)i * 3 + k];
            inside = axis_interval(x[k], -(double)(bb[k] - 1) * gran, step, bb[k], &ix[k], &t[k]) && inside;
        }
        double gv[3] = {0.0, 0.0, 0.0};
        if (inside) {
            // scipy's _evaluate_linear: corners in the order of itertools.product (last axis fastest), weight ((1 * w0) * w1) * w2
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int d0 = c >> 2, d1 = (c >> 1) & 1, d2 = c & 1;
                const double wgt = ((d0 ? t[0] : 1.0 - t[0]) * (d1 ? t[1] : 1.0 - t[1])) * (d2 ? t[2] : 1.0 - t[2]);
                const int cell = ((ix[0] + d0) * b1 + (ix[1] + d1)) * b2 + (ix[2] + d2);
#pragma unroll
                for (int k = 0; k < 3; ++k) gv[k] = gv[k] + (double)grid[(size_t)k * cells + cell] * wgt;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double v = x[k] + gv[k] * mag;
            pos[(size_t)i * 3 + k] = v;
            lo[k] = fmin(lo[k], v);
            hi[k] = fmax(hi[k], v);
        }
    }
    block_minmax(lo, hi, sh, part + (size_t)blockIdx.x * 6);
}

__global__ __launch_bounds__(SEG_BLOCK) void aug_crop(const double *__restrict__ pos, AugSegs s, const double *__restrict__ par,
                                                    uint8_t *__restrict__ valid, int32_t *__restrict__ count,
                                                    int32_t *__restrict__ blk_cnt) {
    __shared__ double p[10];
    __shared__ int kept;
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x < 10) p[threadIdx.x] = par[ch.seg * 10 + threadIdx.x];
    if (threadIdx.x == 0) kept = 0;
    doda_sync();
    if (p[9] == 0.0) return;                             // (uniform over the workgroup: this segment is not tested)
    const bool first = p[9] > 1.0;
    int mine = 0;
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        bool t = first || valid[i] != 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double q = (pos[(size_t)i * 3 + k] - p[k]) + p[3 + k];
            t = t && q >= 0.0 && q < p[6 + k];
        }
        valid[i] = t ? 1 : 0;
        mine += t ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane_id() == 0 && mine) atomicAdd(&kept, mine);
    doda_sync();
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = kept;
        if (kept) atomicAdd(&count[ch.seg], kept);
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void aug_emit(const float *__restrict__ xyz, const double *__restrict__ pos,
                                                    const int32_t *__restrict__ labels, const uint8_t *__restrict__ mask1,
                                                    const uint8_t *__restrict__ mask2, AugSegs s, AugOut o,
                                                    const double *__restrict__ mat, double feat_scale, const double *__restrict__ par,
                                                    const uint8_t *__restrict__ valid, const int32_t *__restrict__ blk_cnt, int batch0,
                                                    int32_t *__restrict__ out_locs, float *__restrict__ out_float,
                                                    int32_t *__restrict__ out_labels, uint8_t *__restrict__ out_mask1,
                                                    uint8_t *__restrict__ out_mask2, int32_t *__restrict__ top, long long out_len) {
    __shared__ double p[6];
    __shared__ double m[9];
    __shared__ Compact cp;
    __shared__ int tmax[3];
    const Chunk ch = chunk_of_block(s);
    const bool use_valid = o.use_valid[ch.seg] != 0;
    if (threadIdx.x < 6) p[threadIdx.x] = par[ch.seg * 10 + threadIdx.x];
    if (threadIdx.x < 9) m[threadIdx.x] = mat[ch.seg * 9 + threadIdx.x];
    if (threadIdx.x < 3) tmax[threadIdx.x] = 0;
    compact_init(cp, ch, use_valid);
    doda_sync();
    // rows kept in the earlier chunks of this segment: their counts
    const size_t first = blockIdx.x - ch.index;
    int run = compact_before(cp, use_valid, ch.index, [&](int b) { return blk_cnt[first + b]; });
    int mx[3] = {0, 0, 0};
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int i = ch.base + r * SEG_BLOCK + threadIdx.x;
        compact_round(cp, run, i < ch.end && (!use_valid || valid[i] != 0), [&](int rank) {
            const long long row = o.base[ch.seg] + rank;
            if (row < 0 || row >= out_len) return;
            double mid[3];
            if (feat_scale == 0.0) point_matmul(xyz, i, m, mid);
            out_locs[(size_t)row * 4] = batch0 + ch.seg;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double x = pos[(size_t)i * 3 + k];
                const int q = (int)((x - p[k]) + p[3 + k]);              // truncation, as the reference's .long()
                out_locs[(size_t)row * 4 + 1 + k] = q;
                mx[k] = q + 1 > mx[k] ? q + 1 : mx[k];
                out_float[(size_t)row * 3 + k] = (float)(feat_scale != 0.0 ? x / feat_scale : mid[k]);
            }
            out_labels[row] = labels[i];
            if (mask1) { out_mask1[row] = mask1[i]; out_mask2[row] = mask2[i]; }
        });
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int v = __shfl_xor(mx[k], d, 64); mx[k] = v > mx[k] ? v : mx[k]; }
        if (lane_id() == 0 && mx[k] > 0) atomicMax(&tmax[k], mx[k]);
    }
    doda_sync();
    if (threadIdx.x < 3 && tmax[threadIdx.x] > 0) atomicMax(&top[threadIdx.x], tmax[threadIdx.x]);
}
}  // namespace

extern "C" int32_t doda_aug_abi_version(void) { return DODA_AUG_ABI_VERSION; }

extern "C" int64_t doda_aug_blocks(const int64_t *offsets_h, int32_t n_seg) {
    AugSegs s;
    if (make_segs(offsets_h, n_seg, &s) != DODA_OK) return -1;
    return s.blk[n_seg];
}

extern "C" int doda_aug_affine(const float *xyz, const int64_t *offsets_h, int32_t n_seg, const double *mat, double scale, double *pos,
                               double *part, double *bounds, doda_stream_t stream) {
    AugSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!mat || !bounds || !(scale > 0.0)) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb > 0) {
        if (!xyz || !pos || !part) return DODA_ERR_INVALID;
        hipLaunchKernelGGL(aug_affine, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, s, mat, scale, pos, part);
    }
    AugGrids g = {};
    hipLaunchKernelGGL(aug_bounds_final, dim3(n_seg), dim3(SEG_BLOCK), 0, as_stream(stream), s, g, 0, (const double *)part, bounds);
    return doda_check_launch();
}

extern "C" int doda_aug_blur(float *noise, float *tmp, const int32_t *bb_h, int32_t n_seg, doda_stream_t stream) {
    AugGrids g = {};
    const int st = make_grids(bb_h, n_seg, &g);
    if (st != DODA_OK) return st;
    const int total = g.base[n_seg];
    if (total == 0) return DODA_OK;
    if (!noise || !tmp) return DODA_ERR_INVALID;
    float *a = noise, *b = tmp;
    for (int pass = 0; pass < 6; ++pass) {
        hipLaunchKernelGGL(aug_blur_pass, dim3(div_up(total, SEG_BLOCK)), dim3(SEG_BLOCK), 0, as_stream(stream), (const float *)a, b, g,
                           (int)n_seg, pass % 3);
        float *t = a; a = b; b = t;
    }
    return doda_check_launch();
}

extern "C" int doda_aug_displace(double *pos, const int64_t *offsets_h, int32_t n_seg, const float *noise, const int32_t *bb_h,
                                 const double *gran_mag_h, double *part, double *bounds, doda_stream_t stream) {
    AugSegs s;
    int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    AugGrids g = {};
    st = make_grids(bb_h, n_seg, &g);
    if (st != DODA_OK) return st;
    if (!gran_mag_h || !bounds) return DODA_ERR_INVALID;
    for (int k = 0; k < n_seg; ++k) {
        g.gran[k] = gran_mag_h[2 * k];
        g.mag[k] = gran_mag_h[2 * k + 1];
        if (g.bb[k][0] > 0 && !(g.gran[k] > 0.0)) return DODA_ERR_INVALID;
    }
    const int nb = s.blk[n_seg];
    if (g.base[n_seg] == 0) return DODA_OK;
    if (nb > 0) {
        if (!pos || !noise || !part) return DODA_ERR_INVALID;
        hipLaunchKernelGGL(aug_displace, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), pos, s, noise, g, part);
    }
    hipLaunchKernelGGL(aug_bounds_final, dim3(n_seg), dim3(SEG_BLOCK), 0, as_stream(stream), s, g, 1, (const double *)part, bounds);
    return doda_check_launch();
}

extern "C" int doda_aug_crop(const double *pos, const int64_t *offsets_h, int32_t n_seg, const double *par, uint8_t *valid,
                             int32_t *count, int32_t *blk_cnt, doda_stream_t stream) {
    AugSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!pos || !par || !valid || !count || !blk_cnt) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(aug_crop, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), pos, s, par, valid, count, blk_cnt);
    return doda_check_launch();
}

extern "C" int doda_aug_emit(const float *xyz, const double *pos, const int32_t *labels, const uint8_t *mask1, const uint8_t *mask2,
                             const int64_t *offsets_h, int32_t n_seg, const double *mat, double feat_scale, const double *par,
                             const uint8_t *valid, const int32_t *blk_cnt, const int32_t *seg_valid_h, const int64_t *out_base_h,
                             int32_t batch0, int32_t *out_locs, float *out_float, int32_t *out_labels, uint8_t *out_mask1,
                             uint8_t *out_mask2, int32_t *top, int64_t out_len, doda_stream_t stream) {
    AugSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!seg_valid_h || !out_base_h || out_len < 0 || feat_scale < 0.0 || batch0 < 0) return DODA_ERR_INVALID;
    if ((mask1 == nullptr) != (mask2 == nullptr) || (mask1 == nullptr) != (out_mask1 == nullptr) ||
        (mask1 == nullptr) != (out_mask2 == nullptr) || (valid == nullptr) != (blk_cnt == nullptr))
        return DODA_ERR_INVALID;
    AugOut o = {};
    for (int k = 0; k < n_seg; ++k) {
        if (out_base_h[k] < 0) return DODA_ERR_INVALID;
        if (seg_valid_h[k] != 0 && !valid) return DODA_ERR_INVALID;
        o.base[k] = out_base_h[k];
        o.use_valid[k] = seg_valid_h[k] != 0;
    }
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !pos || !labels || !mat || !par || !out_locs || !out_float || !out_labels || !top) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(aug_emit, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, pos, labels, mask1, mask2, s, o, mat, feat_scale,
                       par, valid, blk_cnt, (int)batch0, out_locs, out_float, out_labels, out_mask1, out_mask2, top,
                       (long long)out_len);
    return doda_check_launch();
}

// Tail-aware cuboid mixing of the self-training stage (include/doda_mix.h): segment bounds, cuboid classification + statistics, the
// mixed sample's stable compaction + transform, and the extraction of tail-class cuboids for the queue.
//
// reference dataset/augmentor/augmentor_utils.py:255-445 cuts a target and a source scene into cuboids with numpy boolean masks (one
// pass over every point per cuboid and step), moves / shrinks the kept cuboids in place and concatenates them.  Here a batch of
// scenes is a batch of SEGMENTS of one array, cut into chunks of DODA_MIX_CHUNK points, one workgroup each (segments.hpp).
//
// Order and determinism: the outputs keep the points' order (the reference's boolean-mask order) by segments.hpp's stable
// compaction over blk_cnt, the per-(chunk, cuboid) counts the classify pass stored; mix_extract ranks per cuboid with the same
// arithmetic and counters of its own.  The statistics are integer sums (label counts, and coordinates as round(x * 2^28) in
// int64): exact, so the order in which workgroups add them does not show in any bit.
#include "segments.hpp"
#include "../../include/doda_mix.h"

static_assert(DODA_MIX_CHUNK == SEG_CHUNK, "include/doda_mix.h promises the chunk size of segments.hpp");

namespace {
constexpr int MX_C1 = DODA_MIX_MAX_CUBOIDS + 1;          // + the row of points that no cuboid holds
constexpr int MX_K1 = DODA_MIX_MAX_CLASSES + 1;          // + the bin of ignored labels
constexpr double MX_FIX = (double)(1 << DODA_MIX_FIXED_BITS);

using MixSegs = Segs<DODA_MIX_MAX_SEGMENTS>;

__global__ __launch_bounds__(SEG_BLOCK) void mix_bounds_part(const float *__restrict__ xyz, int stride, MixSegs s,
                                                            float *__restrict__ part) {
    __shared__ float sh[SEG_WAVES][6];
    const Chunk ch = chunk_of_block(s);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[(size_t)i * stride + k];
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    block_minmax(lo, hi, sh, part + (size_t)blockIdx.x * 6);
}

// one workgroup per segment: its chunks' partial bounds -> bounds[seg]
__global__ __launch_bounds__(SEG_BLOCK) void mix_bounds_final(MixSegs s, const float *__restrict__ part, float *__restrict__ bounds) {
    __shared__ float sh[SEG_WAVES][6];
    segment_minmax(s, (int)blockIdx.x, part, sh, bounds);
}

__global__ __launch_bounds__(SEG_BLOCK) void mix_classify(const float *__restrict__ xyz, const int32_t *__restrict__ labels, MixSegs s,
                                                        const float *__restrict__ centre, const double *__restrict__ planes, int n_cub,
                                                        int n_classes, uint8_t *__restrict__ cub, int64_t *__restrict__ stats,
                                                        int32_t *__restrict__ blk_cnt) {
    __shared__ double pl[DODA_MIX_MAX_CUBOIDS][6];
    __shared__ unsigned hist[MX_C1 * MX_K1];
    __shared__ unsigned long long sums[MX_C1 * 3];
    __shared__ float ctr[3];
    const Chunk ch = chunk_of_block(s);
    const int c1 = n_cub + 1, k1 = n_classes + 1;
    for (int e = threadIdx.x; e < n_cub * 6; e += SEG_BLOCK) pl[e / 6][e % 6] = planes[(size_t)ch.seg * n_cub * 6 + e];
    for (int e = threadIdx.x; e < c1 * k1; e += SEG_BLOCK) hist[e] = 0u;
    for (int e = threadIdx.x; e < c1 * 3; e += SEG_BLOCK) sums[e] = 0ull;
    if (threadIdx.x < 3) ctr[threadIdx.x] = centre[ch.seg * 3 + threadIdx.x];
    doda_sync();
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int i = ch.base + r * SEG_BLOCK + threadIdx.x;
        const bool valid = i < ch.end;
        int c = n_cub;
        long long fx[3] = {0, 0, 0};
        if (valid) {
            double x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float xc = xyz[(size_t)i * 3 + k] - ctr[k];       // fp32, as the reference's in-place subtraction
                x[k] = (double)xc;
                fx[k] = llrint(x[k] * MX_FIX);
            }
            int id = -1;
            for (int q = 0; q < n_cub; ++q) {                            // the later cuboid wins (augmentor_utils.py:372-374)
                const bool in = x[0] < pl[q][0] && x[1] < pl[q][1] && x[2] < pl[q][2] &&
                                x[0] >= pl[q][3] && x[1] >= pl[q][4] && x[2] >= pl[q][5];
                if (in) id = q;
            }
            cub[i] = id < 0 ? (uint8_t)255 : (uint8_t)id;
            if (id >= 0) c = id;
            const int lab = labels[i];
            atomicAdd(&hist[c * k1 + ((lab >= 0 && lab < n_classes) ? lab : n_classes)], 1u);
        }
        // coordinate sums: one LDS add per distinct cuboid of the wave (a chunk's points mostly share one)
        unsigned long long rem = __ballot(valid);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int c0 = __shfl(c, leader, 64);
            const bool mine = valid && c == c0;
            const unsigned long long m = __ballot(mine);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                long long v = mine ? fx[k] : 0ll;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
                if (lane_id() == leader) atomicAdd(&sums[c0 * 3 + k], (unsigned long long)v);
            }
            rem &= ~m;
        }
    }
    doda_sync();
    int64_t *out = stats + (size_t)ch.seg * c1 * (3 + k1);
    for (int e = threadIdx.x; e < c1 * k1; e += SEG_BLOCK) {
        const unsigned v = hist[e];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(out + (e / k1) * (3 + k1) + 3 + e % k1), (unsigned long long)v);
    }
    for (int e = threadIdx.x; e < c1 * 3; e += SEG_BLOCK) {
        const unsigned long long v = sums[e];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(out + (e / 3) * (3 + k1) + e % 3), v);
    }
    if (threadIdx.x < c1) {
        unsigned t = 0;
        for (int b = 0; b < k1; ++b) t += hist[threadIdx.x * k1 + b];
        blk_cnt[(size_t)blockIdx.x * c1 + threadIdx.x] = (int32_t)t;
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void mix_emit(const float *__restrict__ xyz, int stride, const int32_t *__restrict__ labels,
                                                    const uint8_t *__restrict__ cub, const int32_t *__restrict__ blk_cnt, MixSegs s,
                                                    int n_cub, const float *__restrict__ centre, const double *__restrict__ tab,
                                                    const double *__restrict__ seg_tab, float *__restrict__ out_xyz,
                                                    int32_t *__restrict__ out_labels, uint8_t *__restrict__ mask1,
                                                    uint8_t *__restrict__ mask2, long long out_len) {
    __shared__ double t[MX_C1][7];
    __shared__ double st[5];
    __shared__ float ctr[3];
    __shared__ Compact cp;
    const Chunk ch = chunk_of_block(s);
    const int c1 = n_cub + 1;
    for (int e = threadIdx.x; e < c1 * 7; e += SEG_BLOCK) t[e / 7][e % 7] = tab[(size_t)ch.seg * c1 * 7 + e];
    if (threadIdx.x < 5) st[threadIdx.x] = seg_tab[ch.seg * 5 + threadIdx.x];
    if (threadIdx.x < 3) ctr[threadIdx.x] = centre ? centre[ch.seg * 3 + threadIdx.x] : 0.f;
    compact_init(cp, ch, cub != nullptr);
    doda_sync();
    // rows kept in the earlier chunks of this segment: their (chunk, cuboid) counts of the kept cuboids
    const size_t first = (size_t)(blockIdx.x - ch.index) * c1;
    int run = compact_before(cp, cub != nullptr, ch.index * c1, [&](int p) { return t[p % c1][0] != 0.0 ? blk_cnt[first + p] : 0; });
    const long long out_base = (long long)st[3];
    const uint8_t m1 = st[4] != 0.0 ? 1 : 0;
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int i = ch.base + r * SEG_BLOCK + threadIdx.x;
        const bool valid = i < ch.end;
        int c = 0;
        if (valid && cub) { c = cub[i]; if (c > n_cub) c = n_cub; }
        compact_round(cp, run, valid && t[c][0] != 0.0, [&](int row) {
            const long long o = out_base + row;
            if (o < 0 || o >= out_len) return;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float x = xyz[(size_t)i * stride + k];
                if (centre) x = x - ctr[k];
                x = (float)((double)x + t[c][1 + k]);
                x = (float)((double)x + t[c][4 + k]);
                x = (float)((double)x - st[k]);
                out_xyz[(size_t)o * 3 + k] = x;
            }
            out_labels[o] = labels ? labels[i] : (int32_t)xyz[(size_t)i * stride + 3];
            mask1[o] = m1;
            mask2[o] = (uint8_t)(1 - m1);
        });
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void mix_extract(const float *__restrict__ xyz, const int32_t *__restrict__ labels,
                                                       const uint8_t *__restrict__ cub, const int32_t *__restrict__ blk_cnt, MixSegs s,
                                                       int n_cub, const float *__restrict__ centre, const int64_t *__restrict__ ex_base,
                                                       float *__restrict__ out_rows, long long out_len) {
    __shared__ long long base[MX_C1];
    __shared__ int run[MX_C1];
    __shared__ int wcnt[SEG_WAVES][MX_C1];
    __shared__ float ctr[3];
    const Chunk ch = chunk_of_block(s);
    const int c1 = n_cub + 1;
    if (threadIdx.x < c1) { base[threadIdx.x] = ex_base[(size_t)ch.seg * c1 + threadIdx.x]; run[threadIdx.x] = 0; }
    for (int e = threadIdx.x; e < SEG_WAVES * MX_C1; e += SEG_BLOCK) wcnt[e / MX_C1][e % MX_C1] = 0;
    if (threadIdx.x < 3) ctr[threadIdx.x] = centre[ch.seg * 3 + threadIdx.x];
    doda_sync();
    {
        const int first = s.blk[ch.seg], pairs = (blockIdx.x - first) * c1;
        for (int p = threadIdx.x; p < pairs; p += SEG_BLOCK) {
            const int c = p % c1;
            if (base[c] >= 0) { const int v = blk_cnt[(size_t)first * c1 + p]; if (v) atomicAdd(&run[c], v); }
        }
        doda_sync();
    }
    const int w = threadIdx.x >> 6;
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int i = ch.base + r * SEG_BLOCK + threadIdx.x;
        const bool valid = i < ch.end;
        const int c = valid ? (int)cub[i] : 255;
        const bool want = valid && c < n_cub && base[c] >= 0;
        int rank = 0;
        unsigned long long rem = __ballot(want);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int c0 = __shfl(c, leader, 64);
            const bool mine = want && c == c0;
            const unsigned long long m = __ballot(mine);
            if (mine) rank = mask_rank(m);
            if (lane_id() == leader) wcnt[w][c0] = __popcll(m);
            rem &= ~m;
        }
        doda_sync();
        if (want) {
            int off = run[c];
            for (int v = 0; v < w; ++v) off += wcnt[v][c];
            const long long o = base[c] + off + rank;
            if (o >= 0 && o < out_len) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_rows[(size_t)o * 4 + k] = xyz[(size_t)i * 3 + k] - ctr[k];
                out_rows[(size_t)o * 4 + 3] = (float)labels[i];
            }
        }
        doda_sync();
        if (threadIdx.x < c1) {
            int tsum = 0;
            for (int v = 0; v < SEG_WAVES; ++v) { tsum += wcnt[v][threadIdx.x]; wcnt[v][threadIdx.x] = 0; }
            run[threadIdx.x] += tsum;
        }
        doda_sync();
    }
}
}  // namespace

extern "C" int32_t doda_mix_abi_version(void) { return DODA_MIX_ABI_VERSION; }

extern "C" int64_t doda_mix_blocks(const int64_t *offsets_h, int32_t n_seg) {
    MixSegs s;
    if (make_segs(offsets_h, n_seg, &s) != DODA_OK) return -1;
    return s.blk[n_seg];
}

extern "C" int doda_mix_bounds(const float *xyz, int32_t stride, const int64_t *offsets_h, int32_t n_seg, float *part, float *bounds,
                               doda_stream_t stream) {
    MixSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (stride != 3 && stride != 4) return DODA_ERR_UNSUPPORTED;
    if (!bounds) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb > 0) {
        if (!xyz || !part) return DODA_ERR_INVALID;
        hipLaunchKernelGGL(mix_bounds_part, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, (int)stride, s, part);
    }
    hipLaunchKernelGGL(mix_bounds_final, dim3(n_seg), dim3(SEG_BLOCK), 0, as_stream(stream), s, (const float *)part, bounds);
    return doda_check_launch();
}

extern "C" int doda_mix_classify(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, const float *centre,
                                 const double *planes, int32_t n_cub, int32_t n_classes, uint8_t *cub, int64_t *stats,
                                 int32_t *blk_cnt, doda_stream_t stream) {
    MixSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (n_cub < 1 || n_cub > DODA_MIX_MAX_CUBOIDS || n_classes < 1 || n_classes > DODA_MIX_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !labels || !centre || !planes || !cub || !stats || !blk_cnt) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(mix_classify, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, labels, s, centre, planes, (int)n_cub,
                       (int)n_classes, cub, stats, blk_cnt);
    return doda_check_launch();
}

extern "C" int doda_mix_emit(const float *xyz, int32_t stride, const int32_t *labels, const uint8_t *cub, const int32_t *blk_cnt,
                             const int64_t *offsets_h, int32_t n_seg, int32_t n_cub, const float *centre, const double *tab,
                             const double *seg_tab, float *out_xyz, int32_t *out_labels, uint8_t *mask1, uint8_t *mask2, int64_t out_len,
                             doda_stream_t stream) {
    MixSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (stride != 3 && stride != 4) return DODA_ERR_UNSUPPORTED;
    if (n_cub < 0 || n_cub > DODA_MIX_MAX_CUBOIDS) return DODA_ERR_UNSUPPORTED;
    if ((cub == nullptr) != (blk_cnt == nullptr) || (cub == nullptr) != (n_cub == 0)) return DODA_ERR_INVALID;
    if (!labels && stride != 4) return DODA_ERR_INVALID;
    if (out_len < 0) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !tab || !seg_tab || !out_xyz || !out_labels || !mask1 || !mask2) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(mix_emit, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, (int)stride, labels, cub, blk_cnt, s, (int)n_cub,
                       centre, tab, seg_tab, out_xyz, out_labels, mask1, mask2, (long long)out_len);
    return doda_check_launch();
}

extern "C" int doda_mix_extract(const float *xyz, const int32_t *labels, const uint8_t *cub, const int32_t *blk_cnt,
                                const int64_t *offsets_h, int32_t n_seg, int32_t n_cub, const float *centre, const int64_t *ex_base,
                                float *out_rows, int64_t out_len, doda_stream_t stream) {
    MixSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (n_cub < 1 || n_cub > DODA_MIX_MAX_CUBOIDS) return DODA_ERR_UNSUPPORTED;
    if (out_len < 0) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !labels || !cub || !blk_cnt || !centre || !ex_base || !out_rows) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(mix_extract, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, labels, cub, blk_cnt, s, (int)n_cub, centre,
                       ex_base, out_rows, (long long)out_len);
    return doda_check_launch();
}

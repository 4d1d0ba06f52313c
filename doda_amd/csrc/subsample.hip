// The random subsample of every training item under DATA_PROCESSOR.downsampling_scale (include/doda_subsample.h).
//
// reference dataset/s3dis.py:59-63, dataset/front3d.py:65 and dataset/dataset.py:73-77 draw per sample, in a DataLoader worker,
// np.sort(np.random.permutation(n)[:int(n / ds)]).  Here the scenes of a batch are SEGMENTS of one array (segments.hpp: chunks of
// DODA_SUBSAMPLE_CHUNK points, one workgroup each, the offsets as validated launch arguments) and the draw is an exact k-selection
// on a counter-based key (subsample_key.hpp) followed by segments.hpp's stable compaction:
//
//   sub_hist x 4   radix select of T = the k-th smallest key of the segment, 8 bits per pass from the top: a workgroup counts the
//                  digits of its chunk's keys that agree with the digits already chosen in an LDS histogram and adds it to the
//                  segment's counters; the digits already chosen are resolved by every workgroup from the earlier passes' counters
//                  (resolve: one 256-wide scan per pass), so nothing is read back and no pass is launched per segment;
//   sub_count      per chunk: points with key < T and points with key == T; the first chunk of a segment stores (T, r),
//                  r = k - (points below T) = how many of the equal points are kept;
//   sub_emit       a point is kept iff key < T, or key == T and fewer than r equal points precede it in its segment; its row is
//                  (kept in the earlier chunks) + (kept earlier in the chunk) — compact_before / compact_round with two running
//                  counts, the equal points and the kept points.
//
// The key is recomputed in every pass (ten Philox rounds, no memory traffic) instead of being stored.  Counters are integer atomics
// and no atomic decides an output row: the outputs are a function of the arguments alone.
#include "segments.hpp"
#include "subsample_key.hpp"
#include "../../include/doda_subsample.h"

static_assert(DODA_SUBSAMPLE_CHUNK == SEG_CHUNK, "include/doda_subsample.h promises the chunk size of segments.hpp");
static_assert(DODA_SUBSAMPLE_MAX_SEGMENTS >= 32, "a batch of 32 scenes is one call");

namespace {
using SubSegs = Segs<DODA_SUBSAMPLE_MAX_SEGMENTS>;
constexpr int SUB_BITS = DODA_SUBSAMPLE_RADIX_BITS, SUB_BINS = 1 << SUB_BITS, SUB_LEVELS = DODA_SUBSAMPLE_LEVELS;
static_assert(SUB_BINS == SEG_BLOCK, "resolve() scans one digit counter per thread");
static_assert(SUB_BITS * SUB_LEVELS == 32, "the passes cover the 32-bit key");

struct SubPar {                                          // launch argument: per segment
    int32_t k[DODA_SUBSAMPLE_MAX_SEGMENTS];              // points to keep
    int32_t base[DODA_SUBSAMPLE_MAX_SEGMENTS];           // first output row
    uint32_t seed_lo[DODA_SUBSAMPLE_MAX_SEGMENTS], seed_hi[DODA_SUBSAMPLE_MAX_SEGMENTS];
};

struct SubSel { uint32_t prefix, rem; };                 // the digits chosen so far; the rank (1-based) still to find among their keys
struct SubScan {                                         // in LDS, one per workgroup
    uint32_t wsum[SEG_WAVES];
    SubSel sel;
};

struct SubWs { uint32_t *hist, *thr; int32_t *blk_cnt; };   // [SUB_LEVELS][n_seg][SUB_BINS] | [n_seg][2] | [chunks][2]

size_t ws_layout(void *ws, int n_seg, int n_blk, SubWs *w) {
    uint32_t *p = (uint32_t *)ws;
    w->hist = p;
    w->thr = w->hist + (size_t)SUB_LEVELS * n_seg * SUB_BINS;
    w->blk_cnt = (int32_t *)(w->thr + (size_t)2 * n_seg);
    return ((size_t)SUB_LEVELS * n_seg * SUB_BINS + (size_t)2 * n_seg + (size_t)2 * n_blk) * sizeof(uint32_t);
}

__device__ __forceinline__ uint32_t key_of(const SubPar &p, const SubSegs &s, int seg, int i, uint32_t mask) {
    return subsample_key(p.seed_lo[seg], p.seed_hi[seg], (uint32_t)(i - s.off[seg])) & mask;
}

// By all threads (levels, k uniform over the workgroup, k >= 1): the digits of passes 0 .. levels - 1 and the rank that is left.
// Pass l's counters hold the segment's keys that agree with the digits of the passes before it, per digit; the digit taken is the
// one whose run of counts holds the rank.  Ends behind a barrier.
__device__ __forceinline__ SubSel resolve(const uint32_t *__restrict__ hist, int n_seg, int seg, int levels, uint32_t k, SubScan &sc) {
    SubSel cur = {0u, k};
    for (int l = 0; l < levels; ++l) {
        const uint32_t c = hist[((size_t)l * n_seg + seg) * SUB_BINS + threadIdx.x];
        const uint32_t inc = (uint32_t)wave_inclusive_sum((int)c);
        if (lane_id() == DODA_WAVE - 1) sc.wsum[threadIdx.x >> 6] = inc;
        if (threadIdx.x == 0) { sc.sel.prefix = cur.prefix << SUB_BITS; sc.sel.rem = 0u; }   // (counters that do not hold the rank: keep nothing)
        doda_sync();
        uint32_t excl = inc - c;
#pragma unroll
        for (int w = 0; w < SEG_WAVES; ++w)
            if (w < (int)(threadIdx.x >> 6)) excl += sc.wsum[w];
        if (c != 0u && excl < cur.rem && cur.rem <= excl + c) {
            sc.sel.prefix = (cur.prefix << SUB_BITS) | threadIdx.x;
            sc.sel.rem = cur.rem - excl;
        }
        doda_sync();
        cur = sc.sel;
        doda_sync();
    }
    return cur;
}

__global__ __launch_bounds__(SEG_BLOCK) void sub_hist(SubSegs s, SubPar p, uint32_t mask, int level, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[SUB_BINS];
    __shared__ SubScan sc;
    const Chunk ch = chunk_of_block(s);
    const int k = p.k[ch.seg];
    if (k == 0) return;                                  // (uniform over the workgroup: nothing to select)
    h[threadIdx.x] = 0u;
    const SubSel sel = resolve(hist, s.n, ch.seg, level, (uint32_t)k, sc);
    doda_sync();
    const int shift = 32 - SUB_BITS * (level + 1);
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        const uint32_t key = key_of(p, s, ch.seg, i, mask);
        if (level == 0 || (key >> (shift + SUB_BITS)) == sel.prefix) atomicAdd(&h[(key >> shift) & (SUB_BINS - 1)], 1u);
    }
    doda_sync();
    const uint32_t mine = h[threadIdx.x];
    if (mine) atomicAdd(&hist[((size_t)level * s.n + ch.seg) * SUB_BINS + threadIdx.x], mine);
}

__global__ __launch_bounds__(SEG_BLOCK) void sub_count(SubSegs s, SubPar p, uint32_t mask, const uint32_t *__restrict__ hist,
                                                     uint32_t *__restrict__ thr, int32_t *__restrict__ blk_cnt) {
    __shared__ SubScan sc;
    __shared__ int cnt[2];
    const Chunk ch = chunk_of_block(s);
    const int k = p.k[ch.seg];
    if (k == 0) {
        if (threadIdx.x < 2) blk_cnt[(size_t)blockIdx.x * 2 + threadIdx.x] = 0;
        return;
    }
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    const SubSel sel = resolve(hist, s.n, ch.seg, SUB_LEVELS, (uint32_t)k, sc);      // (its barriers publish cnt)
    int lt = 0, eq = 0;
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        const uint32_t key = key_of(p, s, ch.seg, i, mask);
        lt += key < sel.prefix ? 1 : 0;
        eq += key == sel.prefix ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lt += __shfl_xor(lt, d, 64); eq += __shfl_xor(eq, d, 64); }
    if (lane_id() == 0) {
        if (lt) atomicAdd(&cnt[0], lt);
        if (eq) atomicAdd(&cnt[1], eq);
    }
    doda_sync();
    if (threadIdx.x < 2) blk_cnt[(size_t)blockIdx.x * 2 + threadIdx.x] = cnt[threadIdx.x];
    if (ch.index == 0 && threadIdx.x == 0) { thr[ch.seg * 2] = sel.prefix; thr[ch.seg * 2 + 1] = sel.rem; }
}

__global__ __launch_bounds__(SEG_BLOCK) void sub_emit(const uint32_t *__restrict__ xyz, const int32_t *__restrict__ labels,
                                                    const int32_t *__restrict__ extra_i32, const uint8_t *__restrict__ extra_u8,
                                                    SubSegs s, SubPar p, uint32_t mask, const uint32_t *__restrict__ thr,
                                                    const int32_t *__restrict__ blk_cnt, uint32_t *__restrict__ out_xyz,
                                                    int32_t *__restrict__ out_labels, int32_t *__restrict__ out_idx,
                                                    int32_t *__restrict__ out_extra_i32, uint8_t *__restrict__ out_extra_u8) {
    __shared__ Compact kept, equal;
    const Chunk ch = chunk_of_block(s);
    const int k = p.k[ch.seg];
    if (k == 0) return;                                  // (uniform over the workgroup)
    const uint32_t T = thr[ch.seg * 2];
    const int r = (int)thr[ch.seg * 2 + 1];
    compact_init(kept, ch, true);
    compact_init(equal, ch, true);
    doda_sync();
    // the earlier chunks of this segment: their points below T, their points equal to T (of which the first r are kept)
    const size_t first = blockIdx.x - ch.index;
    const int lt_before = compact_before(kept, true, ch.index, [&](int b) { return blk_cnt[(first + b) * 2]; });
    int run_eq = compact_before(equal, true, ch.index, [&](int b) { return blk_cnt[(first + b) * 2 + 1]; });
    int run = lt_before + (run_eq < r ? run_eq : r);
    const bool ties = blk_cnt[(size_t)blockIdx.x * 2 + 1] != 0;      // (uniform: most chunks hold no point with key == T)
    const size_t base = (size_t)p.base[ch.seg];
    for (int rd = 0; rd < SEG_ROUNDS; ++rd) {
        const int i = ch.base + rd * SEG_BLOCK + threadIdx.x;
        const bool in = i < ch.end;
        const uint32_t key = in ? key_of(p, s, ch.seg, i, mask) : 0u;
        bool keep = in && key < T;
        if (ties) compact_round(equal, run_eq, in && key == T, [&](int rank) { keep = rank < r; });
        compact_round(kept, run, keep, [&](int rank) {
            if (rank >= k) return;                       // (never with the counters of this call: no row outside the segment's k)
            const size_t row = base + rank;
#pragma unroll
            for (int c = 0; c < 3; ++c) out_xyz[row * 3 + c] = xyz[(size_t)i * 3 + c];
            out_labels[row] = labels[i];
            out_idx[row] = i - s.off[ch.seg];
            if (extra_i32) out_extra_i32[row] = extra_i32[i];
            if (extra_u8) out_extra_u8[row] = extra_u8[i];
        });
    }
}
}  // namespace

extern "C" int32_t doda_subsample_abi_version(void) { return DODA_SUBSAMPLE_ABI_VERSION; }

extern "C" size_t doda_subsample_workspace_bytes(const int64_t *offsets_h, int32_t n_seg) {
    SubSegs s;
    if (make_segs(offsets_h, n_seg, &s) != DODA_OK) return 0;
    SubWs w;
    return ws_layout(nullptr, n_seg, s.blk[n_seg], &w);
}

extern "C" int doda_subsample_draw(const float *xyz, const int32_t *labels, const int32_t *extra_i32, const uint8_t *extra_u8,
                                   const int64_t *offsets_h, int32_t n_seg, const int32_t *k_h, const uint64_t *seeds_h,
                                   uint32_t key_mask, float *out_xyz, int32_t *out_labels, int32_t *out_idx, int32_t *out_extra_i32,
                                   uint8_t *out_extra_u8, void *ws, size_t ws_bytes, doda_stream_t stream) {
    SubSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!k_h || !seeds_h) return DODA_ERR_INVALID;
    if ((extra_i32 == nullptr) != (out_extra_i32 == nullptr) || (extra_u8 == nullptr) != (out_extra_u8 == nullptr)) return DODA_ERR_INVALID;
    SubPar p = {};
    long long total = 0;
    for (int b = 0; b < n_seg; ++b) {
        if (k_h[b] < 0 || k_h[b] > s.off[b + 1] - s.off[b]) return DODA_ERR_INVALID;
        p.k[b] = k_h[b];
        p.base[b] = (int32_t)total;
        p.seed_lo[b] = (uint32_t)seeds_h[b];
        p.seed_hi[b] = (uint32_t)(seeds_h[b] >> 32);
        total += k_h[b];
    }
    if (total == 0) return DODA_OK;
    if (!xyz || !labels || !out_xyz || !out_labels || !out_idx || !ws || ((uintptr_t)ws & 3)) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    SubWs w;
    if (ws_bytes < ws_layout(ws, n_seg, nb, &w)) return DODA_ERR_WORKSPACE;
    hipStream_t hs = as_stream(stream);
    if (hipMemsetAsync(w.hist, 0, (size_t)SUB_LEVELS * n_seg * SUB_BINS * sizeof(uint32_t), hs) != hipSuccess) return DODA_ERR_LAUNCH;
    for (int level = 0; level < SUB_LEVELS; ++level)
        hipLaunchKernelGGL(sub_hist, dim3(nb), dim3(SEG_BLOCK), 0, hs, s, p, key_mask, level, w.hist);
    hipLaunchKernelGGL(sub_count, dim3(nb), dim3(SEG_BLOCK), 0, hs, s, p, key_mask, (const uint32_t *)w.hist, w.thr, w.blk_cnt);
    hipLaunchKernelGGL(sub_emit, dim3(nb), dim3(SEG_BLOCK), 0, hs, (const uint32_t *)xyz, labels, extra_i32, extra_u8, s, p, key_mask,
                       (const uint32_t *)w.thr, (const int32_t *)w.blk_cnt, (uint32_t *)out_xyz, out_labels, out_idx, out_extra_i32,
                       out_extra_u8);
    return doda_check_launch();
}

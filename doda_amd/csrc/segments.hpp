// Batches as SEGMENTS of one array, shared by the kernels that keep the points' order (mix.hip, aug.hip).  Internal: nothing here
// is exported, the C ABI of the callers is include/doda_mix.h and include/doda_aug.h.
//
// A segment is cut into chunks of SEG_CHUNK points, one workgroup of SEG_BLOCK threads each, and the segment offsets travel as a
// launch argument (Segs, validated on the host by make_segs: no kernel trusts a device table for its bounds).
//
// Bounds: per-chunk partial min / max (block_minmax), one combining workgroup per segment (segment_minmax); exact in any order.
//
// Stable compaction without a scan launch (Compact): a kept point's row is
//   rows kept in earlier chunks of its segment   (compact_before: from the per-chunk counts an earlier pass stored)
// + rows kept earlier in its chunk                (compact_round: wave ballot + popcount prefix, SEG_ROUNDS rounds of SEG_BLOCK points),
// so no atomic decides a position and the outputs keep the points' order.
#pragma once
#include "common.hpp"

constexpr int SEG_CHUNK = 1024;
constexpr int SEG_BLOCK = 256;
constexpr int SEG_WAVES = SEG_BLOCK / DODA_WAVE;
constexpr int SEG_ROUNDS = SEG_CHUNK / SEG_BLOCK;

template <int MAX_SEGMENTS>
struct Segs {                                            // launch argument: segment offsets and first chunk of every segment
    int32_t n;
    int32_t off[MAX_SEGMENTS + 1];
    int32_t blk[MAX_SEGMENTS + 1];
};

// DODA_OK and *s filled, or the status to return
template <int MAX_SEGMENTS>
int make_segs(const int64_t *offsets_h, int32_t n_seg, Segs<MAX_SEGMENTS> *s) {
    if (!offsets_h || n_seg < 1) return DODA_ERR_INVALID;
    if (n_seg > MAX_SEGMENTS) return DODA_ERR_UNSUPPORTED;
    if (offsets_h[0] != 0) return DODA_ERR_INVALID;
    s->n = n_seg;
    s->off[0] = 0;
    s->blk[0] = 0;
    for (int k = 0; k < n_seg; ++k) {
        const int64_t a = offsets_h[k], b = offsets_h[k + 1];
        if (b < a || b > 0x7fffffffLL) return DODA_ERR_INVALID;
        s->off[k + 1] = (int32_t)b;
        s->blk[k + 1] = s->blk[k] + (int32_t)((b - a + SEG_CHUNK - 1) / SEG_CHUNK);
    }
    return DODA_OK;
}

struct Chunk { int seg, index, base, end; };             // segment, chunk of the segment, first point, one past the last point

// the chunk of this workgroup (blockIdx.x < s.blk[s.n]: the grid is exactly the chunks)
template <int MAX_SEGMENTS>
__device__ __forceinline__ Chunk chunk_of_block(const Segs<MAX_SEGMENTS> &s) {
    const int b = blockIdx.x;
    int seg = 0;
    for (int k = 0; k < s.n; ++k)
        if (b >= s.blk[k + 1]) seg = k + 1;              // (empty segments have no chunk: skipped)
    if (seg >= s.n) seg = s.n - 1;
    Chunk c;
    c.seg = seg;
    c.index = b - s.blk[seg];
    c.base = s.off[seg] + c.index * SEG_CHUNK;
    const int end = c.base + SEG_CHUNK;
    c.end = end < s.off[seg + 1] ? end : s.off[seg + 1];
    return c;
}

// ------------------------------------------------------------------------------------------------ bounds
__device__ __forceinline__ float seg_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float seg_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double seg_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double seg_max(double a, double b) { return fmax(a, b); }

// min / max of 3 + 3 values (T = float, double) over the workgroup -> out[0..2] = min, out[3..5] = max, written by thread 0
template <typename T>
__device__ __forceinline__ void block_minmax(T lo[3], T hi[3], T (*sh)[6], T *__restrict__ out) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = seg_min(lo[k], __shfl_xor(lo[k], d, 64));
            hi[k] = seg_max(hi[k], __shfl_xor(hi[k], d, 64));
        }
    if (lane_id() == 0)
        for (int k = 0; k < 3; ++k) { sh[threadIdx.x >> 6][k] = lo[k]; sh[threadIdx.x >> 6][3 + k] = hi[k]; }
    doda_sync();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SEG_WAVES; ++w)
            for (int k = 0; k < 3; ++k) { lo[k] = seg_min(lo[k], sh[w][k]); hi[k] = seg_max(hi[k], sh[w][3 + k]); }
        for (int k = 0; k < 3; ++k) { out[k] = lo[k]; out[3 + k] = hi[k]; }
    }
}

// one workgroup for segment `seg`: its chunks' partial bounds part[chunk][6] -> bounds[seg][6]
template <typename T, int MAX_SEGMENTS>
__device__ __forceinline__ void segment_minmax(const Segs<MAX_SEGMENTS> &s, int seg, const T *__restrict__ part, T (*sh)[6],
                                               T *__restrict__ bounds) {
    T lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = s.blk[seg] + threadIdx.x; b < s.blk[seg + 1]; b += SEG_BLOCK)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = seg_min(lo[k], part[(size_t)b * 6 + k]);
            hi[k] = seg_max(hi[k], part[(size_t)b * 6 + 3 + k]);
        }
    block_minmax(lo, hi, sh, bounds + seg * 6);
}

// ------------------------------------------------------------------------------------------------ stable compaction
struct Compact {                                         // in LDS, one per workgroup
    int before;                                          // rows kept in the earlier chunks of the segment
    int wcnt[SEG_WAVES];                                 // rows kept per wave in the current round
};

// `counted` (uniform over the workgroup): only some points are kept and an earlier pass stored how many per chunk; otherwise every
// point is kept.  Thread 0 writes; the caller's next doda_sync() (the one that publishes its own LDS tables) publishes it.
__device__ __forceinline__ void compact_init(Compact &c, const Chunk &ch, bool counted) {
    if (threadIdx.x == 0) c.before = counted ? 0 : ch.index * SEG_CHUNK;
}

// After that barrier, by all threads: the rows kept before this chunk.  With `counted` it is the sum of kept_in(0 .. n - 1), the
// stored counts of the segment's earlier chunks.
template <typename F>
__device__ __forceinline__ int compact_before(Compact &c, bool counted, int n, F kept_in) {
    if (counted) {
        int local = 0;
        for (int p = threadIdx.x; p < n; p += SEG_BLOCK) local += kept_in(p);
        if (local) atomicAdd(&c.before, local);
        doda_sync();
    }
    return c.before;
}

// One round of SEG_BLOCK points, by all threads: emit(row) runs for the threads with `keep`, row = run + points kept by the
// lower threads of this round, and run advances by the round's kept points.  The second barrier keeps the next round's counts
// away from this round's readers.
template <typename F>
__device__ __forceinline__ void compact_round(Compact &c, int &run, bool keep, F emit) {
    const unsigned long long m = __ballot(keep);
    if (lane_id() == 0) c.wcnt[threadIdx.x >> 6] = __popcll(m);
    doda_sync();
    int off = run, total = 0;
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) {
        if (w < (int)(threadIdx.x >> 6)) off += c.wcnt[w];
        total += c.wcnt[w];
    }
    if (keep) emit(off + mask_rank(m));
    run += total;
    doda_sync();
}

// The rest of the reference's pointops2_cuda module (include/doda_pointops.h): furthest point sampling and the four operator pairs
// of the point backbone — grouping, interpolation, subtraction, aggregation.
//
// Order.  No float atomic: every scatter of the reference's backward kernels is a gather here.  doda_po_transpose turns
// idx [m][nsample] into one list of flat positions per destination (integer atomics count and fill, then every list is sorted
// ascending), and a backward kernel gives one thread one (destination, channel) element, which walks the list front to back.  All
// arithmetic is __fmul_rn / __fadd_rn / __fsub_rn: one rounding per operation, sums from +0 in the stated order, so the outputs can
// be compared bit for bit with a sequential restatement.
//
// Furthest point sampling is one dependent chain of m iterations per segment; what an iteration waits for is its whole cost.  One
// workgroup of 1024 threads (16 waves, 4 per SIMD: 128 VGPRs per lane) owns a segment.  A lane keeps its first DODA_PO_FPS_REG
// points — coordinates and running distance — in registers; only a segment above 1024 * DODA_PO_FPS_REG points streams its tail
// from xyz and the workspace.  The arg-max is one 64-bit key (float bits of the distance << 32 | ~index: the distance is >= +0, so
// unsigned order is float order, and the complement lets the lowest index win a tie), reduced inside a wave by DPP moves and
// between the waves through one LDS slot per wave.  The slots are double-buffered by iteration parity: a wave that runs ahead
// writes the other buffer, and it cannot reach the buffer of iteration s again before every wave has passed the barrier of
// iteration s + 1, i.e. has finished reading s.  So one barrier per sample remains.  The winning lane writes its point's
// coordinates beside its key; every wave takes the next centre from LDS, never from global memory.
#include "common.hpp"
#include "../../include/doda_pointops.h"

namespace {

constexpr int PO_BLOCK = 256;
constexpr int PO_MAX_GRID = 1 << 20;   // grid-stride above

typedef unsigned long long u64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------
// the index by destination
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PO_BLOCK) void po_count(const int *__restrict__ idx, int total, int n, int *__restrict__ count) {
    for (long long p = (long long)blockIdx.x * PO_BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * PO_BLOCK) {
        const int j = idx[p];
        if ((unsigned)j < (unsigned)n) atomicAdd(count + j, 1);
    }
}

// cursor[] is zero on entry; start[] holds the exclusive sums of the counts, so cursor[j] stays below j's list length.
__global__ __launch_bounds__(PO_BLOCK) void po_fill(const int *__restrict__ idx, int total, int n, const int *__restrict__ start,
                                                   int *__restrict__ cursor, int *__restrict__ pos) {
    for (long long p = (long long)blockIdx.x * PO_BLOCK + threadIdx.x; p < total; p += (long long)gridDim.x * PO_BLOCK) {
        const int j = idx[p];
        if ((unsigned)j >= (unsigned)n) continue;
        const long long at = (long long)start[j] + atomicAdd(cursor + j, 1);
        if (at >= 0 && at < total) pos[at] = (int)p;   // (always true after po_count over the same idx)
    }
}

// pos[s .. e) ascending by one wave: a bitonic network whose comparators all point the same way (first the mirror step of each
// stage, then the half-distance steps), so positions at and above the length behave as +inf without being stored.  The lanes hand
// the list to each other through memory between steps: workgroup-scope fences around a wave barrier.
__device__ __forceinline__ void wave_sort(int *pos, int s, int e) {
    const int len = e - s, lane = lane_id();
    int *a = pos + s;
    unsigned P = 1;
    while (P < (unsigned)len) P <<= 1;
    // Bound: log2(P) * (log2(P) + 1) / 2 steps of P / 128 iterations each.
    for (unsigned k = 2; k <= P; k <<= 1) {
        for (unsigned j = k >> 1; j >= 1; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (unsigned t = lane; t < (P >> 1); t += DODA_WAVE) {
                const unsigned lo = (t / j) * (2 * j) + (t % j);
                const unsigned hi = mirror ? ((lo & ~(k - 1)) + (k - 1) - (lo & (k - 1))) : lo + j;
                if (hi < (unsigned)len) {
                    const int x = a[lo], y = a[hi];
                    if (x > y) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

// One lane per destination for lists of up to DODA_PO_WAVE_LIST entries (insertion sort: the atomics of po_fill arrive nearly in
// order, so it is close to linear); the longer lists of a wave's destinations are then taken one at a time by the whole wave.
__global__ __launch_bounds__(PO_BLOCK) void po_sort_lists(const int *__restrict__ start, int n, int total, int *pos) {
    const int j = blockIdx.x * PO_BLOCK + threadIdx.x;
    int s = 0, e = 0;
    if (j < n) {
        s = clampi(start[j], 0, total);
        e = clampi(start[j + 1], s, total);
    }
    const bool wide = e - s > DODA_PO_WAVE_LIST;
    if (!wide) {
        for (int k = s + 1; k < e; ++k) {          // at most DODA_PO_WAVE_LIST - 1 steps
            const int v = pos[k];
            int q = k;
            while (q > s && pos[q - 1] > v) {       // at most k - s steps
                pos[q] = pos[q - 1];
                --q;
            }
            pos[q] = v;
        }
    }
    u64 todo = __ballot(wide);
    // Bound: one set bit of `todo` is cleared per iteration: at most 64.
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        wave_sort(pos, __shfl(s, src, 64), __shfl(e, src, 64));
    }
}

// ---------------------------------------------------------------------------------------------
// forwards: one thread per output element, channel fastest
// ---------------------------------------------------------------------------------------------
#define PO_FOR_ELEMENTS(e, total_elems) \
    for (long long e = (long long)blockIdx.x * PO_BLOCK + threadIdx.x; e < (total_elems); e += (long long)gridDim.x * PO_BLOCK)

// a row of the indexed array, or nullptr for an index outside it (which then reads as 0)
__device__ __forceinline__ const float *row_of(const float *__restrict__ x, int j, int n, int c) {
    return (unsigned)j < (unsigned)n ? x + (size_t)j * c : nullptr;
}

// The two forwards that only move rows (grouping, subtraction) take V = 4 channels per thread as one 16-byte access where c is a
// multiple of 4 and the arrays are 16-byte aligned, else V = 1; the values are the same either way.
template <int V> struct Chan { typedef float type; };
template <> struct Chan<4> { typedef float4 type; };

template <int V>
__global__ __launch_bounds__(PO_BLOCK) void po_grouping_fwd(const float *__restrict__ inp, const int *__restrict__ idx,
                                                           float *__restrict__ out, int n, long long elems, int c) {
    typedef typename Chan<V>::type T;
    const int cv = c / V;
    PO_FOR_ELEMENTS(e, elems) {                    // e counts groups of V channels
        const long long p = e / cv;
        const int g = (int)(e - p * cv);
        const float *row = row_of(inp, idx[p], n, c);
        T v = T();
        if (row) v = reinterpret_cast<const T *>(row)[g];
        reinterpret_cast<T *>(out)[e] = v;
    }
}

__global__ __launch_bounds__(PO_BLOCK) void po_interpolation_fwd(const float *__restrict__ inp, const int *__restrict__ idx,
                                                                const float *__restrict__ w, float *__restrict__ out, int n,
                                                                long long elems, int k, int c) {
    PO_FOR_ELEMENTS(e, elems) {
        const long long r = e / c;
        const int ch = (int)(e - r * c);
        float acc = 0.f;
        for (int i = 0; i < k; ++i) {
            const float *row = row_of(inp, idx[r * k + i], n, c);
            acc = __fadd_rn(acc, __fmul_rn(row ? row[ch] : 0.f, w[r * k + i]));
        }
        out[e] = acc;
    }
}

__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float4 sub_rn(float4 a, float4 b) {
    return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}

template <int V>
__global__ __launch_bounds__(PO_BLOCK) void po_subtraction_fwd(const float *__restrict__ a, const float *__restrict__ b,
                                                              const int *__restrict__ idx, float *__restrict__ out, int n,
                                                              long long elems, int nsample, int c) {
    typedef typename Chan<V>::type T;
    const int cv = c / V;
    PO_FOR_ELEMENTS(e, elems) {
        const long long p = e / cv;
        const int g = (int)(e - p * cv);
        const long long r = p / nsample;
        const float *row = row_of(b, idx[p], n, c);
        T v = T();
        if (row) v = reinterpret_cast<const T *>(row)[g];
        reinterpret_cast<T *>(out)[e] = sub_rn(reinterpret_cast<const T *>(a)[r * cv + g], v);
    }
}

__global__ __launch_bounds__(PO_BLOCK) void po_aggregation_fwd(const float *__restrict__ inp, const float *__restrict__ position,
                                                              const float *__restrict__ w, const int *__restrict__ idx,
                                                              float *__restrict__ out, int n, long long elems, int nsample, int c,
                                                              int w_c) {
    PO_FOR_ELEMENTS(e, elems) {
        const long long r = e / c;
        const int ch = (int)(e - r * c), wk = ch % w_c;
        float acc = 0.f;
        for (int i = 0; i < nsample; ++i) {
            const long long p = r * nsample + i;
            const float *row = row_of(inp, idx[p], n, c);
            acc = __fadd_rn(acc, __fmul_rn(__fadd_rn(row ? row[ch] : 0.f, position[p * c + ch]), w[p * w_c + wk]));
        }
        out[e] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// backwards
// ---------------------------------------------------------------------------------------------
enum { BWD_GROUPING = 0, BWD_INTERPOLATION = 1, BWD_SUBTRACTION = 2, BWD_AGGREGATION = 3 };

// d_inp[j][ch] = the sum over j's list, front to back, of the operator's term at position p.  g: the incoming gradient; w: the
// forward's weights (interpolation, aggregation); per: positions per gradient row (interpolation k, aggregation nsample).
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float4 add_rn(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float neg_of(float a) { return -a; }
__device__ __forceinline__ float4 neg_of(float4 a) { return make_float4(-a.x, -a.y, -a.z, -a.w); }
__device__ __forceinline__ float mul_rn(float a, float b, float, float, float) { return __fmul_rn(a, b); }
__device__ __forceinline__ float4 mul_rn(float4 a, float b0, float b1, float b2, float b3) {
    return make_float4(__fmul_rn(a.x, b0), __fmul_rn(a.y, b1), __fmul_rn(a.z, b2), __fmul_rn(a.w, b3));
}

// V channels per thread (4: one 16-byte load per list entry, as in the row movers; each channel's sum is the same sequence of
// operations either way).
template <int OP, int V>
__global__ __launch_bounds__(PO_BLOCK) void po_gather_bwd(const float *__restrict__ g, const float *__restrict__ w,
                                                         const int *__restrict__ start, const int *__restrict__ pos,
                                                         float *__restrict__ d_inp, long long elems, int total, int per, int c,
                                                         int w_c) {
    typedef typename Chan<V>::type T;
    const int cv = c / V;
    const T *gv = reinterpret_cast<const T *>(g);
    PO_FOR_ELEMENTS(e, elems) {                    // e counts groups of V channels
        const long long j = e / cv;
        const int ch = (int)(e - j * cv) * V;      // the group's first channel
        const int s = clampi(start[j], 0, total), end = clampi(start[j + 1], s, total);
        T acc = T();
        for (int k = s; k < end; ++k) {            // the list's length
            const int p = pos[k];
            if ((unsigned)p >= (unsigned)total) continue;
            T term;
            if (OP == BWD_GROUPING) {
                term = gv[((size_t)p * c + ch) / V];
            } else if (OP == BWD_SUBTRACTION) {
                term = neg_of(gv[((size_t)p * c + ch) / V]);
            } else if (OP == BWD_INTERPOLATION) {
                const float wp = w[p];
                term = mul_rn(gv[((size_t)(p / per) * c + ch) / V], wp, wp, wp, wp);
            } else {
                const float *wr = w + (size_t)p * w_c;
                term = mul_rn(gv[((size_t)(p / per) * c + ch) / V], wr[ch % w_c], wr[(ch + 1) % w_c], wr[(ch + 2) % w_c],
                              wr[(ch + 3) % w_c]);   // (V == 1 reads the first only)
            }
            acc = add_rn(acc, term);
        }
        reinterpret_cast<T *>(d_inp)[e] = acc;
    }
}

__global__ __launch_bounds__(PO_BLOCK) void po_subtraction_bwd_a(const float *__restrict__ d_out, float *__restrict__ d_a,
                                                                long long elems, int nsample, int c) {
    PO_FOR_ELEMENTS(e, elems) {
        const long long r = e / c;
        const int ch = (int)(e - r * c);
        float acc = 0.f;
        for (int i = 0; i < nsample; ++i) acc = __fadd_rn(acc, d_out[(r * nsample + i) * c + ch]);
        d_a[e] = acc;
    }
}

__global__ __launch_bounds__(PO_BLOCK) void po_aggregation_bwd_pos(const float *__restrict__ w, const float *__restrict__ g,
                                                                  float *__restrict__ d_position, long long elems, int nsample,
                                                                  int c, int w_c) {
    PO_FOR_ELEMENTS(e, elems) {
        const long long p = e / c;
        const int ch = (int)(e - p * c);
        d_position[e] = __fmul_rn(g[(p / nsample) * c + ch], w[p * w_c + ch % w_c]);
    }
}

__global__ __launch_bounds__(PO_BLOCK) void po_aggregation_bwd_w(const float *__restrict__ inp, const float *__restrict__ position,
                                                                const int *__restrict__ idx, const float *__restrict__ g,
                                                                float *__restrict__ d_w, int n, long long elems, int nsample, int c,
                                                                int w_c) {
    PO_FOR_ELEMENTS(e, elems) {
        const long long p = e / w_c;
        const int k = (int)(e - p * w_c);
        const float *row = row_of(inp, idx[p], n, c);
        const float *grow = g + (p / nsample) * c, *prow = position + p * c;
        float acc = 0.f;
        for (int ch = k; ch < c; ch += w_c) acc = __fadd_rn(acc, __fmul_rn(grow[ch], __fadd_rn(row ? row[ch] : 0.f, prow[ch])));
        d_w[e] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// furthest point sampling
// ---------------------------------------------------------------------------------------------
// DPP controls (gfx9): the other lane of a pair, the other pair of a quad, the mirrored lane of a half row and of a row, then the
// last lane of a row to the whole next row and lane 31 to the upper half.
enum { DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140, DPP_BCAST15 = 0x142, DPP_BCAST31 = 0x143 };

// max(v, the key of the lane that CTRL names); a lane without a source, or in a row outside ROW_MASK, keeps v (0 is below every key)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_max(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

// the largest key of the wave, in every lane
__device__ __forceinline__ u64 wave_max_key(u64 v) {
    v = dpp_max<DPP_XOR1, 0xf>(v);
    v = dpp_max<DPP_XOR2, 0xf>(v);
    v = dpp_max<DPP_HALF_MIRROR, 0xf>(v);
    v = dpp_max<DPP_ROW_MIRROR, 0xf>(v);      // every lane: its row's maximum
    v = dpp_max<DPP_BCAST15, 0xa>(v);         // rows 1 and 3: the maximum of rows 0-1 and 2-3
    v = dpp_max<DPP_BCAST31, 0xc>(v);         // row 3: the wave's
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// One workgroup per segment.  DIM: the compile-time dimension (3), or 0 for the route that takes `dim` at run time (its loops are
// unrolled to DODA_PO_FPS_MAX_DIM under `d < dim`, so the coordinate arrays still live in registers).
// Every loop bound and every branch around the barrier depends only on the offsets, which all threads read alike.
template <int DIM>
__global__ __launch_bounds__(DODA_PO_FPS_BLOCK) void po_fps(const float *__restrict__ xyz, const int *__restrict__ offset,
                                                           const int *__restrict__ new_offset, float *__restrict__ ws,
                                                           int *__restrict__ idx, int n, int m, int dim_rt) {
    constexpr int B = DODA_PO_FPS_BLOCK, REG = DODA_PO_FPS_REG, WAVES = B / DODA_WAVE;
    constexpr int D = DIM ? DIM : DODA_PO_FPS_MAX_DIM;
    const int dim = DIM ? DIM : dim_rt;
    __shared__ u64 s_key[2][WAVES];
    __shared__ float s_c[2][WAVES][D];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = clampi(b ? offset[b - 1] : 0, 0, n), len = clampi(offset[b], lo, n) - lo;
    const int olo = clampi(b ? new_offset[b - 1] : 0, 0, m), want = clampi(new_offset[b], olo, m) - olo;
    if (want == 0) return;
    if (len == 0) {
        for (int s = tid; s < want; s += B) idx[olo + s] = -1;
        return;
    }
    const float *seg = xyz + (size_t)lo * dim;
    float *run = ws + lo;

    float px[REG][D], pd[REG];
#pragma unroll
    for (int r = 0; r < REG; ++r) {
        const int i = tid + r * B;
        pd[r] = 1e10f;
#pragma unroll
        for (int d = 0; d < D; ++d) px[r][d] = (i < len && d < dim) ? seg[(size_t)i * dim + d] : 0.f;
    }
    for (int i = REG * B + tid; i < len; i += B) run[i] = 1e10f;   // read back by this thread alone

    float cx[D];
#pragma unroll
    for (int d = 0; d < D; ++d) cx[d] = d < dim ? seg[d] : 0.f;
    if (tid == 0) idx[olo] = lo;

    for (int s = 1; s < want; ++s) {
        u64 best = 0;
#pragma unroll
        for (int r = 0; r < REG; ++r) {
            if (r * B >= len) continue;            // (the same for the whole workgroup: a short segment pays for its own slots only)
            const int i = tid + r * B;
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (d < dim) {
                    const float df = __fsub_rn(px[r][d], cx[d]);
                    acc = __fadd_rn(acc, __fmul_rn(df, df));
                }
            }
            const float t = fminf(pd[r], acc);
            pd[r] = t;
            const u64 key = ((u64)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)i);
            if (i < len && key > best) best = key;
        }
        for (int i = REG * B + tid; i < len; i += B) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (d < dim) {
                    const float df = __fsub_rn(seg[(size_t)i * dim + d], cx[d]);
                    acc = __fadd_rn(acc, __fmul_rn(df, df));
                }
            }
            const float t = fminf(run[i], acc);
            run[i] = t;
            const u64 key = ((u64)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)i);
            if (key > best) best = key;
        }
        const u64 wbest = wave_max_key(best);
        const int par = s & 1, wave = tid >> 6;
        if (best == wbest && best != 0) {          // one lane of the wave: indices are distinct
            const int i = (int)(0xffffffffu - (unsigned)wbest);
            float wx[D];
            if (i < REG * B) {
                const int slot = i / B;
#pragma unroll
                for (int d = 0; d < D; ++d) wx[d] = px[0][d];
#pragma unroll
                for (int r = 1; r < REG; ++r)
#pragma unroll
                    for (int d = 0; d < D; ++d) wx[d] = slot == r ? px[r][d] : wx[d];
            } else {
#pragma unroll
                for (int d = 0; d < D; ++d) wx[d] = d < dim ? seg[(size_t)i * dim + d] : 0.f;
            }
            s_key[par][wave] = wbest;
#pragma unroll
            for (int d = 0; d < D; ++d) s_c[par][wave][d] = wx[d];
        } else if (wbest == 0 && lane_id() == 0) {
            s_key[par][wave] = 0;                  // a wave without points (len < 1024)
        }
        doda_sync();
        // Every row of 16 lanes reads the 16 slots, one per lane, and folds them with four DPP steps; the slot that holds the
        // maximum (keys of different waves differ: their indices do) names the wave whose coordinates are the next centre.
        static_assert(WAVES == 16, "one DPP row per set of slots");
        const u64 slot_key = s_key[par][tid & (WAVES - 1)];
        u64 top = dpp_max<DPP_XOR1, 0xf>(slot_key);
        top = dpp_max<DPP_XOR2, 0xf>(top);
        top = dpp_max<DPP_HALF_MIRROR, 0xf>(top);
        top = dpp_max<DPP_ROW_MIRROR, 0xf>(top);
        const int tw = (__ffsll((long long)__ballot(slot_key == top)) - 1) & (WAVES - 1);
#pragma unroll
        for (int d = 0; d < D; ++d) cx[d] = s_c[par][tw][d];
        if (tid == 0) idx[olo + s] = lo + (int)(0xffffffffu - (unsigned)top);
    }
}

int grid_for(long long elems) {
    const long long blocks = (elems + PO_BLOCK - 1) / PO_BLOCK;
    return (int)(blocks < PO_MAX_GRID ? blocks : PO_MAX_GRID);
}

bool neg(int a, int b = 0, int c = 0, int d = 0, int e = 0) { return a < 0 || b < 0 || c < 0 || d < 0 || e < 0; }

// m * nsample as an int32 count of positions, or -1
long long positions(int m, int nsample) {
    const long long t = (long long)m * nsample;
    return t > INT32_MAX ? -1 : t;
}

template <int OP>
int gather_bwd(const float *g, const float *w, const int32_t *start, const int32_t *pos, float *d_inp, int n, long long total,
               int per, int c, int w_c, doda_stream_t stream) {
    const long long elems = (long long)n * c;
    if (elems == 0) return DODA_OK;
    if (!start || !d_inp || (total > 0 && (!pos || !g || (OP != BWD_GROUPING && OP != BWD_SUBTRACTION && !w)))) return DODA_ERR_INVALID;
    per = per > 0 ? per : 1;
    w_c = w_c > 0 ? w_c : 1;
    if (c % 4 == 0 && al16(g) && al16(d_inp))
        po_gather_bwd<OP, 4><<<grid_for(elems / 4), PO_BLOCK, 0, as_stream(stream)>>>(g, w, start, pos, d_inp, elems / 4, (int)total, per,
                                                                                     c, w_c);
    else
        po_gather_bwd<OP, 1><<<grid_for(elems), PO_BLOCK, 0, as_stream(stream)>>>(g, w, start, pos, d_inp, elems, (int)total, per, c,
                                                                                 w_c);
    return doda_check_launch();
}

}  // namespace

extern "C" {

int32_t doda_pointops_abi_version(void) { return DODA_POINTOPS_ABI_VERSION; }

size_t doda_po_transpose_workspace_bytes(int32_t n) {
    if (n <= 0) return 0;
    return ((size_t)n + scan_ws_ints(n)) * sizeof(int32_t);
}

int doda_po_transpose(const int32_t *idx, int32_t m, int32_t nsample, int32_t n, int32_t *start, int32_t *pos, void *ws,
                      size_t ws_bytes, doda_stream_t stream) {
    if (neg(m, nsample, n)) return DODA_ERR_INVALID;
    const long long total = positions(m, nsample);
    if (total < 0) return DODA_ERR_INVALID;
    if (n == 0) return DODA_OK;
    if (!start || (total > 0 && (!idx || !pos)) || !ws || ((uintptr_t)ws & 3)) return DODA_ERR_INVALID;
    if (ws_bytes < doda_po_transpose_workspace_bytes(n)) return DODA_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    int32_t *count = static_cast<int32_t *>(ws), *scan_ws = count + n;
    if (hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return DODA_ERR_LAUNCH;
    if (total > 0) po_count<<<grid_for(total), PO_BLOCK, 0, s>>>(idx, (int)total, n, count);
    const int st = exclusive_scan_i32(count, start, n, start + n, scan_ws, s);
    if (st != DODA_OK) return st;
    if (total == 0) return doda_check_launch();
    if (hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return DODA_ERR_LAUNCH;
    po_fill<<<grid_for(total), PO_BLOCK, 0, s>>>(idx, (int)total, n, start, count, pos);
    po_sort_lists<<<div_up(n, PO_BLOCK), PO_BLOCK, 0, s>>>(start, n, (int)total, pos);
    return doda_check_launch();
}

int doda_po_grouping_fwd(const float *inp, const int32_t *idx, float *out, int32_t n, int32_t m, int32_t nsample, int32_t c,
                         doda_stream_t stream) {
    if (neg(n, m, nsample, c) || positions(m, nsample) < 0) return DODA_ERR_INVALID;
    const long long elems = positions(m, nsample) * c;
    if (elems == 0) return DODA_OK;
    if (!idx || !out || (n > 0 && !inp)) return DODA_ERR_INVALID;
    if (c % 4 == 0 && al16(inp) && al16(out))
        po_grouping_fwd<4><<<grid_for(elems / 4), PO_BLOCK, 0, as_stream(stream)>>>(inp, idx, out, n, elems / 4, c);
    else
        po_grouping_fwd<1><<<grid_for(elems), PO_BLOCK, 0, as_stream(stream)>>>(inp, idx, out, n, elems, c);
    return doda_check_launch();
}

int doda_po_grouping_bwd(const float *d_out, const int32_t *start, const int32_t *pos, float *d_inp, int32_t n, int32_t total,
                         int32_t c, doda_stream_t stream) {
    if (neg(n, total, c)) return DODA_ERR_INVALID;
    return gather_bwd<BWD_GROUPING>(d_out, nullptr, start, pos, d_inp, n, total, 1, c, 1, stream);
}

int doda_po_interpolation_fwd(const float *inp, const int32_t *idx, const float *w, float *out, int32_t n, int32_t m, int32_t k,
                              int32_t c, doda_stream_t stream) {
    if (neg(n, m, k, c) || positions(m, k) < 0) return DODA_ERR_INVALID;
    const long long elems = (long long)m * c;
    if (elems == 0) return DODA_OK;
    if (!out || (k > 0 && (!idx || !w)) || (n > 0 && k > 0 && !inp)) return DODA_ERR_INVALID;
    po_interpolation_fwd<<<grid_for(elems), PO_BLOCK, 0, as_stream(stream)>>>(inp, idx, w, out, n, elems, k, c);
    return doda_check_launch();
}

int doda_po_interpolation_bwd(const float *d_out, const float *w, const int32_t *start, const int32_t *pos, float *d_inp, int32_t n,
                              int32_t m, int32_t k, int32_t c, doda_stream_t stream) {
    if (neg(n, m, k, c) || positions(m, k) < 0) return DODA_ERR_INVALID;
    return gather_bwd<BWD_INTERPOLATION>(d_out, w, start, pos, d_inp, n, positions(m, k), k, c, 1, stream);
}

int doda_po_subtraction_fwd(const float *a, const float *b, const int32_t *idx, float *out, int32_t n, int32_t m, int32_t nsample,
                            int32_t c, doda_stream_t stream) {
    if (neg(n, m, nsample, c) || positions(m, nsample) < 0) return DODA_ERR_INVALID;
    const long long elems = positions(m, nsample) * c;
    if (elems == 0) return DODA_OK;
    if (!a || !idx || !out || (n > 0 && !b)) return DODA_ERR_INVALID;
    if (c % 4 == 0 && al16(a) && al16(b) && al16(out))
        po_subtraction_fwd<4><<<grid_for(elems / 4), PO_BLOCK, 0, as_stream(stream)>>>(a, b, idx, out, n, elems / 4, nsample, c);
    else
        po_subtraction_fwd<1><<<grid_for(elems), PO_BLOCK, 0, as_stream(stream)>>>(a, b, idx, out, n, elems, nsample, c);
    return doda_check_launch();
}

int doda_po_subtraction_bwd(const float *d_out, const int32_t *start, const int32_t *pos, float *d_a, float *d_b, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, doda_stream_t stream) {
    if (neg(n, m, nsample, c) || positions(m, nsample) < 0) return DODA_ERR_INVALID;
    const long long total = positions(m, nsample), elems_a = (long long)m * c;
    if (elems_a > 0) {
        if (!d_a || (nsample > 0 && !d_out)) return DODA_ERR_INVALID;
        if ((long long)n * c > 0 && (!start || !d_b || (total > 0 && !pos))) return DODA_ERR_INVALID;   // before the first launch
        po_subtraction_bwd_a<<<grid_for(elems_a), PO_BLOCK, 0, as_stream(stream)>>>(d_out, d_a, elems_a, nsample, c);
    }
    return gather_bwd<BWD_SUBTRACTION>(d_out, nullptr, start, pos, d_b, n, total, 1, c, 1, stream);
}

int doda_po_aggregation_fwd(const float *inp, const float *position, const float *w, const int32_t *idx, float *out, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, int32_t w_c, doda_stream_t stream) {
    if (neg(n, m, nsample, c, w_c) || positions(m, nsample) < 0) return DODA_ERR_INVALID;
    const long long elems = (long long)m * c;
    if (elems == 0) return DODA_OK;
    if (nsample > 0 && w_c < 1) return DODA_ERR_INVALID;
    if (!out || (nsample > 0 && (!position || !w || !idx)) || (n > 0 && nsample > 0 && !inp)) return DODA_ERR_INVALID;
    po_aggregation_fwd<<<grid_for(elems), PO_BLOCK, 0, as_stream(stream)>>>(inp, position, w, idx, out, n, elems, nsample, c,
                                                                           w_c > 0 ? w_c : 1);
    return doda_check_launch();
}

int doda_po_aggregation_bwd(const float *inp, const float *position, const float *w, const int32_t *idx, const int32_t *start,
                            const int32_t *pos, const float *d_out, float *d_inp, float *d_position, float *d_w, int32_t n,
                            int32_t m, int32_t nsample, int32_t c, int32_t w_c, doda_stream_t stream) {
    if (neg(n, m, nsample, c, w_c) || positions(m, nsample) < 0) return DODA_ERR_INVALID;
    const long long total = positions(m, nsample), elems_p = total * c, elems_w = total * w_c;
    if (elems_p > 0) {
        if (w_c < 1 || !position || !w || !idx || !d_out || !d_position || !d_w || (n > 0 && !inp)) return DODA_ERR_INVALID;
        if (n > 0 && (!start || !pos || !d_inp)) return DODA_ERR_INVALID;   // before the first launch
        hipStream_t s = as_stream(stream);
        po_aggregation_bwd_pos<<<grid_for(elems_p), PO_BLOCK, 0, s>>>(w, d_out, d_position, elems_p, nsample, c, w_c);
        po_aggregation_bwd_w<<<grid_for(elems_w), PO_BLOCK, 0, s>>>(inp, position, idx, d_out, d_w, n, elems_w, nsample, c, w_c);
    }
    return gather_bwd<BWD_AGGREGATION>(d_out, w, start, pos, d_inp, n, total, nsample, c, w_c, stream);
}

int doda_po_furthestsampling(const float *xyz, const int32_t *offset, const int32_t *new_offset, float *ws, int32_t *idx, int32_t n,
                             int32_t m, int32_t nbatch, int32_t dim, doda_stream_t stream) {
    if (neg(n, m, nbatch) || dim < 1 || dim > DODA_PO_FPS_MAX_DIM) return DODA_ERR_INVALID;
    if (nbatch == 0 || m == 0) return DODA_OK;
    if (!offset || !new_offset || !idx || (n > 0 && (!xyz || !ws))) return DODA_ERR_INVALID;
    if (dim == 3)
        po_fps<3><<<nbatch, DODA_PO_FPS_BLOCK, 0, as_stream(stream)>>>(xyz, offset, new_offset, ws, idx, n, m, dim);
    else
        po_fps<0><<<nbatch, DODA_PO_FPS_BLOCK, 0, as_stream(stream)>>>(xyz, offset, new_offset, ws, idx, n, m, dim);
    return doda_check_launch();
}

}  // extern "C"

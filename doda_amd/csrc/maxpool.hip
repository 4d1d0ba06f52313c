// Indice-pair max pooling on the gather table (spconv v1.2 indice_maxpool /
// indice_maxpool_backward; not called by DODA, named by north_star).  Output-stationary like
// the convolutions: one lane per (output row, channel), each output written once.
// Upstream semantics: out starts at 0 and is max-ed with every paired input
// (out = max(out, in)), so an output with pairs never drops below 0; backward routes dy to
// every paired input whose value equals the pooled output.
//
// doda_maxpool_fwd / doda_maxpool_bwd (include/doda_spconv.h) take the element size: fp32 or bf16 rows, moved as 16-byte pieces
// where a row is a whole number of them.  Their backward is INPUT-stationary over the reverse table: one lane per (input row,
// piece) sums dy over the outputs that row feeds in ascending offset, in fp32, rounds once and writes dx once — no atomic, no
// zero fill, the same bits on every run.  The fp32 module path keeps the two _f32 entry points below as they were.
#include "common.hpp"
#include "../../include/doda_spconv.h"

namespace {
__global__ __launch_bounds__(256) void maxpool_fwd(const float *__restrict__ x, int c,
                                                   const int32_t *__restrict__ tbl, int ld, int K,
                                                   int n_out, float *__restrict__ y) {
    const long long total = (long long)n_out * c;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(e / c), ch = (int)(e - (long long)t * c);
        float m = 0.f;
        for (int o = 0; o < K; ++o) {
            const int j = tbl[(long long)o * ld + t];
            if (j >= 0) {
                const float v = x[(long long)j * c + ch];
                m = v > m ? v : m;
            }
        }
        y[e] = m;
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd(const float *__restrict__ x,
                                                   const float *__restrict__ y,
                                                   const float *__restrict__ dy, int c,
                                                   const int32_t *__restrict__ tbl, int ld, int K,
                                                   int n_out, float *__restrict__ dx) {
    const long long total = (long long)n_out * c;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(e / c), ch = (int)(e - (long long)t * c);
        const float m = y[e], g = dy[e];
        for (int o = 0; o < K; ++o) {
            const int j = tbl[(long long)o * ld + t];
            if (j >= 0 && x[(long long)j * c + ch] == m) atomicAdd(&dx[(long long)j * c + ch], g);
        }
    }
}

// ---- any element size (include/doda_spconv.h) ---------------------------------------------------------------------------------
// E: the element as stored (float, or uint16_t holding a bf16); V elements per lane: one 16-byte piece, or 1 (scalar tail path)
__device__ __forceinline__ float pool_val(float v) { return v; }
__device__ __forceinline__ float pool_val(uint16_t v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ void pool_round(float v, float *out) { *out = v; }
__device__ __forceinline__ void pool_round(float v, uint16_t *out) { *out = __builtin_bit_cast(unsigned short, (__bf16)v); }

template <typename E, int V>
struct alignas(sizeof(E) * V) PoolPiece { E e[V]; };

template <typename E, int V>
__global__ __launch_bounds__(256) void maxpool_fwd_any(const E *__restrict__ x, int c, const int32_t *__restrict__ tbl, int ld, int K,
                                                       int n_in, int n_out, E *__restrict__ y) {
    typedef PoolPiece<E, V> P;
    const int units = c / V;
    const long long total = (long long)n_out * units;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(e / units), u = (int)(e - (long long)t * units);
        P best;
        float m[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { best.e[k] = (E)0; m[k] = 0.f; }
        for (int o = 0; o < K; ++o) {
            const int j = tbl[(long long)o * ld + t];
            if ((unsigned)j >= (unsigned)n_in) continue;
            const P in = *reinterpret_cast<const P *>(x + (long long)j * c + (long long)u * V);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float v = pool_val(in.e[k]);
                if (v > m[k]) { m[k] = v; best.e[k] = in.e[k]; }
            }
        }
        *reinterpret_cast<P *>(y + (long long)t * c + (long long)u * V) = best;
    }
}

template <typename E, int V>
__global__ __launch_bounds__(256) void maxpool_bwd_any(const E *__restrict__ x, const E *__restrict__ y, const E *__restrict__ dy,
                                                       int c, const int32_t *__restrict__ tbl_rev, int ld, int K, int n_in,
                                                       int n_out, E *__restrict__ dx) {
    typedef PoolPiece<E, V> P;
    const int units = c / V;
    const long long total = (long long)n_in * units;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e / units), u = (int)(e - (long long)j * units);
        const long long at = (long long)u * V;
        const P in = *reinterpret_cast<const P *>(x + (long long)j * c + at);
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;
        for (int o = 0; o < K; ++o) {                                     // ascending offsets: one fixed order of the fp32 adds
            const int t = tbl_rev[(long long)o * ld + j];
            if ((unsigned)t >= (unsigned)n_out) continue;
            const P out = *reinterpret_cast<const P *>(y + (long long)t * c + at);
            const P g = *reinterpret_cast<const P *>(dy + (long long)t * c + at);
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (pool_val(in.e[k]) == pool_val(out.e[k])) acc[k] += pool_val(g.e[k]);
        }
        P res;
#pragma unroll
        for (int k = 0; k < V; ++k) pool_round(acc[k], &res.e[k]);
        *reinterpret_cast<P *>(dx + (long long)j * c + at) = res;
    }
}

int pool_grid(long long total) { return (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192); }

// f(element tag, Int<V>): 16-byte pieces where the rows are whole pieces and every base is 16-byte aligned, else one element
template <class F>
void pool_dispatch(int elem_bytes, int c, bool aligned, F f) {
    const bool vec = aligned && ((long long)c * elem_bytes) % 16 == 0;
    if (elem_bytes == 4) { if (vec) f(float(), Int<4>()); else f(float(), Int<1>()); }
    else { if (vec) f(uint16_t(), Int<8>()); else f(uint16_t(), Int<1>()); }
}
}  // namespace

extern "C" int doda_maxpool_fwd_f32(const float *x, int32_t c, const int32_t *tbl, int32_t ld,
                                    int32_t K, int32_t n_out, float *y, doda_stream_t stream) {
    if (c <= 0 || K <= 0 || n_out < 0 || ld < n_out) return DODA_ERR_INVALID;
    if (n_out == 0) return DODA_OK;
    if (!x || !tbl || !y) return DODA_ERR_INVALID;
    const long long total = (long long)n_out * c;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(maxpool_fwd, dim3(grid), dim3(256), 0, as_stream(stream), x, c, tbl, ld, K,
                       n_out, y);
    return doda_check_launch();
}

extern "C" int doda_maxpool_bwd_f32(const float *x, const float *y, const float *dy, int32_t c,
                                    const int32_t *tbl, int32_t ld, int32_t K, int32_t n_out,
                                    float *dx, doda_stream_t stream) {
    if (c <= 0 || K <= 0 || n_out < 0 || ld < n_out) return DODA_ERR_INVALID;
    if (n_out == 0) return DODA_OK;
    if (!x || !y || !dy || !tbl || !dx) return DODA_ERR_INVALID;
    const long long total = (long long)n_out * c;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(maxpool_bwd, dim3(grid), dim3(256), 0, as_stream(stream), x, y, dy, c, tbl,
                       ld, K, n_out, dx);
    return doda_check_launch();
}

extern "C" int doda_maxpool_fwd(const void *x, int32_t c, int32_t elem_bytes, const int32_t *tbl, int32_t ld, int32_t K,
                                int32_t n_in, int32_t n_out, void *y, doda_stream_t stream) {
    if (c <= 0 || K <= 0 || n_in < 0 || n_out < 0 || ld < n_out) return DODA_ERR_INVALID;
    if (elem_bytes != 2 && elem_bytes != 4) return DODA_ERR_UNSUPPORTED;
    if (n_out == 0) return DODA_OK;
    if (!tbl || !y || (!x && n_in > 0)) return DODA_ERR_INVALID;
    pool_dispatch(elem_bytes, c, al16(x) && al16(y), [&](auto tag, auto v) {
        typedef decltype(tag) E;
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((maxpool_fwd_any<E, V>), dim3(pool_grid((long long)n_out * (c / V))), dim3(256), 0, as_stream(stream),
                           (const E *)x, c, tbl, ld, K, n_in, n_out, (E *)y);
    });
    return doda_check_launch();
}

extern "C" int doda_maxpool_bwd(const void *x, const void *y, const void *dy, int32_t c, int32_t elem_bytes, const int32_t *tbl_rev,
                                int32_t ld, int32_t K, int32_t n_in, int32_t n_out, void *dx, doda_stream_t stream) {
    if (c <= 0 || K <= 0 || n_in < 0 || n_out < 0 || ld < n_in) return DODA_ERR_INVALID;
    if (elem_bytes != 2 && elem_bytes != 4) return DODA_ERR_UNSUPPORTED;
    if (n_in == 0) return DODA_OK;
    if (!x || !tbl_rev || !dx || ((!y || !dy) && n_out > 0)) return DODA_ERR_INVALID;
    pool_dispatch(elem_bytes, c, al16(x) && al16(y) && al16(dy) && al16(dx), [&](auto tag, auto v) {
        typedef decltype(tag) E;
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((maxpool_bwd_any<E, V>), dim3(pool_grid((long long)n_in * (c / V))), dim3(256), 0, as_stream(stream),
                           (const E *)x, (const E *)y, (const E *)dy, c, tbl_rev, ld, K, n_in, n_out, (E *)dx);
    });
    return doda_check_launch();
}

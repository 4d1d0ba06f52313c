// The Linear head on a voxel row, shared by the kernels that must agree on its bits: head_ce_fwd / _bwd and the self-training
// confidence (head.hip), the Lovasz-softmax items and backward sweeps (lovasz.hip).  Row loads for bf16 / fp32 features, the
// weights staged in LDS (rounded to bf16 for bf16 features), the logits of one voxel in registers with their argmax; what the two
// backward sweeps have in common (the LDS columns, the d_feats row store, the column sums for db); and the host side of every
// entry point: block count, argument check, the dispatch over element size and class-count bucket.
#pragma once
#include <initializer_list>
#include "common.hpp"
#include "spconv_common.hpp"

namespace {
constexpr int HD_BLOCK = 256;
constexpr int HD_MAX_C = 32;      // feature channels (DODA: 16)
constexpr int HD_MAX_K = 32;      // classes

template <int ESZ> struct HdRow;
template <> struct HdRow<2> {
    static __device__ __forceinline__ void load4(const void *p, float (&v)[4]) {
        const u32x2 r = *reinterpret_cast<const u32x2 *>(p);
        v[0] = __uint_as_float(r[0] << 16); v[1] = __uint_as_float(r[0] & 0xffff0000u);
        v[2] = __uint_as_float(r[1] << 16); v[3] = __uint_as_float(r[1] & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(void *p, float v) { *reinterpret_cast<unsigned short *>(p) = f2bf(v); }
    static __device__ __forceinline__ float load(const void *p) { return __uint_as_float((unsigned)*reinterpret_cast<const unsigned short *>(p) << 16); }
    static __device__ __forceinline__ float wround(float w) { return __uint_as_float((unsigned)f2bf(w) << 16); }
};
template <> struct HdRow<4> {
    static __device__ __forceinline__ void load4(const void *p, float (&v)[4]) {
        const f32x4 r = *reinterpret_cast<const f32x4 *>(p);
        v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
    }
    static __device__ __forceinline__ void store(void *p, float v) { *reinterpret_cast<float *>(p) = v; }
    static __device__ __forceinline__ float load(const void *p) { return *reinterpret_cast<const float *>(p); }
    static __device__ __forceinline__ float wround(float w) { return w; }
};

template <int ESZ, int C>
__device__ __forceinline__ void hd_load_row(const void *feats, long long v, float (&f)[C]) {
#pragma unroll
    for (int q = 0; q < C; q += 4) {
        float t[4];
        HdRow<ESZ>::load4((const char *)feats + ((size_t)v * C + q) * ESZ, t);
        f[q] = t[0]; f[q + 1] = t[1]; f[q + 2] = t[2]; f[q + 3] = t[3];
    }
}
template <int C>
__device__ __forceinline__ float hd_logit(const float (*w)[HD_MAX_C], const float *b, int k, const float (&f)[C]) {
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) z = __builtin_fmaf(w[k][c], f[c], z);
    return z + b[k];
}
template <int ESZ>
__device__ __forceinline__ void hd_stage_weights(const float *__restrict__ weight, const float *__restrict__ bias, int n_cls, int c,
                                                 float (*w)[HD_MAX_C], float *b) {
    for (int e = threadIdx.x; e < n_cls * c; e += HD_BLOCK) w[e / c][e % c] = HdRow<ESZ>::wround(weight[e]);
    for (int k = threadIdx.x; k < n_cls; k += HD_BLOCK) b[k] = bias ? bias[k] : 0.f;
    doda_sync();
}

// NK: the class count rounded up to a multiple of four (compile time): the voxel's logits live in registers — computed once per
// sweep (three recomputations per class, with the class count a run-time bound, took 31 us forward / 121 us backward at 601 k
// voxels) — with the padding classes at -inf.
template <int C, int NK>
__device__ __forceinline__ void hd_logits(const float (*w)[HD_MAX_C], const float *b, int n_cls, const float (&f)[C], float (&z)[NK], float &mx, int &arg) {
    mx = -INFINITY;
    arg = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) t = __builtin_fmaf(w[k][c], f[c], t);     // (fused: the build's -ffp-contract=off would make it two instructions)
        t = k < n_cls ? t + b[k] : -INFINITY;
        z[k] = t;
        if (t > mx) { mx = t; arg = k; }
        if ((k & 3) == 3) asm volatile("" ::: "memory");
    }
}

// ---- the backward sweeps (head_ce_bwd, lovasz_bwd): one voxel per thread, a workgroup's 256 voxels -----------------------------
// The per-class values of a thread's voxel live in LDS COLUMNS (sz[k][thread]: conflict-free) instead of register arrays: the class
// loops stay rolled and the kernels need ~50-60 VGPRs — the register form (three 20-element arrays per thread, loops fully unrolled)
// compiled to 256 VGPRs + spills and ran at 120 us.
// the voxel's logits into its column, -> their max: the same chain of fused multiply-adds as hd_logits (the forward's bits)
template <int C>
__device__ __forceinline__ float hd_logits_lds(const float (*w)[HD_MAX_C], const float *b, int n_cls, const float (&f)[C],
                                               float (*sz)[HD_BLOCK], int tid) {
    float mx = -INFINITY;
#pragma unroll 2
    for (int k = 0; k < n_cls; ++k) {
        const float z = hd_logit<C>(w, b, k, f);
        sz[k][tid] = z;
        mx = fmaxf(mx, z);
    }
    return mx;
}
template <int ESZ, int C>
__device__ __forceinline__ void hd_store_dfeats(void *d_feats, long long v, const float (&df)[C]) {
    char *dfr = (char *)d_feats + (size_t)v * C * ESZ;
    if constexpr (ESZ == 2) {
#pragma unroll
        for (int q = 0; q < C; q += 8) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (unsigned)f2bf(df[q + 2 * j]) | ((unsigned)f2bf(df[q + 2 * j + 1]) << 16);
            *reinterpret_cast<u32x4 *>(dfr + (size_t)q * 2) = o;
        }
    } else {
#pragma unroll
        for (int q = 0; q < C; q += 4) *reinterpret_cast<f32x4 *>(dfr + (size_t)q * 4) = (f32x4){df[q], df[q + 1], df[q + 2], df[q + 3]};
    }
}
// db_partial[workgroup][k] = the column sums of the workgroup's 256 voxels: 8 threads per class over 32 columns each, then the eight
// in order (fixed order)
__device__ __forceinline__ void hd_db_colsums(const float (*sz)[HD_BLOCK], int n_cls, float *__restrict__ db_partial) {
    doda_sync();
    const int k = threadIdx.x >> 3, part = threadIdx.x & 7;
    float t = 0.f;
    if (k < n_cls) {
        for (int q = 0; q < 32; ++q) t += sz[k][part * 32 + q];
    }
    t += __shfl_xor(t, 1, 64);
    t += __shfl_xor(t, 2, 64);
    t += __shfl_xor(t, 4, 64);
    if (k < n_cls && part == 0) db_partial[(size_t)blockIdx.x * n_cls + k] = t;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int hd_blocks(int m) {
    const int nb = div_up(m, HD_BLOCK);    // one voxel per thread: three dependent global reads per voxel (point list -> point ids ->
    return nb < 1 ? 1 : nb;                // labels) want every wave slot of the chip filled (1024 fatter workgroups: 24 / 53 us)
}
// what every entry point of the head rejects as DODA_ERR_INVALID: the voxel count, the element size, the row stride of the point lists
// (1 where the entry point takes none) and its required pointers
inline bool hd_args_bad(int m, int esz, int v2p_ld, std::initializer_list<const void *> required) {
    bool bad = m < 0 || (esz != 2 && esz != 4) || v2p_ld < 1;
    for (const void *p : required) bad = bad || !p;
    return bad;
}
// KERNEL<element bytes, C channels, classes> on GRID workgroups of HD_BLOCK threads (uses the caller's elem_bytes, n_cls and stream
// s): class counts as compile-time multiples of four (DODA: 20 ScanNet / 13 S3DIS / 11 common classes)
#define HD_DISPATCH_ESZ(KERNEL, ESZ, C, GRID, ...)                                                                      \
    do {                                                                                                                \
        const int nk = (n_cls + 3) / 4 * 4;                                                                             \
        if (nk <= 12) hipLaunchKernelGGL((KERNEL<ESZ, C, 12>), dim3(GRID), dim3(HD_BLOCK), 0, s, __VA_ARGS__);          \
        else if (nk <= 16) hipLaunchKernelGGL((KERNEL<ESZ, C, 16>), dim3(GRID), dim3(HD_BLOCK), 0, s, __VA_ARGS__);     \
        else if (nk <= 20) hipLaunchKernelGGL((KERNEL<ESZ, C, 20>), dim3(GRID), dim3(HD_BLOCK), 0, s, __VA_ARGS__);     \
        else hipLaunchKernelGGL((KERNEL<ESZ, C, 32>), dim3(GRID), dim3(HD_BLOCK), 0, s, __VA_ARGS__);                   \
    } while (0)
#define HD_DISPATCH(KERNEL, C, GRID, ...)                                                                               \
    do {                                                                                                                \
        if (elem_bytes == 2) HD_DISPATCH_ESZ(KERNEL, 2, C, GRID, __VA_ARGS__);                                          \
        else HD_DISPATCH_ESZ(KERNEL, 4, C, GRID, __VA_ARGS__);                                                          \
    } while (0)
}  // namespace

// The Linear head on a voxel row, shared by the kernels that must agree on its bits: head_ce_fwd / _bwd and the self-training
// confidence (head.hip), the Lovasz-softmax items and backward sweeps (lovasz.hip).  Row loads for bf16 / fp32 features, the
// weights staged in LDS (rounded to bf16 for bf16 features), the logits of one voxel in registers with their argmax.
#pragma once
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
}  // namespace

// Device helpers shared by the weight-gradient translation units (spconv_wgrad.hip, spconv_wgrad_pairs.hip,
// spconv_wdma.hip, spconv_wwide.hip): the vector types, the block -> job search, the bf16 repack and the one fixed-order
// reduction of chunk partials.  gfx950 only.
// Not shared on purpose: the three transposing LDS reads (BF16::frags' four-in-one asm, wd_tr_b64's tagged asm, ww_tr's
// builtin: see the comments beside each) and wgrad_dma_reduce's summation (eight loads in flight, a fixed tree).
#pragma once
#include "wgrad_backends.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

// block -> job of a many-job launch: binary search over the jobs' INCLUSIVE block prefix, the field END
template <class J, int J::*END>
__device__ __forceinline__ int find_job(const J *jobs, int n_jobs, int blk) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (blk < jobs[mid].*END) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// two fp32 D fragments whose values are bf16-exact -> one bf16 operand: keep the upper halves.  k-slot q of the lane:
// q < 4 -> d0[q], else d1[q-4]
__device__ __forceinline__ bf16x8 pack_hi16(const f32x4 &d0, const f32x4 &d1) {
    u32x4 r;
    r[0] = __builtin_amdgcn_perm(__float_as_uint(d0[1]), __float_as_uint(d0[0]), 0x07060302u);
    r[1] = __builtin_amdgcn_perm(__float_as_uint(d0[3]), __float_as_uint(d0[2]), 0x07060302u);
    r[2] = __builtin_amdgcn_perm(__float_as_uint(d1[1]), __float_as_uint(d1[0]), 0x07060302u);
    r[3] = __builtin_amdgcn_perm(__float_as_uint(d1[3]), __float_as_uint(d1[2]), 0x07060302u);
    return __builtin_bit_cast(bf16x8, r);
}

// The fixed-order fold  dw[q] (+)= sum_{r < R} src(q)[r * stride]  of block `blk` of a reduction over n_quad float quads
// (256 threads).  A block holds EL = 256 / RL quads x RL chunk lanes, RL = reduce_lanes(R): lane l sums chunks l, l + RL,
// ... starting from +0, the lane sums are added through LDS in ascending l, then the old dw when accumulating: deterministic,
// no float atomics.  The sums do not depend on RL's choice: for R <= 16 a lane holds at most one chunk whatever RL is, and
// partials are MFMA sums that started at +0, so a lane without a chunk adds a +0 that changes no bit (RL was 16 for every
// job once: the coarse levels' jobs have 1 .. 4 chunks, so 3/4 .. 15/16 of a block's threads had nothing to read and a
// 7.5 M-parameter network took 117 k blocks of 256 bytes each).
// src(q): chunk 0's quad q; stride: quads between a quad's consecutive chunks.
template <class Src>
__device__ __forceinline__ void wgrad_fold(int blk, int R, long long n_quad, long long stride, float4 *dw, int accumulate,
                                           Src src) {
    __shared__ float4 part[256];
    const int RL = doda_wgrad::reduce_lanes(R), EL = 256 / RL;                 // RL in {1, 2, 4, 8, 16}
    const int el = (int)threadIdx.x % EL, rl = (int)threadIdx.x / EL;
    const long long q = (long long)blk * EL + el;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < n_quad) {
        const float4 *p = src(q);
        for (int r = rl; r < R; r += RL) {
            const float4 v = p[(long long)r * stride];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    part[rl * EL + el] = s;
    doda_sync();
    if (rl == 0 && q < n_quad) {
        float4 t = part[el];
        for (int r = 1; r < RL; ++r) {
            const float4 v = part[r * EL + el];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        if (accumulate) {
            const float4 old = dw[q];
            t.x += old.x; t.y += old.y; t.z += old.z; t.w += old.w;
        }
        dw[q] = t;
    }
}

}  // namespace

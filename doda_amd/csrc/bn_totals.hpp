// BatchNorm over fp64 TOTALS (ABI 9), shared by the BatchNorm sweeps (bn.hip) and by the convolution kernels that fold a
// BatchNorm into their gather (ABI 11, spconv_gather.hip conv_fast<..., PRE>: reference model/unet_block.py:23-30,46-49,67-79 —
// every conv sits behind BatchNorm1d -> ReLU).  One place for the arithmetic, so a BatchNorm applied by its own sweep and the
// same BatchNorm applied inside the consuming conv's gather give the same bits.  gfx950 only.
#pragma once
// (the part above the kernels' arithmetic is plain C++ — constants, TotArgs, the trace line and the entry points' argument checks —
// and is read by the host plan of the op list as well: layers_plan.hpp, built with g++)
#if defined(__HIPCC__)
#include "common.hpp"
typedef float f32x4 __attribute__((ext_vector_type(4)));
#else
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/doda_hip.h"
#endif
#include <stdarg.h>
#include <stdio.h>

constexpr int BN_TOT_MAX_C = 256;
constexpr int BN_TOT_SLOTS = 8;      // = DODA_STATS_SLOTS (spconv_common.hpp)

// ta / tb: the totals of the producers of the columns [0, ca) and [ca, c) (tb null: one producer) — a channel concatenation.
struct TotArgs {
    const double *ta = nullptr, *tb = nullptr;
    int ca = 0, m = 0;
    float eps = 0.f, momentum = 0.f;
    float *rm = nullptr, *rv = nullptr;           // forward: running statistics or null
    long long *nbt = nullptr;
    float *out_a = nullptr, *out_b = nullptr;     // forward: save_mean, save_invstd; backward: dgamma, dbeta
    int accum = 0;                                // backward: dgamma / dbeta are ADDED to (a second backward pass of one optimizer step)
};

// DODA_TRACE_BN=1 (read once): one stderr line per kernel launch of bn.hip and of the BatchNorm / statistics ops of layers.hip —
// `bn route=<kernel> grid= block=`, the kernel's name as a kernel trace shows it, namespaces stripped (tools/bnnumerics.py)
static inline void bn_trace(unsigned grid, unsigned block, const char *fmt, ...) {
    static const bool on = getenv("DODA_TRACE_BN") && getenv("DODA_TRACE_BN")[0] == '1';
    if (!on) return;
    char name[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    fprintf(stderr, "bn route=%s grid=%u block=%u\n", name, grid, block);
}

// ---- argument checks of the entry points (bn.hip), pure: plan_layers (layers_plan.hpp) asks them before anything is launched ----
inline bool bn_args_bad(int m, int c, int elem_bytes) {
    return m <= 0 || c <= 0 || (c % 4) != 0 || c > 1024 || (elem_bytes != 2 && elem_bytes != 4);
}
template <class... P>
inline bool any_null(const P *...p) { return (... || !p); }
// the second-gradient operand: rows at least c elements apart, a multiple of one fragment, fragment-aligned
inline bool add_bad(const void *add, int add_ld, int c, int elem_bytes) {
    return add_ld < c || add_ld % 4 || ((uintptr_t)add % (4 * (size_t)elem_bytes));
}
// the status doda_bn_relu_fwd_totals / doda_bn_relu_bwd_totals return without a launch (DODA_OK: m == 0, or the sweep is launched)
inline int bn_fwd_totals_status(const void *x, int m, int c, int elem_bytes, const double *totals, const double *totals_b, int c_a,
                                const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                                const void *y, const float *save_mean, const float *save_invstd) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes) || c > BN_TOT_MAX_C) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, y, totals, gamma, beta, save_mean, save_invstd) || (!running_mean != !running_var)) return DODA_ERR_INVALID;
    if (totals_b && (c_a <= 0 || c_a >= c || c_a % 4)) return DODA_ERR_INVALID;   // (tot_sums indexes each producer's totals in groups of four channels)
    return DODA_OK;
}
// (the two entry points over a data-grad epilogue's statistics test `add` before m == 0)
inline int bn_bwd_totals_status(const void *x, const void *dy, int m, int c, int elem_bytes, const double *totals,
                                const float *save_mean, const float *save_invstd, const float *gamma, const float *beta,
                                const void *add, int add_ld, const void *dx, const float *dgamma, const float *dbeta) {
    if (add && add_bad(add, add_ld, c, elem_bytes)) return DODA_ERR_INVALID;
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes) || c > BN_TOT_MAX_C) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, dy, dx, totals, gamma, beta, save_mean, save_invstd, dgamma, dbeta)) return DODA_ERR_INVALID;
    return DODA_OK;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void tot_sums(const TotArgs &t, int c, int ch, double &s1, double &s2) {
    const bool first = ch < t.ca;
    const double *src = first ? t.ta : t.tb;
    const int cw = first ? t.ca : c - t.ca, cc = first ? ch : ch - t.ca;
    s1 = 0.0; s2 = 0.0;
#pragma unroll
    for (int k = 0; k < BN_TOT_SLOTS; ++k) {      // (layout: spconv_common.hpp stats_emit — a 128-byte line per four channels)
        s1 += src[((size_t)(k * 2 + 0) * (cw / 4) + cc / 4) * 16 + (cc & 3)];
        s2 += src[((size_t)(k * 2 + 1) * (cw / 4) + cc / 4) * 16 + (cc & 3)];
    }
}

// ---- the per-channel arithmetic: ONE copy for every form of the statistics (standalone partials, statistics rows, fused, totals) ----
// Forward finish: batch mean, biased variance (clamped at 0) and 1 / sqrt(variance + eps) from (sum, sum of squares) over m rows.
// `mean` is the mean of what was summed: the standalone kernels sum x - k (k = the first row) and add k themselves.
struct BnMoments { double mean, var; float invstd; };
__device__ __forceinline__ BnMoments bn_fwd_finish(double s1, double s2, int m, float eps) {
    BnMoments r;
    r.mean = s1 / m;
    r.var = s2 / m - r.mean * r.mean;
    if (r.var < 0.0) r.var = 0.0;
    r.invstd = (float)(1.0 / sqrt(r.var + (double)eps));
    return r;
}
// Running statistics: running_mean takes the batch mean (shift included), running_var the UNBIASED variance.
__device__ __forceinline__ double bn_unbiased(double var, int m) { return m > 1 ? var * (double)m / (double)(m - 1) : var; }
__device__ __forceinline__ float bn_running(float old, float momentum, double v) {
    return (float)((1.0 - momentum) * (double)old + momentum * v);
}
// Backward coefficients, dx = a * (dz - b - xhat * d), and the parameter gradients, from s1 = sum dz, s2 = sum dz * xhat.
struct BnBwdCoef { float a, b, d, dgamma, dbeta; };
__device__ __forceinline__ BnBwdCoef bn_bwd_coef(double s1, double s2, int m, float gamma, float invstd) {
    BnBwdCoef r;
    r.dbeta = (float)s1;
    r.dgamma = (float)s2;
    r.a = gamma * invstd;
    r.b = (float)(s1 / m);
    r.d = (float)(s2 / m);
    return r;
}

// Forward, channel `ch`: batch mean / 1 / sqrt(biased variance + eps) from the totals; `publish` (one workgroup of the launch):
// save_mean / save_invstd, the running statistics (momentum, unbiased variance) and num_batches_tracked.
__device__ __forceinline__ void tot_fwd_channel(const TotArgs &t, int c, int ch, bool publish, float &mu, float &is) {
    double s1, s2;
    tot_sums(t, c, ch, s1, s2);
    const BnMoments mo = bn_fwd_finish(s1, s2, t.m, t.eps);
    mu = (float)mo.mean;
    is = mo.invstd;
    if (publish) {
        t.out_a[ch] = mu;
        t.out_b[ch] = is;
        if (t.rm) {
            t.rm[ch] = bn_running(t.rm[ch], t.momentum, mo.mean);
            t.rv[ch] = bn_running(t.rv[ch], t.momentum, bn_unbiased(mo.var, t.m));
        }
        if (ch == 0 && t.nbt) *t.nbt = *t.nbt + 1;
    }
}

// Backward, channel `ch`: dx = ca * (dz - cb - xhat * cd); `publish`: dbeta = sum dz, dgamma = sum dz * xhat.
__device__ __forceinline__ void tot_bwd_channel(const TotArgs &t, int c, int ch, bool publish, float invstd, float gamma,
                                                float &ca, float &cb, float &cd) {
    double s1, s2;
    tot_sums(t, c, ch, s1, s2);
    const BnBwdCoef k = bn_bwd_coef(s1, s2, t.m, gamma, invstd);
    ca = k.a;
    cb = k.b;
    cd = k.d;
    if (publish) {
        if (t.accum) {
            t.out_b[ch] += k.dbeta;
            t.out_a[ch] += k.dgamma;
        } else {
            t.out_b[ch] = k.dbeta;
            t.out_a[ch] = k.dgamma;
        }
    }
}

// One element of the sweeps, in the order the standalone kernels always used (-ffp-contract=off: every operation rounds):
//   forward  y  = [relu]((x - mu) * is * ga + be)
//   backward dx = ca * ([yv > 0] dz - cb - xh * cd),  xh = (x - mu) * is, yv = xh * ga + be
// The scalar pair serves the conv prologue (spconv_common.hpp pre_piece, which clamps y itself), the 4-channel forms below every
// sweep of bn.hip: the same formulas, operation for operation.
__device__ __forceinline__ float bn_fwd_elem(float x, float mu, float is, float ga, float be) { return (x - mu) * is * ga + be; }
__device__ __forceinline__ float bn_bwd_elem(float x, float dz, float mu, float is, float ga, float be, float ca, float cb, float cd,
                                             int relu) {
    const float xh = (x - mu) * is;
    if (relu) {
        const float yv = xh * ga + be;
        dz = yv > 0.f ? dz : 0.f;
    }
    return ca * (dz - cb - xh * cd);
}
__device__ __forceinline__ f32x4 bn_fwd_elem4(const f32x4 &x, const f32x4 &mu, const f32x4 &is, const f32x4 &ga, const f32x4 &be,
                                              int relu) {
    f32x4 o = (x - mu) * is * ga + be;
    if (relu) {
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = o[q] > 0.f ? o[q] : 0.f;
    }
    return o;
}
// backward, front half: returns xh and masks dz in place (the partial-sum kernels need both)
__device__ __forceinline__ f32x4 bn_bwd_front4(const f32x4 &x, f32x4 &dz, const f32x4 &mu, const f32x4 &is, const f32x4 &ga,
                                               const f32x4 &be, int relu) {
    const f32x4 xh = (x - mu) * is;
    if (relu) {
        const f32x4 yv = xh * ga + be;
#pragma unroll
        for (int q = 0; q < 4; ++q) dz[q] = yv[q] > 0.f ? dz[q] : 0.f;
    }
    return xh;
}
__device__ __forceinline__ f32x4 bn_bwd_tail4(const f32x4 &dz, const f32x4 &xh, const f32x4 &a, const f32x4 &b, const f32x4 &d) {
    return a * (dz - b - xh * d);
}
#endif

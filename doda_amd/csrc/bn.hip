// Fused BatchNorm1d(+ReLU) on sparse-tensor features [M, C].
//
// DODA's U-Net is pre-activation: every sparse conv is preceded by BatchNorm1d(eps=1e-4,
// momentum=0.1) -> ReLU on the [M, C] feature matrix (reference model/unet.py:28,42-45,
// model/unet_block.py:23-30,46-49,67-79: 65 BN+ReLU pairs per forward).  Measured on MI355X,
// PyTorch's channels-last BN reductions take ~40 us per call at these shapes and BN is the largest
// single item of the training step, so the pair is provided as three HBM-bound passes:
//   stats   : per-channel mean / biased variance, shifted by the first row so that
//             E[(x-k)^2] - E[x-k]^2 does not cancel (fp32 partials per block, fp64 combine);
//             also applies the running-stat update (momentum, unbiased variance);
//   apply   : y = [relu]((x - mean) * invstd * gamma + beta);
//   backward: dz = dy * [y > 0] (mask recomputed from x, y is never re-read); per-channel sums of
//             dz and dz*xhat (block partials, fp64 combine), then
//             dx = gamma*invstd * (dz - mean(dz) - xhat * mean(dz*xhat)), dgamma, dbeta.
// Lanes own 4-channel fragments (8 B bf16 / 16 B fp32); consecutive lanes walk consecutive
// fragments, so every access is a contiguous wave-wide burst.  All reductions are fixed-order:
// results are run-to-run deterministic.  Algorithmic bytes: fwd 3 passes, bwd 5 passes of M*C*s.
//
// Four forms of the statistics share this file: standalone (bn_stats_partial / bn_stats_final, bn_bwd_partial / bn_bwd_final,
// then the apply sweeps; bn_small_* in one launch up to BN_SMALL_ROWS rows), statistics ROWS of a conv epilogue
// (bn_fwd_final_stats / bn_bwd_final_stats + the apply sweeps, or bn_fused_* in one launch) and fp64 TOTALS (bn_apply /
// bn_bwd_apply<.., TOT>: no reduction launch).  Each piece of arithmetic exists once:
//   bn_totals.hpp   the element (bn_fwd_elem4, bn_bwd_front4 + bn_bwd_tail4; scalar twins for the conv prologue), the per-channel
//                   finish (bn_fwd_finish, bn_unbiased + bn_running, bn_bwd_coef) and the totals prologue's channels;
//   here            partial_park / partial_row (LDS layout, barrier and column sum of the two partial-sum kernels), sum_rows (the statistics
//                   rows, four in flight; first row and stride by the caller), bwd_coef4, apply_grid / plain_grid /
//                   fused_grid / tot_grid_cap, launch_apply / launch_bwd_apply<T, TOT>, BN_DISPATCH (element type),
//                   any_null / add_bad / bn_args_bad and tot_fwd_args / tot_bwd_args for the entry points;
//   common.hpp      al16 and env_ll (with layers.hip).
// Which threads finish which channels differs per form on purpose (see fwd_final_body) and stays with the kernels.
#include "common.hpp"
#include "bn_totals.hpp"

typedef short s16x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) {
    // gfx950: v_cvt_pk_bf16_f32 (round to nearest even, NaN stays NaN) — the integer form cost ten instructions and an
    // EXEC round trip per value in the store epilogues
    return __builtin_bit_cast(unsigned short, (__bf16)f);
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, const f32x4 &v) { *reinterpret_cast<f32x4 *>(p) = v; }

struct F32 {
    typedef float elem;
    static constexpr int W = 1;   // 4-channel fragments per 16-byte access
    static const char *name() { return "F32"; }   // (bn_trace)
    static __device__ __forceinline__ f32x4 load4(const elem *p) { return ld4(p); }
    static __device__ __forceinline__ void store4(elem *p, const f32x4 &v) { st4(p, v); }
    static __device__ __forceinline__ void loadw(const elem *p, f32x4 (&v)[1]) { v[0] = load4(p); }
    static __device__ __forceinline__ void storew(elem *p, const f32x4 (&v)[1]) { store4(p, v[0]); }
};
struct BF16 {
    typedef unsigned short elem;
    static __device__ __forceinline__ f32x4 load4(const elem *p) {
        const s16x4 r = *reinterpret_cast<const s16x4 *>(p);
        return (f32x4){bf2f((unsigned short)r[0]), bf2f((unsigned short)r[1]), bf2f((unsigned short)r[2]), bf2f((unsigned short)r[3])};
    }
    static __device__ __forceinline__ void store4(elem *p, const f32x4 &v) {
        s16x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (short)f2bf(v[q]);
        *reinterpret_cast<s16x4 *>(p) = o;
    }
    static constexpr int W = 2;   // two 4-channel fragments (8 channels) per 16-byte access
    static const char *name() { return "BF16"; }
    typedef short s16x8_ __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ void loadw(const elem *p, f32x4 (&v)[2]) {
        const s16x8_ r = *reinterpret_cast<const s16x8_ *>(p);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            v[h] = (f32x4){bf2f((unsigned short)r[4 * h]), bf2f((unsigned short)r[4 * h + 1]), bf2f((unsigned short)r[4 * h + 2]),
                           bf2f((unsigned short)r[4 * h + 3])};
    }
    static __device__ __forceinline__ void storew(elem *p, const f32x4 (&v)[2]) {
        s16x8_ o;
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = (short)f2bf(v[q >> 2][q & 3]);
        *reinterpret_cast<s16x8_ *>(p) = o;
    }
};

constexpr int BN_BLOCK = 256;
constexpr int BN_MAX_BLOCKS = 1024;

// geometry shared by the reduction kernels: a block covers RPB rows per sweep, lane = (row lane, frag)
struct Geo {
    int nf;    // fragments per row = C/4
    int rpb;   // row lanes per block
};

// ---- the partial-sum kernels' common half: this thread's sums into LDS [rpb][2][c] (partial_park, by the threads that own rows),
// then a fixed-order column sum, one partial row per block (partial_row, all threads)
__device__ __forceinline__ void partial_park(float *lds, int rl, int f, int c, const f32x4 &s1, const f32x4 &s2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lds[(rl * 2 + 0) * c + f * 4 + q] = s1[q];
        lds[(rl * 2 + 1) * c + f * 4 + q] = s2[q];
    }
}
__device__ __forceinline__ void partial_row(const float *lds, int c, int rpb, float *__restrict__ partial /*[blocks][2][C]*/) {
    doda_sync();
    for (int e = threadIdx.x; e < 2 * c; e += BN_BLOCK) {
        float t = 0.f;
        for (int r = 0; r < rpb; ++r) t += lds[r * 2 * c + e];
        partial[(long long)blockIdx.x * 2 * c + e] = t;
    }
}

// ---- pass 1: per-block partial sums of (x-k) and (x-k)^2 -------------------------------------
template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_stats_partial(const typename T::elem *__restrict__ x,
                                                             int m, int c, Geo g,
                                                             float *__restrict__ partial /*[blocks][2][C]*/) {
    extern __shared__ float lds[];  // [rpb][2][C]
    const int f = threadIdx.x % g.nf, rl = threadIdx.x / g.nf;
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
    if (rl < g.rpb) {
        const f32x4 k = T::load4(x + f * 4);  // shift: first row
        for (long long r = (long long)blockIdx.x * g.rpb + rl; r < m; r += (long long)gridDim.x * g.rpb) {
            const f32x4 v = T::load4(x + r * c + f * 4) - k;
            s1 += v;
            s2 += v * v;
        }
        partial_park(lds, rl, f, c, s1, s2);
    }
    partial_row(lds, c, g.rpb, partial);
}

__device__ __forceinline__ double wave_sum(double v) {  // fixed-order butterfly: deterministic
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- combine (one wave per channel): mean, invstd, running stats -------------------------------
template <class T>
__global__ __launch_bounds__(64) void bn_stats_final(const typename T::elem *__restrict__ x,
                                                     const float *__restrict__ partial, int nblocks,
                                                     int m, int c, float eps, float momentum,
                                                     float *__restrict__ mean, float *__restrict__ invstd,
                                                     float *__restrict__ running_mean,
                                                     float *__restrict__ running_var,
                                                     long long *__restrict__ num_batches_tracked) {
    const int ch = blockIdx.x;
    // everything lane 0 needs at the end is requested before the partial sums are read: one memory
    // round trip (2-3 us for a kernel this small) instead of two
    const f32x4 k4 = T::load4(x + (ch & ~3));
    float rm_old = 0.f, rv_old = 0.f;
    long long n_tracked = 0;
    if (threadIdx.x == 0 && running_mean) { rm_old = running_mean[ch]; rv_old = running_var[ch]; }
    if (threadIdx.x == 0 && ch == 0 && num_batches_tracked) n_tracked = *num_batches_tracked;
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) {
        s1 += (double)partial[(long long)b * 2 * c + ch];
        s2 += (double)partial[(long long)b * 2 * c + c + ch];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x != 0) return;
    if (ch == 0 && num_batches_tracked) *num_batches_tracked = n_tracked + 1;
    const BnMoments mo = bn_fwd_finish(s1, s2, m, eps);
    const double mu = (double)k4[ch & 3] + mo.mean;
    mean[ch] = (float)mu;
    invstd[ch] = mo.invstd;
    if (running_mean) {
        running_mean[ch] = bn_running(rm_old, momentum, mu);
        running_var[ch] = bn_running(rv_old, momentum, bn_unbiased(mo.var, m));
    }
}

// ---- statistics from TOTALS (ABI 9) ---------------------------------------------------------------------------------
// The conv epilogues can add their workgroups' (sum, sum of squares) straight into DODA_STATS_SLOTS rows of fp64 totals
// (spconv_common.hpp stats_emit: hardware fp64 atomics, no return) instead of writing one row per workgroup.  The apply
// sweeps below then need no reduction launch in front of them: the first c threads of every workgroup add the eight slots of
// their channel (fixed order, fp64), do the arithmetic of bn_fwd_final_stats / bn_bwd_final_stats and park the per-channel
// vectors in LDS; workgroup 0 publishes what later kernels need.  (Round 3's form of this — the conv kernel's LAST workgroup
// summing the rows behind a ticket — made the conv kernels 15-160 % slower: profiles/r03_stats_finish_ab.txt.)
// ta / tb: the totals of the producers of the columns [0, ca) and [ca, c) (tb null: one producer) — a channel concatenation.
// (TotArgs, tot_sums and the per-channel arithmetic: bn_totals.hpp — shared with the conv kernels that fold a BatchNorm into their gather)
__device__ __forceinline__ void tot_fwd_prologue(const TotArgs &t, int c, float *v_mu, float *v_is) {
    for (int ch = threadIdx.x; ch < c; ch += BN_BLOCK) {
        float mu, is;
        tot_fwd_channel(t, c, ch, blockIdx.x == 0, mu, is);
        v_mu[ch] = mu;
        v_is[ch] = is;
    }
    doda_sync();
}
__device__ __forceinline__ void tot_bwd_prologue(const TotArgs &t, int c, const float *__restrict__ invstd,
                                                 const float *__restrict__ gamma, float *v_co /*[3][c]*/) {
    for (int ch = threadIdx.x; ch < c; ch += BN_BLOCK) {
        float ca, cb, cd;
        tot_bwd_channel(t, c, ch, blockIdx.x == 0, invstd[ch], gamma[ch], ca, cb, cd);   // dx = a * (dz - b - xhat * d)
        v_co[ch] = ca;
        v_co[c + ch] = cb;
        v_co[2 * c + ch] = cd;
    }
    doda_sync();
}

// ---- pass 2: normalise + affine (+ReLU) --------------------------------------------------------
// Round 3: the launcher picks a grid whose thread count is a multiple of the fragments per row, so a thread's channels
// never change while it strides over the rows: the per-channel vectors are loaded ONCE into registers (they used to be
// four extra vector loads per 8 bytes of payload — the sweep was bound by the texture path's instruction rate, 3.3 TB/s
// at level 1, not by HBM), and bf16 rows move in 16-byte accesses (two fragments per thread).  Same arithmetic, same
// order: results unchanged bit for bit.  FIXED = false: the general form (any grid).
template <class T, bool FIXED, bool TOT = false>
__global__ __launch_bounds__(BN_BLOCK) void bn_apply(const typename T::elem *__restrict__ x,
                                                     long long n_frag, int nf,
                                                     const float *mean,
                                                     const float *invstd,
                                                     const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, int relu,
                                                     typename T::elem *__restrict__ y, const TotArgs tot = TotArgs()) {
    // (round 6) FIXED: this thread's first rows are REQUESTED before the totals prologue (its fp64 arithmetic and barrier are a
    // dependent round trip of their own): with the whole grid resident at once (tot_grid_cap) every workgroup used to sit
    // through the prologue with no row in flight — 12-16 us per level-1 sweep of 38 MB in the step, 7.5 us without the prologue
    f32x4 pre_v[T::W];
    [[maybe_unused]] bool pre_have = false;
    if constexpr (FIXED && TOT) {
        const long long n_w0 = n_frag / T::W, e00 = (long long)blockIdx.x * BN_BLOCK + threadIdx.x;
        pre_have = e00 < n_w0;
        T::loadw(x + (pre_have ? e00 : 0) * (4 * T::W), pre_v);
    }
    if constexpr (TOT) {   // mean / invstd from the totals, through LDS
        __shared__ __attribute__((aligned(16))) float v_mu[BN_TOT_MAX_C], v_is[BN_TOT_MAX_C];
        tot_fwd_prologue(tot, nf * 4, v_mu, v_is);
        mean = v_mu;
        invstd = v_is;
    }
    if constexpr (FIXED) {
        constexpr int W = T::W;
        const long long n_w = n_frag / W, e0 = (long long)blockIdx.x * BN_BLOCK + threadIdx.x;
        const int f = (int)(e0 % (nf / W)) * W;
        f32x4 mu[W], is[W], ga[W], be[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            mu[w] = ld4(mean + (f + w) * 4);
            is[w] = ld4(invstd + (f + w) * 4);
            ga[w] = ld4(gamma + (f + w) * 4);
            be[w] = ld4(beta + (f + w) * 4);
        }
        for (long long e = e0; e < n_w; e += (long long)gridDim.x * BN_BLOCK) {
            f32x4 v[W];
            if (TOT && e == e0) {
#pragma unroll
                for (int w = 0; w < W; ++w) v[w] = pre_v[w];
            } else T::loadw(x + e * (4 * W), v);
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = bn_fwd_elem4(v[w], mu[w], is[w], ga[w], be[w], relu);
            T::storew(y + e * (4 * W), v);
        }
        return;
    }
    for (long long e = (long long)blockIdx.x * BN_BLOCK + threadIdx.x; e < n_frag;
         e += (long long)gridDim.x * BN_BLOCK) {
        const int f = (int)(e % nf);
        T::store4(y + e * 4, bn_fwd_elem4(T::load4(x + e * 4), ld4(mean + f * 4), ld4(invstd + f * 4), ld4(gamma + f * 4),
                                          ld4(beta + f * 4), relu));
    }
}

// grid of a sweep without a fixed column per thread: one workgroup per BN_BLOCK fragments, at most `cap`
inline int plain_grid(long long n_frag, int cap = 4096) {
    return (int)((n_frag + BN_BLOCK - 1) / BN_BLOCK < cap ? (n_frag + BN_BLOCK - 1) / BN_BLOCK : cap);
}
// grid of an apply sweep: as many workgroups as fragments need (<= cap), rounded DOWN so that the thread count is a
// multiple of the 16-byte columns per row (then FIXED applies); *fixed = false when no such grid exists or an operand is
// not `aligned` for 16-byte accesses: then the plain grid of the general sweep
inline int apply_grid(long long n_frag, int nf, int W, bool aligned, int cap, bool *fixed) {
    *fixed = false;
    if (!aligned || nf % W != 0 || n_frag % W != 0) return plain_grid(n_frag);
    const int cols = nf / W;
    long long grid = (n_frag / W + BN_BLOCK - 1) / BN_BLOCK;
    if (grid > cap) grid = cap;
    if (grid < 1) grid = 1;
    int a = cols, b = BN_BLOCK;            // q = cols / gcd(cols, BN_BLOCK): grid must be a multiple of q
    while (b) { const int t = a % b; a = b; b = t; }
    const int q = cols / a;
    if (grid < q) return plain_grid(n_frag);
    *fixed = true;
    return (int)(grid - grid % q);
}

// ---- backward pass 1: per-block partial sums of dz and dz*xhat --------------------------------
template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_bwd_partial(const typename T::elem *__restrict__ x,
                                                           const typename T::elem *__restrict__ dy,
                                                           int m, int c, Geo g,
                                                           const float *__restrict__ mean,
                                                           const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, int relu,
                                                           float *__restrict__ partial) {
    extern __shared__ float lds[];
    const int f = threadIdx.x % g.nf, rl = threadIdx.x / g.nf;
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
    if (rl < g.rpb) {
        const f32x4 mu = ld4(mean + f * 4), is = ld4(invstd + f * 4), ga = ld4(gamma + f * 4), be = ld4(beta + f * 4);
        for (long long r = (long long)blockIdx.x * g.rpb + rl; r < m; r += (long long)gridDim.x * g.rpb) {
            f32x4 dz = T::load4(dy + r * c + f * 4);
            const f32x4 xh = bn_bwd_front4(T::load4(x + r * c + f * 4), dz, mu, is, ga, be, relu);
            s1 += dz;
            s2 += dz * xh;
        }
        partial_park(lds, rl, f, c, s1, s2);
    }
    partial_row(lds, c, g.rpb, partial);
}

__global__ __launch_bounds__(64) void bn_bwd_final(const float *__restrict__ partial, int nblocks,
                                                   int m, int c, const float *__restrict__ invstd,
                                                   const float *__restrict__ gamma,
                                                   float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                   float *__restrict__ coef /*[3][C]*/) {
    const int ch = blockIdx.x;
    const float ga = gamma[ch], is = invstd[ch];   // requested before the partial sums (see bn_stats_final)
    double s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) {
        s1 += (double)partial[(long long)b * 2 * c + ch];
        s2 += (double)partial[(long long)b * 2 * c + c + ch];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x != 0) return;
    const BnBwdCoef k = bn_bwd_coef(s1, s2, m, ga, is);
    dbeta[ch] = k.dbeta;
    dgamma[ch] = k.dgamma;
    coef[ch] = k.a;
    coef[c + ch] = k.b;
    coef[2 * c + ch] = k.d;
}

template <class T, bool FIXED, bool TOT = false>
__global__ __launch_bounds__(BN_BLOCK) void bn_bwd_apply(const typename T::elem *__restrict__ x,
                                                         const typename T::elem *__restrict__ dy,
                                                         long long n_frag, int nf, int c,
                                                         const float *__restrict__ mean,
                                                         const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, int relu,
                                                         const float *coef,
                                                         typename T::elem *__restrict__ dx,
                                                         const typename T::elem *__restrict__ add, int add_ld = 0,
                                                         const TotArgs tot = TotArgs()) {
    f32x4 pre_x[T::W], pre_dz[T::W], pre_av[T::W];   // (round 6: first rows requested before the totals prologue, see bn_apply)
    if constexpr (FIXED && TOT) {
        const int cols0 = nf / T::W;
        const long long n_w0 = n_frag / T::W, e00 = (long long)blockIdx.x * BN_BLOCK + threadIdx.x;
        const long long ee = e00 < n_w0 ? e00 : 0;
        T::loadw(x + ee * (4 * T::W), pre_x);
        T::loadw(dy + ee * (4 * T::W), pre_dz);
        if (add) T::loadw(add_ld ? add + (ee / cols0) * add_ld + (int)(ee % cols0) * T::W * 4 : add + ee * (4 * T::W), pre_av);
    }
    if constexpr (TOT) {   // the three coefficient vectors from the totals, through LDS
        __shared__ __attribute__((aligned(16))) float v_co[3 * BN_TOT_MAX_C];
        tot_bwd_prologue(tot, c, invstd, gamma, v_co);
        coef = v_co;
    }
    if constexpr (FIXED) {   // (see bn_apply: per-thread channel vectors in registers, 16-byte accesses)
        constexpr int W = T::W;
        const int cols = nf / W;
        const long long n_w = n_frag / W, e0 = (long long)blockIdx.x * BN_BLOCK + threadIdx.x;
        const int f = (int)(e0 % cols) * W;
        f32x4 mu[W], is[W], ga[W], be[W], ca[W], cb[W], cd[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            mu[w] = ld4(mean + (f + w) * 4);
            is[w] = ld4(invstd + (f + w) * 4);
            ga[w] = ld4(gamma + (f + w) * 4);
            be[w] = ld4(beta + (f + w) * 4);
            ca[w] = ld4(coef + (f + w) * 4);
            cb[w] = ld4(coef + c + (f + w) * 4);
            cd[w] = ld4(coef + 2 * c + (f + w) * 4);
        }
        for (long long e = e0; e < n_w; e += (long long)gridDim.x * BN_BLOCK) {
            f32x4 xv[W], dz[W], av[W];
            if (TOT && e == e0) {
#pragma unroll
                for (int w = 0; w < W; ++w) { xv[w] = pre_x[w]; dz[w] = pre_dz[w]; av[w] = pre_av[w]; }
            } else {
                T::loadw(x + e * (4 * W), xv);
                T::loadw(dy + e * (4 * W), dz);
                if (add) T::loadw(add_ld ? add + (e / cols) * add_ld + f * 4 : add + e * (4 * W), av);
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const f32x4 xh = bn_bwd_front4(xv[w], dz[w], mu[w], is[w], ga[w], be[w], relu);
                f32x4 o = bn_bwd_tail4(dz[w], xh, ca[w], cb[w], cd[w]);
                if (add) o += av[w];
                xv[w] = o;
            }
            T::storew(dx + e * (4 * W), xv);
        }
        return;
    }
    for (long long e = (long long)blockIdx.x * BN_BLOCK + threadIdx.x; e < n_frag;
         e += (long long)gridDim.x * BN_BLOCK) {
        const int f = (int)(e % nf);
        f32x4 dz = T::load4(dy + e * 4);
        const f32x4 xh = bn_bwd_front4(T::load4(x + e * 4), dz, ld4(mean + f * 4), ld4(invstd + f * 4), ld4(gamma + f * 4),
                                       ld4(beta + f * 4), relu);
        f32x4 o = bn_bwd_tail4(dz, xh, ld4(coef + f * 4), ld4(coef + c + f * 4), ld4(coef + 2 * c + f * 4));
        // a second gradient of x (residual / skip path) summed here; add_ld != 0: its rows lie add_ld elements apart
        // (a column slice of a wider matrix: the gradient of torch.cat's input, reference model/unet_block.py:93)
        if (add) o += T::load4(add_ld ? add + (e / nf) * add_ld + f * 4 : add + e * 4);
        T::store4(dx + e * 4, o);
    }
}

// DODA_BN_TOT_GRID: cap of the totals sweeps' grids.  (round 6) at most 1024 workgroups (4 per CU, all resident at once): every
// workgroup pays the totals prologue — 16 doubles per channel out of padded 128-byte lines, fp64 division / square root, a barrier —
// once per ~5 x 16 bytes per thread at level 1 instead of once per 16 bytes.  In-step sums of bn_apply + bn_bwd_apply
// (tools/layers_prof.sh): 4096 workgroups 613 us, 2048 573, 1024 518, 768 518, 512 531, 256 667
inline int tot_grid_cap() {
    static const int cap = [] { const int v = (int)env_ll("DODA_BN_TOT_GRID", 1024); return v < 64 ? 64 : v > 4096 ? 4096 : v; }();
    return cap;
}
// TOT: mean / invstd (forward) and coef (backward) are unused — the kernels derive them from `tot`
template <class T, bool TOT>
int launch_apply(const void *x_, long long n_frag, int nf, const float *mean, const float *invstd, const float *gamma,
                 const float *beta, int relu, void *y_, const TotArgs &tot, hipStream_t s) {
    typedef typename T::elem elem;
    const elem *x = (const elem *)x_;
    elem *y = (elem *)y_;
    bool fixed;
    const int grid = apply_grid(n_frag, nf, T::W, al16(x) && al16(y), TOT ? tot_grid_cap() : 4096, &fixed);
    bn_trace(grid, BN_BLOCK, "bn_apply<%s, %s, %s>", T::name(), fixed ? "true" : "false", TOT ? "true" : "false");
    hipLaunchKernelGGL((fixed ? bn_apply<T, true, TOT> : bn_apply<T, false, TOT>), dim3(grid), dim3(BN_BLOCK), 0, s, x, n_frag, nf, mean,
                       invstd, gamma, beta, relu, y, tot);
    return doda_check_launch();
}
template <class T, bool TOT>
int launch_bwd_apply(const void *x_, const void *dy_, long long n_frag, int nf, int c, const float *mean, const float *invstd,
                     const float *gamma, const float *beta, int relu, const float *coef, void *dx_, const void *add_, int add_ld,
                     const TotArgs &tot, hipStream_t s) {
    typedef typename T::elem elem;
    const elem *x = (const elem *)x_, *dy = (const elem *)dy_, *add = (const elem *)add_;
    elem *dx = (elem *)dx_;
    const bool aligned = al16(x) && al16(dy) && al16(dx) && (!add || (al16(add) && add_ld % (4 * T::W) == 0));
    bool fixed;
    const int grid = apply_grid(n_frag, nf, T::W, aligned, TOT ? tot_grid_cap() : 4096, &fixed);
    bn_trace(grid, BN_BLOCK, "bn_bwd_apply<%s, %s, %s>", T::name(), fixed ? "true" : "false", TOT ? "true" : "false");
    hipLaunchKernelGGL((fixed ? bn_bwd_apply<T, true, TOT> : bn_bwd_apply<T, false, TOT>), dim3(grid), dim3(BN_BLOCK), 0, s, x, dy, n_frag,
                       nf, c, mean, invstd, gamma, beta, relu, coef, dx, add, add_ld, tot);
    return doda_check_launch();
}

// ---- small-M variants: ONE launch per direction --------------------------------------------------
// Deep U-Net levels have a few hundred to ~10k rows; three launches per BN pass are then pure
// launch-floor time.  Here a block owns one 4-channel fragment column over ALL rows, so the
// statistics need no cross-block step: sweep 1 reduces, sweep 2 applies (rows stay in L2).
constexpr int BN_SMALL_ROWS = 4096;   // measured: at ~11k rows the C/4 blocks of this form take up to 80 us

// both sums through ONE LDS exchange (the small kernels are launch-floor kernels: every barrier pair counts)
__device__ __forceinline__ void block_sum4x2(f32x4 &a, f32x4 &b, float (*lds)[8]) {  // 256 threads, fixed order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] += __shfl_xor(a[q], d, 64); b[q] += __shfl_xor(b[q], d, 64); }
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { lds[wid][q] = a[q]; lds[wid][4 + q] = b[q]; }
    }
    doda_sync();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = (lds[0][q] + lds[1][q]) + (lds[2][q] + lds[3][q]);
        b[q] = (lds[0][4 + q] + lds[1][4 + q]) + (lds[2][4 + q] + lds[3][4 + q]);
    }
}

template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_small_fwd(const typename T::elem *__restrict__ x, int m,
                                                         int c, float eps, float momentum,
                                                         const float *__restrict__ gamma,
                                                         const float *__restrict__ beta,
                                                         float *__restrict__ running_mean,
                                                         float *__restrict__ running_var,
                                                         long long *__restrict__ nbt, int relu,
                                                         typename T::elem *__restrict__ y,
                                                         float *__restrict__ mean,
                                                         float *__restrict__ invstd) {
    __shared__ float lds[4][8];
    const int f = blockIdx.x;
    // Every global read of the kernel is issued up front and independently (rows past m re-read row
    // m-1 and are masked): a dependent round trip to L2/HBM costs 2-3 us here and the old form had
    // four of them in series (shift row, stats sweep, affine parameters, apply sweep).
    constexpr int RPT = BN_SMALL_ROWS / BN_BLOCK;
    const f32x4 k = T::load4(x + f * 4);
    const f32x4 ga = ld4(gamma + f * 4), be = ld4(beta + f * 4);
    // (the running statistics and the batch counter too: updating them element by element at the end
    // cost thread 0 five more dependent round trips)
    f32x4 rm = {0, 0, 0, 0}, rv = {0, 0, 0, 0};
    long long n_tracked = 0;
    if (threadIdx.x == 0 && running_mean) {
        rm = ld4(running_mean + f * 4);
        rv = ld4(running_var + f * 4);
    }
    if (threadIdx.x == 0 && f == 0 && nbt) n_tracked = *nbt;
    f32x4 xv[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = threadIdx.x + i * BN_BLOCK;
        xv[i] = T::load4(x + (long long)(r < m ? r : m - 1) * c + f * 4);
    }
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const f32x4 v = xv[i] - k;
        const float w = threadIdx.x + i * BN_BLOCK < m ? 1.f : 0.f;
        s1 += v * w;
        s2 += v * v * w;
    }
    block_sum4x2(s1, s2, lds);
    f32x4 mu, is;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const BnMoments mo = bn_fwd_finish((double)s1[q], (double)s2[q], m, eps);
        const double muq = (double)k[q] + mo.mean;
        mu[q] = (float)muq;
        is[q] = mo.invstd;
        rm[q] = bn_running(rm[q], momentum, muq);
        rv[q] = bn_running(rv[q], momentum, bn_unbiased(mo.var, m));
    }
    if (threadIdx.x == 0) {
        st4(mean + f * 4, mu);
        st4(invstd + f * 4, is);
        if (running_mean) {
            st4(running_mean + f * 4, rm);
            st4(running_var + f * 4, rv);
        }
        if (f == 0 && nbt) *nbt = n_tracked + 1;
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = threadIdx.x + i * BN_BLOCK;
        if (r < m) T::store4(y + (long long)r * c + f * 4, bn_fwd_elem4(xv[i], mu, is, ga, be, relu));
    }
}

template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_small_bwd(const typename T::elem *__restrict__ x,
                                                         const typename T::elem *__restrict__ dy,
                                                         int m, int c, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, int relu,
                                                         typename T::elem *__restrict__ dx,
                                                         float *__restrict__ dgamma,
                                                         float *__restrict__ dbeta,
                                                         const typename T::elem *__restrict__ add, int add_ld = 0) {
    __shared__ float lds[4][8];
    const int f = blockIdx.x;
    const f32x4 mu = ld4(mean + f * 4), is = ld4(invstd + f * 4), ga = ld4(gamma + f * 4), be = ld4(beta + f * 4);
    constexpr int RPT = BN_SMALL_ROWS / BN_BLOCK;
    f32x4 xh[RPT], dz[RPT], ad[RPT];   // all reads up front, kept for the apply pass (see bn_small_fwd)
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = threadIdx.x + i * BN_BLOCK;
        const long long off = (long long)(r < m ? r : m - 1) * c + f * 4;
        xh[i] = T::load4(x + off);
        dz[i] = T::load4(dy + off);
        ad[i] = add ? T::load4(add_ld ? add + (long long)(r < m ? r : m - 1) * add_ld + f * 4 : add + off) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        xh[i] = bn_bwd_front4(xh[i], dz[i], mu, is, ga, be, relu);
        const float w = threadIdx.x + i * BN_BLOCK < m ? 1.f : 0.f;
        s1 += dz[i] * w;
        s2 += dz[i] * xh[i] * w;
    }
    block_sum4x2(s1, s2, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { dbeta[f * 4 + q] = s1[q]; dgamma[f * 4 + q] = s2[q]; }
    }
    const float inv_m = 1.f / (float)m;
    const f32x4 a = ga * is, b = s1 * inv_m, d = s2 * inv_m;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = threadIdx.x + i * BN_BLOCK;
        if (r < m) T::store4(dx + (long long)r * c + f * 4, bn_bwd_tail4(dz[i], xh[i], a, b, d) + ad[i]);
    }
}

// ---- statistics delivered by a conv epilogue (doda_spconv_gather_ex) ---------------------------------
// `stats` = [rows][2][c] partial sums, one row per workgroup tile of the conv.  One block per 4-channel
// fragment: 256 threads walk the rows with 16-byte loads, fp64 sums, fixed-order tree in LDS.
// both sums at once: one pair of barriers instead of two (the `final` kernels are launch-floor kernels: 75 per step)
__device__ __forceinline__ void block_sum_d8(double (&a)[4], double (&b)[4], double (*lds)[8]) {   // 256 threads, fixed order
#pragma unroll
    for (int q = 0; q < 4; ++q) { a[q] = wave_sum(a[q]); b[q] = wave_sum(b[q]); }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { lds[wid][q] = a[q]; lds[wid][4 + q] = b[q]; }
    }
    doda_sync();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        a[q] = (lds[0][q] + lds[1][q]) + (lds[2][q] + lds[3][q]);
        b[q] = (lds[0][4 + q] + lds[1][4 + q]) + (lds[2][4 + q] + lds[3][4 + q]);
    }
}

// this thread's share of the partial rows of channel quad f: rows r0, r0 + step, ...  Four rows per trip with all eight loads
// issued before the first add: a level-1 layer has ~4700 partial rows and four blocks to reduce them, so
// the kernel is a chain of L2 round trips (13.4 us with one row per trip)
__device__ __forceinline__ void sum_rows(const float *__restrict__ stats, int rows, int c, int f, int r0, int step,
                                         double (&s1)[4], double (&s2)[4]) {
    int r = r0;
    for (; r + 3 * step < rows; r += 4 * step) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float *p = stats + (long long)(r + k * step) * 2 * c + f * 4;
            a[k] = ld4(p);
            b[k] = ld4(p + c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) { s1[q] += (double)a[k][q]; s2[q] += (double)b[k][q]; }
    }
    for (; r < rows; r += step) {
        const f32x4 a = ld4(stats + (long long)r * 2 * c + f * 4);
        const f32x4 b = ld4(stats + (long long)r * 2 * c + c + f * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { s1[q] += (double)a[q]; s2[q] += (double)b[q]; }
    }
}

// (bodies as device functions: the chained kernels below run them in their first workgroups)
__device__ __forceinline__ void fwd_final_body(int f, const float *__restrict__ stats, int rows, int m, int c, float eps,
                                               float momentum, float *__restrict__ mean, float *__restrict__ invstd,
                                               float *__restrict__ running_mean, float *__restrict__ running_var,
                                               long long *__restrict__ nbt) {
    __shared__ double lds[4][8];
    // threads 0..3 finish one channel each (the fp64 divide / square root chains of the four channels side by side);
    // what they need at the end is requested before the partial sums: one round trip, not two
    const int q = threadIdx.x & 3;
    float rm = 0.f, rv = 0.f;
    long long n_tracked = 0;
    if (threadIdx.x < 4 && running_mean) {
        rm = running_mean[f * 4 + q];
        rv = running_var[f * 4 + q];
    }
    if (threadIdx.x == 0 && f == 0 && nbt) n_tracked = *nbt;
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    sum_rows(stats, rows, c, f, threadIdx.x, BN_BLOCK, s1, s2);
    block_sum_d8(s1, s2, lds);
    if (threadIdx.x >= 4) return;
    double a1 = s1[0], a2 = s2[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) { if (q == k) { a1 = s1[k]; a2 = s2[k]; } }
    const BnMoments mo = bn_fwd_finish(a1, a2, m, eps);
    mean[f * 4 + q] = (float)mo.mean;
    invstd[f * 4 + q] = mo.invstd;
    if (running_mean) {
        running_mean[f * 4 + q] = bn_running(rm, momentum, mo.mean);
        running_var[f * 4 + q] = bn_running(rv, momentum, bn_unbiased(mo.var, m));
    }
    if (threadIdx.x == 0 && f == 0 && nbt) *nbt = n_tracked + 1;
}

__global__ __launch_bounds__(BN_BLOCK) void bn_fwd_final_stats(const float *__restrict__ stats, int rows, int m, int c,
                                                               float eps, float momentum, float *__restrict__ mean,
                                                               float *__restrict__ invstd,
                                                               float *__restrict__ running_mean,
                                                               float *__restrict__ running_var,
                                                               long long *__restrict__ nbt) {
    fwd_final_body(blockIdx.x, stats, rows, m, c, eps, momentum, mean, invstd, running_mean, running_var, nbt);
}

// bn_bwd_coef for the four channels of a fragment
__device__ __forceinline__ void bwd_coef4(const double (&s1)[4], const double (&s2)[4], int m, const f32x4 &ga, const f32x4 &is,
                                          f32x4 &a, f32x4 &b, f32x4 &d, f32x4 &dg, f32x4 &db) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const BnBwdCoef k = bn_bwd_coef(s1[q], s2[q], m, ga[q], is[q]);
        a[q] = k.a; b[q] = k.b; d[q] = k.d; dg[q] = k.dgamma; db[q] = k.dbeta;
    }
}

__device__ __forceinline__ void bwd_final_body(int f, const float *__restrict__ stats, int rows, int m, int c,
                                               const float *__restrict__ invstd, const float *__restrict__ gamma,
                                               float *__restrict__ dgamma, float *__restrict__ dbeta,
                                               float *__restrict__ coef /*[3][C]*/) {
    __shared__ double lds[4][8];
    const f32x4 ga = ld4(gamma + f * 4), is = ld4(invstd + f * 4);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    sum_rows(stats, rows, c, f, threadIdx.x, BN_BLOCK, s1, s2);
    block_sum_d8(s1, s2, lds);
    if (threadIdx.x != 0) return;
    f32x4 db, dg, a, bb, dd;
    bwd_coef4(s1, s2, m, ga, is, a, bb, dd, dg, db);
    st4(dbeta + f * 4, db);
    st4(dgamma + f * 4, dg);
    st4(coef + f * 4, a);           // dx = a * (dz - b - xhat * d)
    st4(coef + c + f * 4, bb);
    st4(coef + 2 * c + f * 4, dd);
}

__global__ __launch_bounds__(BN_BLOCK) void bn_bwd_final_stats(const float *__restrict__ stats, int rows, int m, int c,
                                                               const float *__restrict__ invstd,
                                                               const float *__restrict__ gamma,
                                                               float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                               float *__restrict__ coef /*[3][C]*/) {
    bwd_final_body(blockIdx.x, stats, rows, m, c, invstd, gamma, dgamma, dbeta, coef);
}

// ---- final + apply in ONE launch (round 3) ----------------------------------------------------------
// The `final` kernels above are four to twelve blocks chasing L2 round trips: 6-7 us each, 75 of them per U-Net
// step.  When the conv epilogue delivers few partial rows (the persistent tile kernels write ONE per workgroup:
// <= 768 rows, ~100 KB) every workgroup of the apply pass can afford to reduce them itself — same rows, same
// order, same fp64 combine in every workgroup, so all of them arrive at identical statistics — and the dependent
// launch disappears.  A fixed grid of BN_FUSED_BLOCKS workgroups keeps the redundant reads (grid x partial bytes,
// L2 hits) well below the tensor itself; mean / invstd / gamma / beta (or the backward coefficients) then sit in
// LDS for the apply sweep instead of being re-read per element.  Workgroup 0 publishes the statistics.
constexpr int BN_FUSED_BLOCKS = 256;
constexpr int BN_FUSED_MAX_PARTIAL_BYTES = 160 * 1024;
constexpr int BN_FUSED_MAX_C = 64;          // channels whose vectors fit the LDS arrays below

// every thread's share of the partial rows of its fragment: thread = (row lane rl, fragment f); returns the totals of
// fragment f in all threads with rl == 0 ... through LDS, fixed order
__device__ __forceinline__ void fused_reduce(const float *__restrict__ stats, int rows, int c, int nf, int rpb,
                                             double (*red)[8], double (&s1)[4], double (&s2)[4]) {
    const int f = threadIdx.x % nf, rl = threadIdx.x / nf;
#pragma unroll
    for (int q = 0; q < 4; ++q) { s1[q] = 0.0; s2[q] = 0.0; }
    if (rl < rpb) sum_rows(stats, rows, c, f, rl, rpb, s1, s2);
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[threadIdx.x][q] = s1[q]; red[threadIdx.x][4 + q] = s2[q]; }
    doda_sync();
    if (rl == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { s1[q] = 0.0; s2[q] = 0.0; }
        for (int k = 0; k < rpb; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { s1[q] += red[k * nf + f][q]; s2[q] += red[k * nf + f][4 + q]; }
        }
    }
}

template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_fused_fwd(const typename T::elem *__restrict__ x, long long n_frag, int nf,
                                                         int rpb, const float *__restrict__ stats, int rows, int m,
                                                         float eps, float momentum, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float *__restrict__ mean,
                                                         float *__restrict__ invstd, float *__restrict__ running_mean,
                                                         float *__restrict__ running_var, long long *__restrict__ nbt,
                                                         int relu, typename T::elem *__restrict__ y) {
    __shared__ double red[BN_BLOCK][8];
    __shared__ f32x4 v_mu[BN_FUSED_MAX_C / 4], v_is[BN_FUSED_MAX_C / 4];
    const int c = nf * 4;
    double s1[4], s2[4];
    fused_reduce(stats, rows, c, nf, rpb, red, s1, s2);
    if (threadIdx.x < nf) {
        const int f = threadIdx.x;
        f32x4 mu, is;
        BnMoments mo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mo[q] = bn_fwd_finish(s1[q], s2[q], m, eps);
            mu[q] = (float)mo[q].mean;
            is[q] = mo[q].invstd;
        }
        v_mu[f] = mu;      // (the apply sweep evaluates (x - mean) * invstd * gamma + beta exactly as bn_apply does)
        v_is[f] = is;
        if (blockIdx.x == 0) {
            st4(mean + f * 4, mu);
            st4(invstd + f * 4, is);
            if (running_mean) {
                f32x4 rm = ld4(running_mean + f * 4), rv = ld4(running_var + f * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    rm[q] = bn_running(rm[q], momentum, mo[q].mean);
                    rv[q] = bn_running(rv[q], momentum, bn_unbiased(mo[q].var, m));
                }
                st4(running_mean + f * 4, rm);
                st4(running_var + f * 4, rv);
            }
            if (f == 0 && nbt) *nbt = *nbt + 1;
        }
    }
    doda_sync();
    for (long long e = (long long)blockIdx.x * BN_BLOCK + threadIdx.x; e < n_frag; e += (long long)gridDim.x * BN_BLOCK) {
        const int f = (int)(e % nf);
        T::store4(y + e * 4, bn_fwd_elem4(T::load4(x + e * 4), v_mu[f], v_is[f], ld4(gamma + f * 4), ld4(beta + f * 4), relu));
    }
}

template <class T>
__global__ __launch_bounds__(BN_BLOCK) void bn_fused_bwd(const typename T::elem *__restrict__ x,
                                                         const typename T::elem *__restrict__ dy, long long n_frag,
                                                         int nf, int rpb, const float *__restrict__ stats, int rows,
                                                         int m, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd,
                                                         const float *__restrict__ gamma, const float *__restrict__ beta,
                                                         int relu, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                         typename T::elem *__restrict__ dx,
                                                         const typename T::elem *__restrict__ add) {
    __shared__ double red[BN_BLOCK][8];
    __shared__ f32x4 v_a[BN_FUSED_MAX_C / 4], v_b[BN_FUSED_MAX_C / 4], v_d[BN_FUSED_MAX_C / 4];
    const int c = nf * 4;
    double s1[4], s2[4];
    fused_reduce(stats, rows, c, nf, rpb, red, s1, s2);
    if (threadIdx.x < nf) {
        const int f = threadIdx.x;
        f32x4 db, dg, a, bb, dd;
        bwd_coef4(s1, s2, m, ld4(gamma + f * 4), ld4(invstd + f * 4), a, bb, dd, dg, db);
        v_a[f] = a; v_b[f] = bb; v_d[f] = dd;
        if (blockIdx.x == 0) {
            st4(dbeta + f * 4, db);
            st4(dgamma + f * 4, dg);
        }
    }
    doda_sync();
    for (long long e = (long long)blockIdx.x * BN_BLOCK + threadIdx.x; e < n_frag; e += (long long)gridDim.x * BN_BLOCK) {
        const int f = (int)(e % nf);
        f32x4 dz = T::load4(dy + e * 4);
        const f32x4 xh = bn_bwd_front4(T::load4(x + e * 4), dz, ld4(mean + f * 4), ld4(invstd + f * 4), ld4(gamma + f * 4),
                                       ld4(beta + f * 4), relu);
        f32x4 o = bn_bwd_tail4(dz, xh, v_a[f], v_b[f], v_d[f]);
        if (add) o += T::load4(add + e * 4);
        T::store4(dx + e * 4, o);
    }
}

constexpr long long BN_FUSED_SMALL_ELEMS = 2500000;   // m * c up to which the one-launch form is the default (levels 3-4: 35-46k x 48, 8-11k x 64)
inline bool fused_ok(int rows, int c, int m) {
    // For LARGE tensors off by default: measured in the U-Net step (same box, alternating runs) 7.7-7.8 ms against
    // 6.45-6.54 ms — a 256-workgroup apply sweep is far below the HBM rate the 4096-block one reaches, and more workgroups
    // multiply the redundant partial reads; DODA_BN_FUSED_FINAL=1 switches it on everywhere (parity tests).
    // SMALL tensors (levels 3-4 of the U-Net; the levels below take the one-launch bn_small_*):
    // both launches are launch-floor kernels (5 + 5 us) and the sweep is a few workgroups — one launch (round 3,
    // DODA_BN_FUSED_SMALL=0 switches that off).
    static const bool on = getenv("DODA_BN_FUSED_FINAL") && getenv("DODA_BN_FUSED_FINAL")[0] == '1';
    // DODA_BN_FUSED_SMALL: 0 = off, 1 / unset = the default threshold, larger values = that many elements
    static const long long small_elems = [] { const long long v = env_ll("DODA_BN_FUSED_SMALL", 1); return v == 1 ? BN_FUSED_SMALL_ELEMS : v; }();
    const bool want = on || (long long)m * c <= small_elems;
    return want && c <= BN_FUSED_MAX_C && c / 4 <= BN_BLOCK && (long long)rows * 2 * c * 4 <= BN_FUSED_MAX_PARTIAL_BYTES;
}
inline int fused_grid(long long n_frag) { return plain_grid(n_frag, BN_FUSED_BLOCKS); }

Geo make_geo(int c) {
    Geo g;
    g.nf = c / 4;
    g.rpb = BN_BLOCK / g.nf;
    if (g.rpb < 1) g.rpb = 1;
    return g;
}

int n_blocks_for(int m, const Geo &g) {
    int nb = div_up(m, g.rpb * 8);  // >= 8 rows per lane
    if (nb > BN_MAX_BLOCKS) nb = BN_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    return nb;
}

template <class T>
int run_fwd(const void *x_, int m, int c, float eps, float momentum, const float *gamma,
            const float *beta, float *running_mean, float *running_var, long long *nbt, int training,
            int relu, void *y_, float *mean, float *invstd, void *ws, size_t ws_bytes, hipStream_t s) {
    typedef typename T::elem elem;
    const elem *x = (const elem *)x_;
    const Geo g = make_geo(c);
    if (training && m <= BN_SMALL_ROWS) {
        bn_trace(c / 4, BN_BLOCK, "bn_small_fwd<%s>", T::name());
        hipLaunchKernelGGL((bn_small_fwd<T>), dim3(c / 4), dim3(BN_BLOCK), 0, s, x, m, c, eps, momentum,
                           gamma, beta, running_mean, running_var, nbt, relu, (elem *)y_, mean, invstd);
        return doda_check_launch();
    }
    if (training) {
        const int nb = n_blocks_for(m, g);
        if (ws_bytes < (size_t)nb * 2 * c * 4) return DODA_ERR_WORKSPACE;
        float *partial = (float *)ws;
        bn_trace(nb, BN_BLOCK, "bn_stats_partial<%s>", T::name());
        bn_trace(c, 64, "bn_stats_final<%s>", T::name());
        hipLaunchKernelGGL((bn_stats_partial<T>), dim3(nb), dim3(BN_BLOCK), (size_t)g.rpb * 2 * c * 4, s,
                           x, m, c, g, partial);
        hipLaunchKernelGGL((bn_stats_final<T>), dim3(c), dim3(64), 0, s, x, partial, nb, m,
                           c, eps, momentum, mean, invstd, running_mean, running_var, nbt);
    }
    return launch_apply<T, false>(x, (long long)m * g.nf, g.nf, mean, invstd, gamma, beta, relu, y_, TotArgs(), s);
}

template <class T>
int run_bwd(const void *x_, const void *dy_, int m, int c, const float *mean, const float *invstd,
            const float *gamma, const float *beta, int relu, void *dx_, float *dgamma, float *dbeta,
            void *ws, size_t ws_bytes, const void *add_, int add_ld, hipStream_t s) {
    typedef typename T::elem elem;
    const elem *x = (const elem *)x_, *dy = (const elem *)dy_;
    const Geo g = make_geo(c);
    if (add_ld == c) add_ld = 0;   // dense
    if (m <= BN_SMALL_ROWS) {
        bn_trace(c / 4, BN_BLOCK, "bn_small_bwd<%s>", T::name());
        hipLaunchKernelGGL((bn_small_bwd<T>), dim3(c / 4), dim3(BN_BLOCK), 0, s, x, dy, m, c, mean, invstd,
                           gamma, beta, relu, (elem *)dx_, dgamma, dbeta, (const elem *)add_, add_ld);
        return doda_check_launch();
    }
    const int nb = n_blocks_for(m, g);
    if (ws_bytes < (size_t)nb * 2 * c * 4 + (size_t)3 * c * 4) return DODA_ERR_WORKSPACE;
    float *partial = (float *)ws;
    float *coef = partial + (size_t)nb * 2 * c;
    bn_trace(nb, BN_BLOCK, "bn_bwd_partial<%s>", T::name());
    bn_trace(c, 64, "bn_bwd_final");
    hipLaunchKernelGGL((bn_bwd_partial<T>), dim3(nb), dim3(BN_BLOCK), (size_t)g.rpb * 2 * c * 4, s, x, dy,
                       m, c, g, mean, invstd, gamma, beta, relu, partial);
    hipLaunchKernelGGL(bn_bwd_final, dim3(c), dim3(64), 0, s, partial, nb, m, c, invstd,
                       gamma, dgamma, dbeta, coef);
    return launch_bwd_apply<T, false>(x, dy, (long long)m * g.nf, g.nf, c, mean, invstd, gamma, beta, relu, coef, dx_, add_, add_ld,
                                      TotArgs(), s);
}

// ---- BatchNorm(+ReLU) over statistics that a conv epilogue accumulated ------------------------------
template <class T>
int run_fwd_stats(const void *x_, int m, int c, const float *stats, int rows, float eps, float momentum,
                  const float *gamma, const float *beta, float *rm, float *rv, long long *nbt, int relu,
                  void *y_, float *mean, float *invstd, hipStream_t s) {
    typedef typename T::elem elem;
    const Geo g = make_geo(c);
    const long long n_frag = (long long)m * g.nf;
    if (fused_ok(rows, c, m)) {      // final + apply in one launch: few partial rows
        bn_trace(fused_grid(n_frag), BN_BLOCK, "bn_fused_fwd<%s>", T::name());
        hipLaunchKernelGGL((bn_fused_fwd<T>), dim3(fused_grid(n_frag)), dim3(BN_BLOCK), 0, s, (const elem *)x_, n_frag, g.nf, g.rpb,
                           stats, rows, m, eps, momentum, gamma, beta, mean, invstd, rm, rv, nbt, relu, (elem *)y_);
        return doda_check_launch();
    }
    bn_trace(c / 4, BN_BLOCK, "bn_fwd_final_stats");
    hipLaunchKernelGGL(bn_fwd_final_stats, dim3(c / 4), dim3(BN_BLOCK), 0, s, stats, rows, m, c, eps, momentum, mean,
                       invstd, rm, rv, nbt);
    return launch_apply<T, false>(x_, n_frag, g.nf, mean, invstd, gamma, beta, relu, y_, TotArgs(), s);
}

template <class T>
int run_bwd_stats(const void *x_, const void *dy_, int m, int c, const float *stats, int rows,
                  const float *mean, const float *invstd, const float *gamma, const float *beta, int relu,
                  const void *add_, int add_ld, void *dx_, float *dgamma, float *dbeta, float *coef, hipStream_t s) {
    typedef typename T::elem elem;
    const Geo g = make_geo(c);
    const long long n_frag = (long long)m * g.nf;
    if (add_ld == c || !add_) add_ld = 0;   // dense
    if (!add_ld && fused_ok(rows, c, m)) {      // final + apply in one launch: few partial rows (opt-in; dense `add` only)
        bn_trace(fused_grid(n_frag), BN_BLOCK, "bn_fused_bwd<%s>", T::name());
        hipLaunchKernelGGL((bn_fused_bwd<T>), dim3(fused_grid(n_frag)), dim3(BN_BLOCK), 0, s, (const elem *)x_, (const elem *)dy_,
                           n_frag, g.nf, g.rpb, stats, rows, m, mean, invstd, gamma, beta, relu, dgamma, dbeta, (elem *)dx_,
                           (const elem *)add_);
        return doda_check_launch();
    }
    bn_trace(c / 4, BN_BLOCK, "bn_bwd_final_stats");
    hipLaunchKernelGGL(bn_bwd_final_stats, dim3(c / 4), dim3(BN_BLOCK), 0, s, stats, rows, m, c, invstd, gamma, dgamma,
                       dbeta, coef);
    return launch_bwd_apply<T, false>(x_, dy_, n_frag, g.nf, c, mean, invstd, gamma, beta, relu, coef, dx_, add_, add_ld, TotArgs(), s);
}

// ---- argument checks of the entry points ---------------------------------------------------------------------------
// (bn_args_bad, any_null, add_bad and the two totals entry points' checks: bn_totals.hpp, shared with the op list's host plan)
// TotArgs of the forward / backward totals sweeps (backward: no running statistics; `accum` is the op list's alone, layers.hip)
TotArgs tot_fwd_args(const double *ta, const double *tb, int ca, int m, float eps, float momentum, float *rm, float *rv,
                     long long *nbt, float *save_mean, float *save_invstd) {
    TotArgs t;
    t.ta = ta; t.tb = tb; t.ca = ca; t.m = m; t.eps = eps; t.momentum = momentum;
    t.rm = rm; t.rv = rv; t.nbt = nbt;
    t.out_a = save_mean; t.out_b = save_invstd;
    return t;
}
TotArgs tot_bwd_args(const double *totals, int c, int m, float *dgamma, float *dbeta) {
    TotArgs t;
    t.ta = totals; t.ca = c; t.m = m;
    t.out_a = dgamma; t.out_b = dbeta;
    return t;
}
}  // namespace

// the value of an expression in T, with T = F32 or BF16 by the element size (which has passed bn_args_bad)
#define BN_DISPATCH(elem_bytes, ...) \
    ((elem_bytes) == 4 ? [&] { typedef F32 T; return __VA_ARGS__; }() : [&] { typedef BF16 T; return __VA_ARGS__; }())

extern "C" size_t doda_bn_workspace_bytes(int32_t m, int32_t c) {
    if (m <= 0 || c <= 0 || c % 4) return 256;
    const Geo g = make_geo(c);
    return align_up((size_t)n_blocks_for(m, g) * 2 * c * 4 + (size_t)3 * c * 4, 256);
}

extern "C" int doda_bn_relu_fwd(const void *x, int32_t m, int32_t c, int32_t elem_bytes, float eps,
                                float momentum, const float *gamma, const float *beta,
                                float *running_mean, float *running_var,
                                int64_t *num_batches_tracked, int32_t training, int32_t relu,
                                void *y, float *save_mean, float *save_invstd, void *ws,
                                size_t ws_bytes, doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, y, gamma, beta, save_mean, save_invstd, ws)) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, run_fwd<T>(x, m, c, eps, momentum, gamma, beta, running_mean, running_var, (long long *)num_batches_tracked,
                                              training, relu, y, save_mean, save_invstd, ws, ws_bytes, as_stream(stream)));
}

extern "C" int doda_bn_relu_bwd(const void *x, const void *dy, int32_t m, int32_t c,
                                int32_t elem_bytes, const float *save_mean,
                                const float *save_invstd, const float *gamma, const float *beta,
                                int32_t relu, void *dx, float *dgamma, float *dbeta, void *ws,
                                size_t ws_bytes, doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, dy, dx, gamma, beta, save_mean, save_invstd, dgamma, dbeta, ws)) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, run_bwd<T>(x, dy, m, c, save_mean, save_invstd, gamma, beta, relu, dx, dgamma, dbeta, ws, ws_bytes,
                                              nullptr, 0, as_stream(stream)));
}

// dx = BN backward + add: `add` ([m, c], dtype of x) is a second gradient of the same x — in a
// pre-activation residual block x feeds both the BatchNorm and the skip connection — so the
// gradient accumulation rides in the apply pass instead of a separate elementwise kernel.
extern "C" int doda_bn_relu_bwd_add(const void *x, const void *dy, int32_t m, int32_t c,
                                       int32_t elem_bytes, const float *save_mean,
                                       const float *save_invstd, const float *gamma, const float *beta,
                                       int32_t relu, const void *add, int32_t add_ld, void *dx, float *dgamma,
                                       float *dbeta, void *ws, size_t ws_bytes, doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, dy, dx, gamma, beta, save_mean, save_invstd, dgamma, dbeta, ws, add)) return DODA_ERR_INVALID;
    if (add_bad(add, add_ld, c, elem_bytes)) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, run_bwd<T>(x, dy, m, c, save_mean, save_invstd, gamma, beta, relu, dx, dgamma, dbeta, ws, ws_bytes,
                                              add, add_ld, as_stream(stream)));
}

extern "C" int doda_bn_relu_fwd_stats(const void *x, int32_t m, int32_t c, int32_t elem_bytes, const float *stats,
                                      int32_t stats_rows, float eps, float momentum, const float *gamma,
                                      const float *beta, float *running_mean, float *running_var,
                                      int64_t *num_batches_tracked, int32_t relu, void *y, float *save_mean,
                                      float *save_invstd, doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, y, stats, gamma, beta, save_mean, save_invstd) || stats_rows <= 0) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, run_fwd_stats<T>(x, m, c, stats, stats_rows, eps, momentum, gamma, beta, running_mean, running_var,
                                                    (long long *)num_batches_tracked, relu, y, save_mean, save_invstd, as_stream(stream)));
}

extern "C" int doda_bn_relu_apply(const void *x, int32_t m, int32_t c, int32_t elem_bytes, const float *mean,
                                  const float *invstd, const float *gamma, const float *beta, int32_t relu, void *y,
                                  doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, y, mean, invstd, gamma, beta)) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, launch_apply<T, false>(x, (long long)m * (c / 4), c / 4, mean, invstd, gamma, beta, relu, y, TotArgs(),
                                                          as_stream(stream)));
}

// ABI 6: the reduction alone — the apply pass rides in the consuming convolution's prologue (spconv_tile.hip, PRE)
extern "C" int doda_bn_fwd_final(const float *stats, int32_t stats_rows, int32_t m, int32_t c, float eps, float momentum,
                                 float *running_mean, float *running_var, int64_t *num_batches_tracked, float *save_mean,
                                 float *save_invstd, doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, 2)) return DODA_ERR_UNSUPPORTED;
    if (any_null(stats, save_mean, save_invstd) || stats_rows <= 0 || (!running_mean != !running_var)) return DODA_ERR_INVALID;
    bn_trace(c / 4, BN_BLOCK, "bn_fwd_final_stats");
    hipLaunchKernelGGL(bn_fwd_final_stats, dim3(c / 4), dim3(BN_BLOCK), 0, as_stream(stream), stats, stats_rows, m, c, eps,
                       momentum, save_mean, save_invstd, running_mean, running_var, (long long *)num_batches_tracked);
    return doda_check_launch();
}

// ABI 9: BatchNorm(+ReLU) over TOTALS that conv epilogues accumulated (doda_conv_epilogue.stats_totals): ONE launch.
// totals_b / c_a: the columns [c_a, c) come from a second producer (a channel concatenation); totals_b null: c_a is ignored.
extern "C" int doda_bn_relu_fwd_totals(const void *x, int32_t m, int32_t c, int32_t elem_bytes, const double *totals,
                                       const double *totals_b, int32_t c_a, float eps, float momentum, const float *gamma,
                                       const float *beta, float *running_mean, float *running_var,
                                       int64_t *num_batches_tracked, int32_t relu, void *y, float *save_mean,
                                       float *save_invstd, doda_stream_t stream) {
    const int st = bn_fwd_totals_status(x, m, c, elem_bytes, totals, totals_b, c_a, gamma, beta, running_mean, running_var, y, save_mean, save_invstd);
    if (st != DODA_OK || m == 0) return st;
    const TotArgs t = tot_fwd_args(totals, totals_b, totals_b ? c_a : c, m, eps, momentum, running_mean, running_var,
                                   (long long *)num_batches_tracked, save_mean, save_invstd);
    return BN_DISPATCH(elem_bytes, launch_apply<T, true>(x, (long long)m * (c / 4), c / 4, nullptr, nullptr, gamma, beta, relu, y, t,
                                                         as_stream(stream)));
}

// (the two entry points over a data-grad epilogue's statistics test `add` before m == 0)
extern "C" int doda_bn_relu_bwd_totals(const void *x, const void *dy, int32_t m, int32_t c, int32_t elem_bytes,
                                       const double *totals, const float *save_mean, const float *save_invstd,
                                       const float *gamma, const float *beta, int32_t relu, const void *add, int32_t add_ld,
                                       void *dx, float *dgamma, float *dbeta, doda_stream_t stream) {
    const int st = bn_bwd_totals_status(x, dy, m, c, elem_bytes, totals, save_mean, save_invstd, gamma, beta, add, add_ld, dx, dgamma, dbeta);
    if (st != DODA_OK || m == 0) return st;
    if (add_ld == c || !add) add_ld = 0;   // dense
    return BN_DISPATCH(elem_bytes, launch_bwd_apply<T, true>(x, dy, (long long)m * (c / 4), c / 4, c, save_mean, save_invstd, gamma, beta,
                                                             relu, nullptr, dx, add, add_ld, tot_bwd_args(totals, c, m, dgamma, dbeta),
                                                             as_stream(stream)));
}

extern "C" int doda_bn_relu_bwd_stats(const void *x, const void *dy, int32_t m, int32_t c, int32_t elem_bytes,
                                         const float *stats, int32_t stats_rows, const float *save_mean,
                                         const float *save_invstd, const float *gamma, const float *beta, int32_t relu,
                                         const void *add, int32_t add_ld, void *dx, float *dgamma, float *dbeta,
                                         float *coef_ws, doda_stream_t stream) {
    if (add && add_bad(add, add_ld, c, elem_bytes)) return DODA_ERR_INVALID;
    if (m == 0) return DODA_OK;
    if (bn_args_bad(m, c, elem_bytes)) return DODA_ERR_UNSUPPORTED;
    if (any_null(x, dy, dx, stats, gamma, beta, save_mean, save_invstd, dgamma, dbeta, coef_ws) || stats_rows <= 0) return DODA_ERR_INVALID;
    return BN_DISPATCH(elem_bytes, run_bwd_stats<T>(x, dy, m, c, stats, stats_rows, save_mean, save_invstd, gamma, beta, relu, add, add_ld,
                                                    dx, dgamma, dbeta, coef_ws, as_stream(stream)));
}

// Per-layer backend of the U-Net op list (ABI 11: doda_layers_run; ABI 12: every level — GEMM ops carry their table's tilebook).
//
// The deep levels of DODA's U-Net (reference model/unet_block.py:55-100 UBlock: blocks -> strided conv -> UBlock -> inverse conv ->
// concatenation -> blocks_tail, ResidualBlocks of model/unet_block.py:9-37 inside) are described by the caller as a list of
// doda_cx_op (include/doda_hip.h).  Every op is a WHOLE-CHIP launch of the kernels the module-by-module path uses anyway (doda_spconv_gather_ex, the BatchNorm sweeps over fp64 totals), issued back to back
// from C++ with nothing in between — and a BatchNorm whose consumer is the next convolution of the list is folded into that
// convolution's gather (doda_conv_prologue):
//     BNFWD ; GEMM(x = its output)                 -> one launch   (forward:  BatchNorm1d -> ReLU -> conv)
//     BNBWD ; GEMM(x = its output)                 -> one launch   (backward: the BatchNorm's input gradient feeds the previous conv's
//                                                                   data gradient; the skip gradient rides along as `add`)
// wherever the BatchNorm's rows are few enough for its own sweep to be a launch-floor kernel (DODA_PRE_FWD_ROWS, default 16384 /
// DODA_PRE_BWD_ROWS, default 0 = the backward BatchNorm keeps its own 3.3 us launch: measured, see switches_from_env below).
// The folded and the unfolded form of an op give the same bits (bn_totals.hpp), so the fusion is a schedule, not a numerics change.
// (Round 5 walked the same list inside ONE persistent launch on one XCD: 1/8 of the chip's matrix rate and loads in flight lost to
// the whole-chip kernels at the bench size and, once those were issued from here, at the host floor too — removed in ABI 11.)
#include "common.hpp"
#include "spconv_common.hpp"
#include "layers_plan.hpp"
#include <stdlib.h>
#include <string.h>
#include <new>
#include <type_traits>

namespace {

// ---- standalone BatchNorm ops in the general (strided, split-output) form -------------------------------------------------
// y[:, 0:c_split) -> y, y[:, c_split:c) -> y2: the two halves of a concatenation's gradient as two dense tensors.
template <int ESZ, int KIND>
__global__ __launch_bounds__(256) void lay_bn(const void *__restrict__ x_, unsigned x_ld, int c, const PreArgs pre, void *__restrict__ y_,
                                              unsigned y_ld, void *__restrict__ y2_, unsigned y2_ld, int c_split) {
    typedef typename std::conditional<ESZ == 2, unsigned short, float>::type elem;
    __shared__ __attribute__((aligned(16))) float co[PreForm<ESZ, KIND>::NVEC][PRE_MAX_C];
    const PreRaw raw = pre_request<KIND>(pre, c);
    pre_finish<ESZ, KIND>(pre, c, raw, co);
    doda_sync();
    // a thread keeps ONE 16-byte column piece for the whole sweep (the block uses the largest multiple of the pieces per row among
    // its 256 threads): the per-channel coefficients are read from LDS once, no division per piece, four rows in flight per thread
    constexpr int NV = 16 / ESZ, U = 4;
    const int ppr = c / NV, rpb = 256 / ppr;
    const int tr = (int)threadIdx.x / ppr, c0 = ((int)threadIdx.x - tr * ppr) * NV;
    if (tr >= rpb) return;
    PreCo<ESZ, KIND> cv;
    pre_load_co<ESZ, KIND>(co, c0, cv);
    const elem *x = (const elem *)x_;
    const bool left = c0 < c_split;
    elem *const yo = left ? (elem *)y_ + c0 : (elem *)y2_ + (c0 - c_split);
    const size_t yl = left ? y_ld : y2_ld;
    const long long rows = pre.rows, step = (long long)gridDim.x * rpb;
    for (long long r0 = (long long)blockIdx.x * rpb + tr; r0 < rows; r0 += step * U) {
        u32x4 xv[U], uv[U], av[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const long long r = r0 + k * step < rows ? r0 + k * step : r0;   // (past the end: the first row again, not stored)
            xv[k] = *reinterpret_cast<const u32x4 *>(x + r * x_ld + c0);
            uv[k] = av[k] = xv[k];
            if constexpr (KIND >= 2) uv[k] = *reinterpret_cast<const u32x4 *>((const elem *)pre.aux + r * pre.aux_ld + c0);
            if constexpr (KIND >= 3) av[k] = *reinterpret_cast<const u32x4 *>((const elem *)pre.add + r * pre.add_ld + c0);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const long long r = r0 + k * step;
            const u32x4 o = pre_piece<ESZ, KIND>(xv[k], uv[k], av[k], cv, pre.relu, ~0u);
            if (r < rows) *reinterpret_cast<u32x4 *>(yo + r * yl) = o;
        }
    }
}

// (sum x, sum x^2) of a [rows, c] matrix into fp64 totals (layout: spconv_common.hpp stats_emit).  One thread per (row lane,
// 4-channel group); fp32 partial sums over at most a few hundred rows per thread, fp64 atomics per workgroup.
template <int ESZ>
__global__ __launch_bounds__(256) void lay_stats(const void *__restrict__ x_, unsigned x_ld, int rows, int c, double *__restrict__ tot) {
    typedef typename std::conditional<ESZ == 2, unsigned short, float>::type elem;
    const elem *x = (const elem *)x_;
    const int nf = c / 4, rpb = 256 / nf > 0 ? 256 / nf : 1;
    const int f = threadIdx.x % nf, rl = threadIdx.x / nf;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    __shared__ float red[2][256][4];
    if (rl < rpb && f < nf) {
        for (long long r = (long long)blockIdx.x * rpb + rl; r < rows; r += (long long)gridDim.x * rpb) {
            f32x4 v;
            if constexpr (ESZ == 2) {
                const u32x2 p = *reinterpret_cast<const u32x2 *>(x + r * x_ld + f * 4);
                v = (f32x4){__uint_as_float(p[0] << 16), __uint_as_float(p[0] & 0xffff0000u), __uint_as_float(p[1] << 16),
                            __uint_as_float(p[1] & 0xffff0000u)};
            } else {
                v = *reinterpret_cast<const f32x4 *>(x + r * x_ld + f * 4);
            }
            s1 += v;
            s2 += v * v;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[0][threadIdx.x][q] = s1[q]; red[1][threadIdx.x][q] = s2[q]; }
    doda_sync();
    if (rl == 0 && f < nf) {
        for (int k = 1; k < rpb; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) { s1[q] += red[0][k * nf + f][q]; s2[q] += red[1][k * nf + f][q]; }
        const size_t slot = (size_t)(blockIdx.x & (DODA_STATS_SLOTS - 1));
        double *t1 = tot + ((slot * 2 + 0) * (size_t)nf + (size_t)f) * 16, *t2 = tot + ((slot * 2 + 1) * (size_t)nf + (size_t)f) * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) { unsafeAtomicAdd(t1 + q, (double)s1[q]); unsafeAtomicAdd(t2 + q, (double)s2[q]); }
    }
}

static_assert(LAY_MAX_C == PRE_MAX_C && LAY_MAX_C == BN_TOT_MAX_C && LAY_FOLD_MIN_C_BF16 == 32 && LAY_BLOCK == 256,
              "layers_plan.hpp restates these constants (the wide packing starts at 32 channels: gather_plan.hpp pack_mode)");

// PreArgs of a BatchNorm op the plan has accepted (BNFWD: kind 1; BNBWD: kind 2 / 3)
PreArgs pre_of(const doda_cx_op &o) {
    PreArgs p{};
    p.relu = (o.flags & DODA_CX_F_RELU) ? 1 : 0;
    p.rows = o.rows;
    p.tot.ta = (const double *)o.stats; p.tot.ca = o.c_in; p.tot.m = o.rows;
    p.gamma = o.gamma; p.beta = o.beta; p.mean = o.mean; p.invstd = o.invstd;
    p.side = o.y; p.side_ld = (unsigned)o.y_ld;
    if (o.kind == DODA_CX_BNFWD) {
        p.kind = 1;
        if (o.flags & DODA_CX_F_TRAINING) {
            const int split = lay_split(o);
            p.tot.tb = split < o.c_in ? (const double *)o.stats_b : nullptr;
            p.tot.ca = split;
            p.tot.nbt = (long long *)o.nbt;
            p.tot.out_a = o.mean; p.tot.out_b = o.invstd;
        } else p.tot.ta = nullptr;
        p.tot.rm = o.running_mean; p.tot.rv = o.running_var;
        p.tot.eps = o.eps; p.tot.momentum = o.momentum;
    } else {
        p.kind = o.res ? 3 : 2;
        p.tot.out_a = o.dgamma; p.tot.out_b = o.dbeta; p.tot.accum = (o.flags & DODA_CX_F_ACCUM) ? 1 : 0;
        p.aux = o.aux; p.aux_ld = (unsigned)o.aux_ld;
        p.add = o.res; p.add_ld = (unsigned)o.res_ld;
    }
    return p;
}

template <int ESZ>
int launch_bn(const doda_cx_op &o, const LayerStep &st, hipStream_t s) {
    const PreArgs p = pre_of(o);
    const int split = o.kind == DODA_CX_BNBWD ? lay_split(o) : o.c_in;
    bn_trace(st.grid, st.block, "lay_bn<%d, %d>", ESZ, (int)st.kind);
    const auto go = [&](auto kind) {
        hipLaunchKernelGGL((lay_bn<ESZ, decltype(kind)::value>), dim3(st.grid), dim3(st.block), 0, s, o.x, (unsigned)o.x_ld, o.c_in, p, o.y,
                           (unsigned)o.y_ld, o.y2, (unsigned)o.y2_ld, split);
    };
    if (st.kind == 1) go(std::integral_constant<int, 1>{});
    else if (st.kind == 2) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 3>{});
    return doda_check_launch();
}

// dense BatchNorm ops of many rows: the register-resident sweeps of bn.hip (the plan has asked their argument checks)
int launch_bn_totals(const doda_cx_op &o, int esz, hipStream_t s) {
    const int relu = (o.flags & DODA_CX_F_RELU) ? 1 : 0, split = lay_split(o);
    if (o.kind == DODA_CX_BNFWD)
        return doda_bn_relu_fwd_totals(o.x, o.rows, o.c_in, esz, (const double *)o.stats, split < o.c_in ? (const double *)o.stats_b : nullptr,
                                       split, o.eps, o.momentum, o.gamma, o.beta, o.running_mean, o.running_var, o.nbt, relu, o.y, o.mean,
                                       o.invstd, (doda_stream_t)s);
    return doda_bn_relu_bwd_totals(o.aux, o.x, o.rows, o.c_in, esz, (const double *)o.stats, o.mean, o.invstd, o.gamma, o.beta, relu, o.res,
                                   o.res ? o.res_ld : 0, o.y, o.dgamma, o.dbeta, (doda_stream_t)s);
}

int launch_stats(const doda_cx_op &o, int esz, const LayerStep &st, hipStream_t s) {
    bn_trace(st.grid, st.block, "lay_stats<%d>", esz);
    if (esz == 2) hipLaunchKernelGGL((lay_stats<2>), dim3(st.grid), dim3(st.block), 0, s, o.x, (unsigned)o.x_ld, o.rows, o.c_in, (double *)o.stats);
    else hipLaunchKernelGGL((lay_stats<4>), dim3(st.grid), dim3(st.block), 0, s, o.x, (unsigned)o.x_ld, o.rows, o.c_in, (double *)o.stats);
    return doda_check_launch();
}

// the convolution of the list on the route the plan holds, optionally with a BatchNorm op folded into its gather
int launch_gemm(const doda_cx_op &o, const doda_cx_op *bn, const LayerStep &st, hipStream_t s) {
    if (st.call.n_out == 0) return DODA_OK;   // (a fold in front of a convolution of no output rows)
    doda_conv_epilogue ep;
    doda_conv_prologue q;
    int32_t stats_rows = 0;
    const void *x;
    gemm_call(o, bn, &ep, &q, &stats_rows, &x);
    return doda_gather::launch(st.call, st.gather, x, (const float *)o.w, o.tbl, o.y, nullptr, &ep, s);
}

// Defaults from measurements on MI355X (tools/prebench_prof.sh, tools/layers_ab.py): at 1900 rows x 80 channels a standalone
// totals sweep (lay_bn) is a 3.3 us kernel + ~2 us boundary; folding costs the conv +5.3 us forward (break-even on the GPU, one launch
// less on the host: 4.88 -> 4.81 ms per bench step) and +8.3 us backward (two gathered operands, ~60 vector instructions per piece:
// 4.81 -> 4.89 ms) — so the forward folds, the backward does not (DODA_PRE_BWD_ROWS=4096 to fold it on a host-bound box).
LayerSwitches switches_from_env() {
    LayerSwitches sw;
    sw.pre_fwd_rows = env_ll("DODA_PRE_FWD_ROWS", LAY_PRE_FWD_ROWS);
    sw.pre_bwd_rows = env_ll("DODA_PRE_BWD_ROWS", LAY_PRE_BWD_ROWS);
    sw.lay_bn_grid = env_ll("DODA_LAY_BN_GRID", LAY_BN_GRID);
    sw.tuned_rows_bf16 = env_ll("DODA_LAY_TUNED_ROWS", LAY_TUNED_ROWS_BF16);
    return sw;
}
// (the environment once, at the first list or option call: as gather_switches, spconv_gather.hip)
LayerSwitches &layer_switches() {
    static LayerSwitches sw = switches_from_env();
    return sw;
}

}  // namespace

namespace doda_layers {
long long fwd_rows() { return layer_switches().pre_fwd_rows; }
long long bwd_rows() { return layer_switches().pre_bwd_rows; }
void set_fwd_rows(long long v) { layer_switches().pre_fwd_rows = v < 0 ? 0 : v; }
void set_bwd_rows(long long v) { layer_switches().pre_bwd_rows = v < 0 ? 0 : v; }
}  // namespace doda_layers

// plan the whole list (layers_plan.hpp), then launch its steps: an error return has enqueued nothing but for a failed launch
extern "C" int doda_layers_run(const doda_cx_op *ops_h, int32_t n_ops, int32_t elem_bytes, int32_t *n_launches_h, doda_stream_t stream) {
    if (n_launches_h) *n_launches_h = 0;
    thread_local std::vector<LayerStep> steps;   // (keeps its capacity: no allocation per call in the steady state)
    int st = DODA_ERR_NOMEM;
    try { st = plan_layers(ops_h, n_ops, elem_bytes, layer_switches(), doda_gather::switches(), steps); } catch (const std::bad_alloc &) {}
    if (st != DODA_OK) return st;
    hipStream_t s = as_stream(stream);
    for (const LayerStep &step : steps) {
        const doda_cx_op &o = ops_h[step.first];
        switch (step.route) {
        case LR_GEMM: st = launch_gemm(o, nullptr, step, s); break;
        case LR_GEMM_FOLD: st = launch_gemm(ops_h[step.first + 1], &o, step, s); break;
        case LR_LAY_BN: st = elem_bytes == 2 ? launch_bn<2>(o, step, s) : launch_bn<4>(o, step, s); break;
        case LR_BN_TOTALS: st = launch_bn_totals(o, elem_bytes, s); break;
        case LR_LAY_STATS: st = launch_stats(o, elem_bytes, step, s); break;
        }
        if (st != DODA_OK) return st;
    }
    if (n_launches_h) *n_launches_h = (int32_t)steps.size();
    return DODA_OK;
}

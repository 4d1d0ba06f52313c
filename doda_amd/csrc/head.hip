// Point head + loss without the point-level score matrix (ABI 11: doda_head_ce_fwd / _bwd); the self-training confidence
// (doda_st_voxel_confidence, include/doda_selftrain.h) shares its logit code.
//
// reference model/unet.py:62-64,107-108,196: feats_pt = out.features[p2v]; scores = Linear(feats_pt); loss =
// CrossEntropyLoss(ignore_index)(scores, labels) — a [N points, n_cls] fp32 matrix (62 MB at 781 k points x 20 classes) that the
// per-layer path writes and re-reads five times (gather-GEMM, loss forward, loss backward, cast + column sums, the two
// gradient GEMMs: ~210 us of a 4.8 ms step).  Every point of a voxel reads the SAME feature row, so its logits are its voxel's:
// with z_v = W f_v + b,  lse_v = log sum exp z_v  and the voxel's point list (v2p_map, reference lib/pointgroup_ops voxelize_idx)
//     loss   = (1 / n_valid) sum_v [ cnt_v lse_v - sum_{p in v, valid} z_v[y_p] ]
//     dz_v   = (g / n_valid) [ cnt_v softmax(z_v) - hist_v ]          (hist_v[k] = valid points of v labelled k)
//     df_v   = W^T dz_v,   dW = sum_v dz_v f_v^T,   db = sum_v dz_v
// i.e. two sweeps over the VOXEL rows (19 MB of features + the point lists + the labels): one thread per voxel, the weights
// in LDS, logits recomputed instead of stored.  dz_v is written once at voxel level (the operand of the library's weight-gradient
// kernel over an identity table); db as per-workgroup rows the caller adds (fixed order: deterministic).  The per-voxel argmax
// (the training meters' prediction, reference tool/train.py accuracy) rides in the forward sweep.
// bf16 features: the weights are rounded to bf16 first, as the gather-GEMM's pre-pack does; accumulation in fp32.
#include "common.hpp"
#include "spconv_common.hpp"
#include "head_common.hpp"
#include "../../include/doda_selftrain.h"

namespace {

// forward: per-workgroup (loss sum, valid count) partials; pred[v] = argmax_k z_v[k]
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(HD_BLOCK, 4) void head_ce_fwd(const void *__restrict__ feats, int m, const float *__restrict__ weight,
                                                        const float *__restrict__ bias, int n_cls, const int32_t *__restrict__ v2p,
                                                        int v2p_ld, const long long *__restrict__ labels, long long ignore_index,
                                                        float *__restrict__ partial, int32_t *__restrict__ pred) {
    __shared__ float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    __shared__ float red[2][HD_BLOCK / 64];
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);
    float loss = 0.f, cnt = 0.f;
#pragma unroll 1
    for (long long v = (long long)blockIdx.x * HD_BLOCK + threadIdx.x; v < m; v += (long long)gridDim.x * HD_BLOCK) {
        asm volatile("" ::: "memory");      // (the 320 staged weights stay in LDS: hoisted out of this loop they cost 256 VGPRs + spills)
        float f[C], z[NK], mx;
        int arg;
        hd_load_row<ESZ, C>(feats, v, f);
        const int32_t *row = v2p + v * v2p_ld;
        const int np = row[0];
        hd_logits<C, NK>(w, b, n_cls, f, z, mx, arg);
        if (pred) pred[v] = arg;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) s += __expf(z[k] - mx);
        const float lse = mx + __logf(s);
#pragma unroll 1
        for (int i = 0; i < np; ++i) {
            const long long lab = labels[row[1 + i]];
            if (lab != ignore_index && lab >= 0 && lab < n_cls) {
                float zy = 0.f;
#pragma unroll
                for (int k = 0; k < NK; ++k) zy = (int)lab == k ? z[k] : zy;
                loss += lse - zy;
                cnt += 1.f;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { loss += __shfl_xor(loss, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = loss; red[1][threadIdx.x >> 6] = cnt; }
    doda_sync();
    if (threadIdx.x == 0) {
        float a = 0.f, c2 = 0.f;
        for (int q = 0; q < HD_BLOCK / 64; ++q) { a += red[0][q]; c2 += red[1][q]; }
        partial[2 * blockIdx.x] = a;
        partial[2 * blockIdx.x + 1] = c2;
    }
}

// self-training confidence (include/doda_selftrain.h): pred[v] = argmax_k z_v[k] through the same hd_logits as head_ce_fwd (same
// bits), conf[v] = 1 / sum_k exp(z_v[k] - max) — the largest softmax probability — with the accurate expf (no point-level matrix)
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(HD_BLOCK, 4) void st_voxel_conf(const void *__restrict__ feats, int m, const float *__restrict__ weight,
                                                          const float *__restrict__ bias, int n_cls, int32_t *__restrict__ pred,
                                                          float *__restrict__ conf) {
    __shared__ float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);
#pragma unroll 1
    for (long long v = (long long)blockIdx.x * HD_BLOCK + threadIdx.x; v < m; v += (long long)gridDim.x * HD_BLOCK) {
        asm volatile("" ::: "memory");
        float f[C], z[NK], mx;
        int arg;
        hd_load_row<ESZ, C>(feats, v, f);
        hd_logits<C, NK>(w, b, n_cls, f, z, mx, arg);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) s += expf(z[k] - mx);      // (padding classes: exp(-inf) = 0; the argmax term: exactly 1)
        pred[v] = arg;
        conf[v] = 1.f / s;
    }
}

// out[0] = sum(loss) / max(n_valid, 1), out[1] = n_valid (fixed order, fp64).  1024 threads: two or three partial rows each — one
// round trip instead of the 37 dependent ones a single wave needed over 2349 rows (11 us)
__global__ __launch_bounds__(1024) void head_ce_final(const float *__restrict__ partial, int nblocks, float *__restrict__ out) {
    __shared__ double red[2][16];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 1024) { a += (double)partial[2 * k]; b += (double)partial[2 * k + 1]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    doda_sync();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int q = 0; q < 16; ++q) { a += red[0][q]; b += red[1][q]; }
        out[0] = (float)(a / (b > 1.0 ? b : 1.0));
        out[1] = (float)b;
    }
}

// backward: d_feats [m, C], dz [m, n_cls] (storage type of the features), db partial rows [blocks][n_cls].
// The per-class values of a thread's voxel (exp(z - max), then dz) live in its LDS column (head_common.hpp): a point's label indexes
// its class directly (dz[label] -= scale).
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(HD_BLOCK) void head_ce_bwd(const void *__restrict__ feats, int m, const float *__restrict__ weight,
                                                        const float *__restrict__ bias, int n_cls, const int32_t *__restrict__ v2p,
                                                        int v2p_ld, const long long *__restrict__ labels, long long ignore_index,
                                                        const float *__restrict__ out, const float *__restrict__ grad,
                                                        void *__restrict__ d_feats, void *__restrict__ dz_out, float *__restrict__ db_partial) {
    __shared__ __attribute__((aligned(16))) float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    __shared__ float sz[NK][HD_BLOCK];
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);
    const float nv = out[1] > 1.f ? out[1] : 1.f;
    const float scale = grad[0] / nv;
    const int tid = threadIdx.x;
    const long long v = (long long)blockIdx.x * HD_BLOCK + tid;
#pragma unroll 1
    for (int k = 0; k < NK; ++k) sz[k][tid] = 0.f;      // (a thread past the last voxel contributes zeros to hd_db_colsums)
    if (v < m) {
        float f[C];
        hd_load_row<ESZ, C>(feats, v, f);
        const int32_t *row = v2p + v * v2p_ld;
        const int np = row[0];
        const float mx = hd_logits_lds<C>(w, b, n_cls, f, sz, tid);
        float s = 0.f;
#pragma unroll 2
        for (int k = 0; k < n_cls; ++k) {
            const float e = __expf(sz[k][tid] - mx);
            sz[k][tid] = e;
            s += e;
        }
        // valid points: their count now, their classes after the softmax term
        float cntv = 0.f;
#pragma unroll 1
        for (int i = 0; i < np; ++i) {
            const long long lab = labels[row[1 + i]];
            cntv += (lab != ignore_index && lab >= 0 && lab < n_cls) ? 1.f : 0.f;
        }
        const float a = cntv * scale / s;        // dz_k = a exp(z_k - mx) - scale hist_k
#pragma unroll 2
        for (int k = 0; k < n_cls; ++k) sz[k][tid] *= a;
#pragma unroll 1
        for (int i = 0; i < np; ++i) {
            const long long lab = labels[row[1 + i]];
            if (lab != ignore_index && lab >= 0 && lab < n_cls) sz[(int)lab][tid] -= scale;
        }
        float df[C];
#pragma unroll
        for (int c = 0; c < C; ++c) df[c] = 0.f;
        char *dzr = (char *)dz_out + (size_t)v * n_cls * ESZ;
#pragma unroll 1
        for (int k = 0; k < n_cls; k += 2) {      // two classes per step: one 4- / 8-byte store of dz (even n_cls)
            const float g0 = sz[k][tid], g1 = k + 1 < n_cls ? sz[k + 1][tid] : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) df[c] = __builtin_fmaf(g0, w[k][c], df[c]);
            if (k + 1 < n_cls) {
#pragma unroll
                for (int c = 0; c < C; ++c) df[c] = __builtin_fmaf(g1, w[k + 1][c], df[c]);
                if (n_cls & 1) {      // (odd rows start at odd elements: a paired store would be misaligned)
                    HdRow<ESZ>::store(dzr + (size_t)k * ESZ, g0);
                    HdRow<ESZ>::store(dzr + (size_t)(k + 1) * ESZ, g1);
                } else if constexpr (ESZ == 2)
                    *reinterpret_cast<unsigned *>(dzr + (size_t)k * 2) = (unsigned)f2bf(g0) | ((unsigned)f2bf(g1) << 16);
                else
                    *reinterpret_cast<f32x2 *>(dzr + (size_t)k * 4) = (f32x2){g0, g1};
            } else HdRow<ESZ>::store(dzr + (size_t)k * ESZ, g0);
        }
        hd_store_dfeats<ESZ, C>(d_feats, v, df);
    }
    hd_db_colsums(sz, n_cls, db_partial);
}

// dW of the head from the voxel-level score gradient, bf16: partial[wg][32 classes][16 channels] = sum over the workgroup's voxels of
// dz_v[k] f_v[c].  Voxels are the MFMA's k dimension: a wave parks 64 voxels' dz / feature rows in LDS class- / channel-major
// (lane = voxel writes a column), so that lane (row i, group g) of v_mfma_f32_16x16x32_bf16 reads its eight consecutive voxels of
// class / channel i with one 16-byte read; 4 MFMAs per 64 voxels, accumulators across the wave's chunks, the four waves summed in
// order.  Replaces the gather-table weight-gradient kernel over an identity table (50 us for this shape: 20 is not a multiple of
// its 16-channel blocks).
__global__ __launch_bounds__(HD_BLOCK) void head_dw_bf16(const unsigned short *__restrict__ feats, const unsigned short *__restrict__ dz,
                                                         int m, int n_cls, float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) unsigned short sdz[4][32][64 + 8], sf[4][16][64 + 8];   // (+8: rows 144 bytes apart, 16-byte aligned)
    __shared__ f32x4 red[3][2][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int k = n_cls; k < 32; ++k) sdz[wid][k][lane] = 0;                  // padding classes: zero rows, written once
    const long long n_chunks = ((long long)m + 63) / 64;
    for (long long ch = (long long)blockIdx.x * 4 + wid; ch < n_chunks; ch += (long long)gridDim.x * 4) {
        const long long v = ch * 64 + lane;
        if (v < m) {
            const u32x4 f0 = *reinterpret_cast<const u32x4 *>(feats + v * 16), f1 = *reinterpret_cast<const u32x4 *>(feats + v * 16 + 8);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sf[wid][2 * q][lane] = (unsigned short)(f0[q] & 0xffffu); sf[wid][2 * q + 1][lane] = (unsigned short)(f0[q] >> 16);
                sf[wid][8 + 2 * q][lane] = (unsigned short)(f1[q] & 0xffffu); sf[wid][9 + 2 * q][lane] = (unsigned short)(f1[q] >> 16);
            }
            const unsigned short *r = dz + v * n_cls;
            for (int k = 0; k + 1 < n_cls; k += 2) {      // (rows of n_cls bf16: 4-byte aligned when n_cls is even; odd: element by element)
                if ((n_cls & 1) == 0) {
                    const unsigned p = *reinterpret_cast<const unsigned *>(r + k);
                    sdz[wid][k][lane] = (unsigned short)(p & 0xffffu); sdz[wid][k + 1][lane] = (unsigned short)(p >> 16);
                } else { sdz[wid][k][lane] = r[k]; sdz[wid][k + 1][lane] = r[k + 1]; }
            }
            if (n_cls & 1) sdz[wid][n_cls - 1][lane] = r[n_cls - 1];
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) sf[wid][c][lane] = 0;
            for (int k = 0; k < n_cls; ++k) sdz[wid][k][lane] = 0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (wave-private LDS: its own writes are visible to its own reads after the wait)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const u32x4 bv = *reinterpret_cast<const u32x4 *>(&sf[wid][i][32 * st + 8 * g]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const u32x4 av = *reinterpret_cast<const u32x4 *>(&sdz[wid][16 * t + i][32 * st + 8 * g]);
                mma_bf16_k32(acc[t], av, bv);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // D[row = class 16 t + 4 g + r][col = channel i]; the four waves in order
    if (wid > 0) { red[wid - 1][0][lane] = acc[0]; red[wid - 1][1][lane] = acc[1]; }
    doda_sync();
    if (wid == 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x4 a = acc[t];
#pragma unroll
            for (int q = 0; q < 3; ++q) a += red[q][t][lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) partial[(size_t)blockIdx.x * 512 + (size_t)(16 * t + 4 * g + r) * 16 + i] = a[r];
        }
    }
}

}  // namespace

extern "C" int32_t doda_head_ce_blocks(int32_t m) { return hd_blocks(m > 0 ? m : 1); }

extern "C" int doda_head_ce_fwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                                int32_t n_cls, const int32_t *v2p, int32_t v2p_ld, const int64_t *labels, int64_t ignore_index,
                                float *out, int32_t *pred, float *partial_ws, int32_t n_blocks, doda_stream_t stream) {
    if (!out) return DODA_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (m == 0) { (void)hipMemsetAsync(out, 0, 8, s); return DODA_OK; }
    if (hd_args_bad(m, elem_bytes, v2p_ld, {feats, weight, v2p, labels, partial_ws}) || n_cls <= 0) return DODA_ERR_INVALID;
    if (c != 16 || n_cls > 32) return DODA_ERR_UNSUPPORTED;     // (DODA's head: 16 channels, <= 20 classes; others take the matrix path)
    if (n_blocks != hd_blocks(m)) return DODA_ERR_WORKSPACE;
    HD_DISPATCH(head_ce_fwd, 16, n_blocks, feats, m, weight, bias, n_cls, v2p, v2p_ld, (const long long *)labels, (long long)ignore_index,
                partial_ws, pred);
    hipLaunchKernelGGL(head_ce_final, dim3(1), dim3(1024), 0, s, (const float *)partial_ws, n_blocks, out);
    return doda_check_launch();
}

extern "C" int doda_head_ce_bwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                                int32_t n_cls, const int32_t *v2p, int32_t v2p_ld, const int64_t *labels, int64_t ignore_index,
                                const float *out, const float *grad, void *d_feats, void *dz, float *db_partial, int32_t n_blocks,
                                doda_stream_t stream) {
    if (m == 0) return DODA_OK;
    if (hd_args_bad(m, elem_bytes, v2p_ld, {feats, weight, v2p, labels, out, grad, d_feats, dz, db_partial}) || n_cls <= 0)
        return DODA_ERR_INVALID;
    if (c != 16 || n_cls > 32) return DODA_ERR_UNSUPPORTED;
    if (n_blocks != hd_blocks(m)) return DODA_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    HD_DISPATCH(head_ce_bwd, 16, n_blocks, feats, m, weight, bias, n_cls, v2p, v2p_ld, (const long long *)labels, (long long)ignore_index,
                out, grad, d_feats, dz, db_partial);
    return doda_check_launch();
}

extern "C" int doda_st_voxel_confidence(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight,
                                        const float *bias, int32_t n_cls, int32_t *pred, float *conf, doda_stream_t stream) {
    if (hd_args_bad(m, elem_bytes, 1, {weight, pred, conf}) || (m > 0 && !feats)) return DODA_ERR_INVALID;
    if ((c != 16 && c != 32) || n_cls < 2 || n_cls > DODA_ST_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    if (m == 0) return DODA_OK;
    hipStream_t s = as_stream(stream);
    // (32 channels, the reference configs' `mid_channel: 16 # or 32`: this entry point only)
    if (c == 16) HD_DISPATCH(st_voxel_conf, 16, hd_blocks(m), feats, m, weight, bias, n_cls, pred, conf);
    else HD_DISPATCH(st_voxel_conf, 32, hd_blocks(m), feats, m, weight, bias, n_cls, pred, conf);
    return doda_check_launch();
}

extern "C" int32_t doda_head_dw_blocks(int32_t m) {
    int nb = div_up(div_up(m > 0 ? m : 1, 64), 4);
    if (nb > 1024) nb = 1024;
    return nb < 1 ? 1 : nb;
}

extern "C" int doda_head_dw_bf16(const void *feats, const void *dz, int32_t m, int32_t c, int32_t n_cls, float *partial, int32_t n_blocks,
                                 doda_stream_t stream) {
    if (m < 0 || !partial) return DODA_ERR_INVALID;
    if (c != 16 || n_cls < 1 || n_cls > 32) return DODA_ERR_UNSUPPORTED;
    if (n_blocks != doda_head_dw_blocks(m)) return DODA_ERR_WORKSPACE;
    if (m > 0 && (!feats || !dz || ((uintptr_t)feats & 15) || ((uintptr_t)dz & 3))) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(head_dw_bf16, dim3(n_blocks), dim3(HD_BLOCK), 0, as_stream(stream), (const unsigned short *)feats,
                       (const unsigned short *)dz, m, n_cls, partial);
    return doda_check_launch();
}

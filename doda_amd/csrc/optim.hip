// Optimizer step over every parameter of a network in ONE launch (SGD: doda_sgd_multi; SGD / Adam / AdamW with an optional
// gradient-norm clip, one launch more: doda_optim_step, include/doda_optim.h — second half of this file).
//
// The reference trains with torch.optim.SGD (util/common_utils.py:196-215, tool/train.py:235-268); the
// U-Net has 281 parameter tensors, most of them BatchNorm vectors of 16..224 floats.  torch's fused
// multi-tensor path packs at most ~110 tensor addresses into one kernel-argument block, so the step is
// five launches of ~30-50 us each; here the per-tensor descriptors live in device memory (uploaded with the
// launch: the gradient tensors are new allocations every step) and one grid covers all tensors.
// The arithmetic is torch's FusedSgdMathFunctor term by term (hyper-parameters are doubles there, so the
// mixed products round once, from double): bit-identical parameters and momentum buffers.
#include "common.hpp"
#include "../../include/doda_optim.h"

#include <mutex>
#include <string.h>

namespace {

constexpr int SGD_BLOCK = 256;
constexpr int SGD_PER_THREAD = 8;                       // two 16-byte vectors per thread
constexpr int SGD_TILE = SGD_BLOCK * SGD_PER_THREAD;    // elements per block

struct SgdDesc {            // device descriptor (32 bytes)
    float *p;
    const float *g;
    float *buf;             // momentum buffer or null
    int n;                  // elements
    int blk_end;            // inclusive prefix of blocks; bit 31 of `n` is not used
};

// torch's kernel is compiled with floating-point contraction, this library without (the voxel / kNN
// kernels must round every operation like the reference's): the fused multiply-adds are spelled out.
// The new buffer value is a double there; only the Nesterov term sees it unrounded (tools/sgdprobe.py).
__device__ __forceinline__ void sgd_one(float &p, float g, float *buf, bool first, double lr, double momentum,
                                        double dampening, double wd, bool nesterov, bool maximize) {
    if (maximize) g = -g;
    if (wd != 0.0) g = (float)fma(wd, (double)p, (double)g);
    if (buf) {
        const double b = first ? (double)g : fma(momentum, (double)*buf, (1.0 - dampening) * (double)g);
        *buf = (float)b;
        g = nesterov ? (float)fma(momentum, b, (double)g) : (float)b;
    }
    p = (float)fma(-lr, (double)g, (double)p);
}

__global__ __launch_bounds__(SGD_BLOCK) void sgd_multi(const SgdDesc *__restrict__ descs, const int *__restrict__ first,
                                                       int n_desc, double lr, double momentum, double dampening,
                                                       double wd, int nesterov, int maximize) {
    int lo = 0, hi = n_desc - 1;
    while (lo < hi) {   // first descriptor whose inclusive end exceeds this block
        const int mid = (lo + hi) >> 1;
        if ((int)blockIdx.x < descs[mid].blk_end) hi = mid; else lo = mid + 1;
    }
    const SgdDesc d = descs[lo];
    const bool is_first = first[lo] != 0;
    const int blk = (int)blockIdx.x - (lo == 0 ? 0 : descs[lo - 1].blk_end);
    const long long base = (long long)blk * SGD_TILE;
    const bool vec = (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.buf) & 15) == 0;
#pragma unroll
    for (int k = 0; k < SGD_PER_THREAD / 4; ++k) {
        const long long e = base + ((long long)k * SGD_BLOCK + threadIdx.x) * 4;
        if (e >= d.n) break;
        if (vec && e + 3 < d.n) {
            float4 p = *reinterpret_cast<float4 *>(d.p + e);
            const float4 g = *reinterpret_cast<const float4 *>(d.g + e);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (d.buf && !is_first) b = *reinterpret_cast<const float4 *>(d.buf + e);
            sgd_one(p.x, g.x, d.buf ? &b.x : nullptr, is_first, lr, momentum, dampening, wd, nesterov, maximize);
            sgd_one(p.y, g.y, d.buf ? &b.y : nullptr, is_first, lr, momentum, dampening, wd, nesterov, maximize);
            sgd_one(p.z, g.z, d.buf ? &b.z : nullptr, is_first, lr, momentum, dampening, wd, nesterov, maximize);
            sgd_one(p.w, g.w, d.buf ? &b.w : nullptr, is_first, lr, momentum, dampening, wd, nesterov, maximize);
            *reinterpret_cast<float4 *>(d.p + e) = p;
            if (d.buf) *reinterpret_cast<float4 *>(d.buf + e) = b;
        } else {
            for (int q = 0; q < 4 && e + q < d.n; ++q) {
                float p = d.p[e + q];
                float b = (d.buf && !is_first) ? d.buf[e + q] : 0.f;
                sgd_one(p, d.g[e + q], d.buf ? &b : nullptr, is_first, lr, momentum, dampening, wd, nesterov, maximize);
                d.p[e + q] = p;
                if (d.buf) d.buf[e + q] = b;
            }
        }
    }
}

// ---- include/doda_optim.h: SGD / Adam / AdamW with the gradient-norm clip folded in --------------------------------
// Same scheme as sgd_multi (descriptors in device memory, block-prefix binary search, 16-byte vectors with a scalar tail and an
// unaligned fallback).  The clip is two launches: grad_sqsum_multi leaves one fp64 partial per workgroup, and every workgroup of the
// update launch adds the partials in one fixed order in its prologue (the launch boundary is the only synchronisation: no float
// atomic, no ticket), so all workgroups scale by the same coef and a rerun gives the same bits.
constexpr int OPT_TILE = DODA_OPTIM_TILE;
static_assert(OPT_TILE == SGD_TILE, "both launches tile like sgd_multi");
// Grid cap of the sum-of-squares launch: two workgroups on each of the 256 CUs.  At 32 bytes in flight per thread that is 4 MB of
// outstanding loads, enough to cover HBM latency at full bandwidth, and each update workgroup's prologue re-reads only
// 512 x 8 B = 4 KB of partials from L2 (two per thread).  A larger cap buys no bandwidth and lengthens every prologue.
constexpr int NORM_CAP = DODA_OPTIM_NORM_BLOCKS;

struct OptDesc {            // device descriptor (56 bytes)
    float *p;
    float *g;
    float *s1;              // sgd: momentum buffer or null; adam: exp_avg
    float *s2;              // adam: exp_avg_sq
    int n;
    int blk_end;            // inclusive prefix of tiles
    float bc1, bc2s;        // adam: bias_correction1, bias_correction2_sqrt (torch's opmath_t for fp32 tensors is float)
    int first;              // sgd: the buffer holds no value yet
    int pad;
};

__device__ __forceinline__ int find_desc(const OptDesc *__restrict__ descs, int lo, int n_desc, int tile) {
    int hi = n_desc - 1;
    while (lo < hi) {   // first descriptor whose inclusive end exceeds this tile
        const int mid = (lo + hi) >> 1;
        if (tile < descs[mid].blk_end) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// sum over the workgroup in a fixed tree; every thread returns the total
__device__ __forceinline__ double block_sum(double a, double *sh) {
    sh[threadIdx.x] = a;
    doda_sync();
    for (int s = SGD_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        doda_sync();
    }
    return sh[0];
}

__global__ __launch_bounds__(SGD_BLOCK) void grad_sqsum_multi(const OptDesc *__restrict__ descs, int n_desc, int n_tiles,
                                                              double *__restrict__ partial) {
    __shared__ double sh[SGD_BLOCK];
    double acc = 0.0;       // (double)g * (double)g is exact; the fma rounds the sum once per term
    int lo = 0;             // tiles only grow along the stride: the search resumes where it stood
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        lo = find_desc(descs, lo, n_desc, (int)tile);
        const float *g = descs[lo].g;
        const int n = descs[lo].n;
        const long long base = (tile - (lo == 0 ? 0 : descs[lo - 1].blk_end)) * OPT_TILE;
        const bool vec = ((uintptr_t)g & 15) == 0;
#pragma unroll
        for (int k = 0; k < SGD_PER_THREAD / 4; ++k) {
            const long long e = base + ((long long)k * SGD_BLOCK + threadIdx.x) * 4;
            if (e >= n) break;
            if (vec && e + 3 < n) {
                const float4 v = *reinterpret_cast<const float4 *>(g + e);
                acc = fma((double)v.x, (double)v.x, acc);
                acc = fma((double)v.y, (double)v.y, acc);
                acc = fma((double)v.z, (double)v.z, acc);
                acc = fma((double)v.w, (double)v.w, acc);
            } else {
                for (int q = 0; q < 4 && e + q < n; ++q) acc = fma((double)g[e + q], (double)g[e + q], acc);
            }
        }
    }
    const double total = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// torch's adam_math for fp32 tensors (opmath_t = float, hyper-parameters double), with the fused multiply-adds its build contracts
// spelled out (an fadd of two fmuls contracts on its left operand, an fsub of an fmul to fma(-a, b, c)); step_size, the square
// root, its quotient and the last line are float arithmetic there.
template <bool ADAMW>
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const doda_optim_hyper &h, float bc1, float bc2s) {
    if (h.maximize) g = -g;
    if (h.weight_decay != 0.0) {
        if (ADAMW) p = (float)fma(-(h.lr * h.weight_decay), (double)p, (double)p);
        else g = (float)fma((double)p, h.weight_decay, (double)g);
    }
    m = (float)fma(h.beta1, (double)m, (1.0 - h.beta1) * (double)g);
    v = (float)fma(h.beta2, (double)v, ((1.0 - h.beta2) * (double)g) * (double)g);
    const float step_size = (float)(h.lr / (double)bc1);
    const float denom = (float)((double)(sqrtf(v) / bc2s) + h.eps);
    p = p - step_size * m / denom;
}

template <int KIND>
__device__ __forceinline__ void optim_one(float &p, float g, float &a, float &b, const OptDesc &d, const doda_optim_hyper &h) {
    if (KIND == DODA_OPTIM_SGD)
        sgd_one(p, g, d.s1 ? &a : nullptr, d.first != 0, h.lr, h.beta1, h.beta2, h.weight_decay, h.nesterov != 0, h.maximize != 0);
    else
        adam_one<KIND == DODA_OPTIM_ADAMW>(p, g, a, b, h, d.bc1, d.bc2s);
}

template <int KIND, bool CLIP>
__global__ __launch_bounds__(SGD_BLOCK) void optim_multi(const OptDesc *__restrict__ descs, int n_desc, doda_optim_hyper h,
                                                         const double *__restrict__ partial, int n_partial, double max_norm,
                                                         float *__restrict__ norm_out) {
    float coef = 1.f;
    if (CLIP) {
        __shared__ double sh[SGD_BLOCK];
        double a = 0.0;
        for (int i = threadIdx.x; i < n_partial; i += SGD_BLOCK) a += partial[i];
        const double norm = sqrt(block_sum(a, sh));
        const double c = max_norm / (norm + 1e-6);
        coef = (float)(c > 1.0 ? 1.0 : c);      // a NaN norm stays a NaN coef (fmin would drop it)
        if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    }
    constexpr bool ADAM = KIND != DODA_OPTIM_SGD;
    const int lo = find_desc(descs, 0, n_desc, (int)blockIdx.x);
    const OptDesc d = descs[lo];
    const long long base = (long long)((int)blockIdx.x - (lo == 0 ? 0 : descs[lo - 1].blk_end)) * OPT_TILE;
    const bool has1 = ADAM || d.s1 != nullptr, load1 = ADAM || (d.s1 != nullptr && !d.first);
    const bool vec = (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.s1 | (uintptr_t)(ADAM ? d.s2 : nullptr)) & 15) == 0;
#pragma unroll
    for (int k = 0; k < SGD_PER_THREAD / 4; ++k) {
        const long long e = base + ((long long)k * SGD_BLOCK + threadIdx.x) * 4;
        if (e >= d.n) break;
        if (vec && e + 3 < d.n) {
            float4 p = *reinterpret_cast<float4 *>(d.p + e);
            float4 g = *reinterpret_cast<const float4 *>(d.g + e);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (load1) a = *reinterpret_cast<const float4 *>(d.s1 + e);
            if (ADAM) b = *reinterpret_cast<const float4 *>(d.s2 + e);
            if (CLIP) {
                g.x *= coef; g.y *= coef; g.z *= coef; g.w *= coef;
                *reinterpret_cast<float4 *>(d.g + e) = g;
            }
            optim_one<KIND>(p.x, g.x, a.x, b.x, d, h);
            optim_one<KIND>(p.y, g.y, a.y, b.y, d, h);
            optim_one<KIND>(p.z, g.z, a.z, b.z, d, h);
            optim_one<KIND>(p.w, g.w, a.w, b.w, d, h);
            *reinterpret_cast<float4 *>(d.p + e) = p;
            if (has1) *reinterpret_cast<float4 *>(d.s1 + e) = a;
            if (ADAM) *reinterpret_cast<float4 *>(d.s2 + e) = b;
        } else {
            for (int q = 0; q < 4 && e + q < d.n; ++q) {
                float p = d.p[e + q], g = d.g[e + q];
                float a = load1 ? d.s1[e + q] : 0.f, b = ADAM ? d.s2[e + q] : 0.f;
                if (CLIP) { g *= coef; d.g[e + q] = g; }
                optim_one<KIND>(p, g, a, b, d, h);
                d.p[e + q] = p;
                if (has1) d.s1[e + q] = a;
                if (ADAM) d.s2[e + q] = b;
            }
        }
    }
}

template <int KIND>
void launch_optim(bool clip, unsigned blocks, hipStream_t s, const OptDesc *descs, int n_desc, const doda_optim_hyper &h,
                  const double *partial, int n_partial, double max_norm, float *norm_out) {
    if (clip)
        hipLaunchKernelGGL((optim_multi<KIND, true>), dim3(blocks), dim3(SGD_BLOCK), 0, s, descs, n_desc, h, partial, n_partial,
                           max_norm, norm_out);
    else
        hipLaunchKernelGGL((optim_multi<KIND, false>), dim3(blocks), dim3(SGD_BLOCK), 0, s, descs, n_desc, h, partial, n_partial,
                           max_norm, norm_out);
}

// pinned staging ring for the descriptor upload (grow-only slots, reuse of a slot guarded by its event)
struct Slot {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int ev_dev = -1;    // device the event was created on (an event can only be recorded on that device's streams)
    bool pending = false;
};
std::mutex g_mu;
Slot g_slot[4];
unsigned g_next = 0;

// under g_mu: the next slot of the ring, its previous upload complete, at least `need` bytes, its event on the current device
int acquire_slot(size_t need, Slot **out) {
    Slot &sl = g_slot[g_next++ & 3u];
    if (sl.pending) { hipEventSynchronize(sl.ev); sl.pending = false; }
    if (sl.cap < need) {
        if (sl.host) hipHostFree(sl.host);
        sl.cap = align_up(need, 4096) * 2;
        if (hipHostMalloc(&sl.host, sl.cap, hipHostMallocDefault) != hipSuccess) { sl.host = nullptr; sl.cap = 0; return DODA_ERR_NOMEM; }
    }
    int cur_dev = 0;
    hipGetDevice(&cur_dev);
    if (sl.ev && sl.ev_dev != cur_dev) { hipEventDestroy(sl.ev); sl.ev = nullptr; }   // library used from another device
    if (!sl.ev && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) return DODA_ERR_LAUNCH;
    sl.ev_dev = cur_dev;
    *out = &sl;
    return DODA_OK;
}

// under g_mu: the slot's first `bytes` bytes to the device on `s`; the slot is busy until the copy has run
int upload_slot(Slot &sl, void *dev, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(dev, sl.host, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return DODA_ERR_LAUNCH;
    hipEventRecord(sl.ev, s);
    sl.pending = true;
    return DODA_OK;
}

}  // namespace

extern "C" size_t doda_sgd_multi_desc_bytes(int32_t n_tensors) {
    if (n_tensors <= 0) return 0;
    return align_up((size_t)n_tensors * sizeof(SgdDesc), 16) + align_up((size_t)n_tensors * sizeof(int), 16);
}

extern "C" int doda_sgd_multi(const doda_sgd_tensor *t, int32_t n_tensors, double lr, double momentum, double dampening,
                              double weight_decay, int32_t nesterov, int32_t maximize, void *desc_dev,
                              size_t desc_bytes, doda_stream_t stream) {
    if (n_tensors == 0) return DODA_OK;
    if (n_tensors < 0 || !t || !desc_dev) return DODA_ERR_INVALID;
    const size_t need = doda_sgd_multi_desc_bytes(n_tensors);
    if (desc_bytes < need) return DODA_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    const size_t first_off = align_up((size_t)n_tensors * sizeof(SgdDesc), 16);
    long long blocks = 0;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Slot *sl = nullptr;
        if (const int st = acquire_slot(need, &sl)) return st;
        SgdDesc *d = (SgdDesc *)sl->host;
        int *first = (int *)((char *)sl->host + first_off);
        for (int k = 0; k < n_tensors; ++k) {
            if (!t[k].p || !t[k].g || t[k].n < 0 || t[k].n > 0x7fffffffll) return DODA_ERR_INVALID;
            if (momentum != 0.0 && !t[k].buf) return DODA_ERR_INVALID;
            blocks += (t[k].n + SGD_TILE - 1) / SGD_TILE;
            if (blocks > 0x7fffffffll) return DODA_ERR_UNSUPPORTED;
            d[k].p = t[k].p; d[k].g = t[k].g; d[k].buf = momentum != 0.0 ? t[k].buf : nullptr;
            d[k].n = (int)t[k].n; d[k].blk_end = (int)blocks;
            first[k] = t[k].first_step ? 1 : 0;
        }
        if (blocks == 0) return DODA_OK;
        if (const int st = upload_slot(*sl, desc_dev, need, s)) return st;
    }
    hipLaunchKernelGGL(sgd_multi, dim3((unsigned)blocks), dim3(SGD_BLOCK), 0, s, (const SgdDesc *)desc_dev,
                       (const int *)((const char *)desc_dev + first_off), n_tensors, lr, momentum, dampening,
                       weight_decay, nesterov, maximize);
    return doda_check_launch();
}

// ---- include/doda_optim.h ---------------------------------------------------------------------------------------
extern "C" int32_t doda_optim_abi_version(void) { return DODA_OPTIM_ABI_VERSION; }

extern "C" size_t doda_optim_workspace_bytes(int32_t n_tensors) {
    if (n_tensors <= 0) return 0;
    return align_up((size_t)n_tensors * sizeof(OptDesc), 16) + (size_t)NORM_CAP * sizeof(double);
}

extern "C" int doda_optim_step(const doda_optim_tensor *t, int32_t n_tensors, int32_t kind, const doda_optim_hyper *hyper,
                               double max_norm, float *norm_out, void *ws, size_t ws_bytes, doda_stream_t stream) {
    if (n_tensors == 0) return DODA_OK;
    if (n_tensors < 0 || !t || !hyper || !ws || ((uintptr_t)ws & 15)) return DODA_ERR_INVALID;
    if (kind != DODA_OPTIM_SGD && kind != DODA_OPTIM_ADAM && kind != DODA_OPTIM_ADAMW) return DODA_ERR_INVALID;
    const bool clip = max_norm > 0.0;
    if (clip && !norm_out) return DODA_ERR_INVALID;
    const doda_optim_hyper h = *hyper;
    const bool adam = kind != DODA_OPTIM_SGD;
    const bool need1 = adam || h.beta1 != 0.0;      // sgd: beta1 carries the momentum
    long long blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        if (t[k].n < 0 || t[k].n > 0x7fffffffll) return DODA_ERR_INVALID;
        if (t[k].n > 0 && (!t[k].p || !t[k].g || (need1 && !t[k].state1) || (adam && !t[k].state2))) return DODA_ERR_INVALID;
        blocks += (t[k].n + OPT_TILE - 1) / OPT_TILE;
        if (blocks > 0x7fffffffll) return DODA_ERR_UNSUPPORTED;
    }
    const size_t need = doda_optim_workspace_bytes(n_tensors);
    if (ws_bytes < need) return DODA_ERR_WORKSPACE;
    if (blocks == 0) return DODA_OK;
    hipStream_t s = as_stream(stream);
    const size_t desc_bytes = align_up((size_t)n_tensors * sizeof(OptDesc), 16);
    {
        std::lock_guard<std::mutex> lock(g_mu);
        Slot *sl = nullptr;
        if (const int st = acquire_slot(desc_bytes, &sl)) return st;
        OptDesc *d = (OptDesc *)sl->host;
        long long end = 0;
        for (int k = 0; k < n_tensors; ++k) {
            end += (t[k].n + OPT_TILE - 1) / OPT_TILE;
            d[k].p = t[k].p; d[k].g = t[k].g;
            d[k].s1 = need1 ? t[k].state1 : nullptr;
            d[k].s2 = adam ? t[k].state2 : nullptr;
            d[k].n = (int)t[k].n; d[k].blk_end = (int)end;
            d[k].bc1 = (float)t[k].bias_correction1; d[k].bc2s = (float)t[k].bias_correction2_sqrt;
            d[k].first = t[k].first_step ? 1 : 0;
            d[k].pad = 0;
        }
        if (const int st = upload_slot(*sl, ws, desc_bytes, s)) return st;
    }
    const OptDesc *descs = (const OptDesc *)ws;
    double *partial = (double *)((char *)ws + desc_bytes);
    const int n_partial = clip ? (int)(blocks < NORM_CAP ? blocks : NORM_CAP) : 0;
    if (clip) {
        hipLaunchKernelGGL(grad_sqsum_multi, dim3((unsigned)n_partial), dim3(SGD_BLOCK), 0, s, descs, (int)n_tensors, (int)blocks,
                           partial);
        if (const int st = doda_check_launch()) return st;
    }
    if (kind == DODA_OPTIM_SGD) launch_optim<DODA_OPTIM_SGD>(clip, (unsigned)blocks, s, descs, n_tensors, h, partial, n_partial, max_norm, norm_out);
    else if (kind == DODA_OPTIM_ADAM) launch_optim<DODA_OPTIM_ADAM>(clip, (unsigned)blocks, s, descs, n_tensors, h, partial, n_partial, max_norm, norm_out);
    else launch_optim<DODA_OPTIM_ADAMW>(clip, (unsigned)blocks, s, descs, n_tensors, h, partial, n_partial, max_norm, norm_out);
    return doda_check_launch();
}

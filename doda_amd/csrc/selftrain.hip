// Pseudo labels of the self-training stage (include/doda_selftrain.h): the point store, the radix-select histograms and the
// labelling pass.
//
// reference util/pseudo_labels_util.py:93-142 files every target point's confidence under its predicted class in Python lists
// (pandas groupby, list.sort: ~10^8 floats for ScanNet) and takes sorted[max(1, int(r * n)) - 1] per class.  Here the points'
// (class, confidence) pairs go to a device store once (5 bytes per point) and the k-th largest confidence of each class comes from
// integer histograms of the fp32 bit patterns (positive floats order as their uint32 bits): 4 levels of 8 bits, one pass over the
// store each, with the host choosing the bin that holds rank k between levels.  Every histogram is counted in an LDS-private copy
// per workgroup (uint32) and added to the int64 result with one integer atomic per non-empty bin: exact, independent of the order of
// arrival, and summable across ranks.
#include "common.hpp"
#include "../../include/doda_selftrain.h"

namespace {
constexpr int ST_BLOCK = 256;
constexpr int ST_BINS = 1 << DODA_ST_RADIX_BITS;
constexpr int ST_MAX_BLOCKS = 2048;      // grid-stride beyond: each workgroup's histogram flush is n_cls * 256 bins

inline int st_blocks(long long n) {
    long long nb = (n + ST_BLOCK * 4 - 1) / (ST_BLOCK * 4);
    if (nb > ST_MAX_BLOCKS) nb = ST_MAX_BLOCKS;
    return nb < 1 ? 1 : (int)nb;
}

__device__ __forceinline__ void st_hist_zero(unsigned *h, int n) {
    for (int e = threadIdx.x; e < n; e += ST_BLOCK) h[e] = 0u;
    doda_sync();
}
__device__ __forceinline__ void st_hist_flush(const unsigned *h, int n, int64_t *out) {
    doda_sync();
    for (int e = threadIdx.x; e < n; e += ST_BLOCK) {
        const unsigned v = h[e];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(out + e), (unsigned long long)v);
    }
}

// store_cls / store_conf at offset + i <- pred / conf of point i's voxel; hist (optional): level 0 (the top 8 key bits) per class
__global__ __launch_bounds__(ST_BLOCK) void st_point_store(const int32_t *__restrict__ pred, const float *__restrict__ conf, int m,
                                                          const int32_t *__restrict__ p2v, long long n, int n_cls,
                                                          uint8_t *__restrict__ store_cls, float *__restrict__ store_conf,
                                                          long long offset, int64_t *__restrict__ hist) {
    extern __shared__ unsigned sh[];
    const int nh = hist ? n_cls * ST_BINS : 0;
    st_hist_zero(sh, nh);
    for (long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * ST_BLOCK) {
        const int v = p2v[i];
        int c = 0;
        float x = 0.f;
        if (v >= 0 && v < m) { c = pred[v]; x = conf[v]; }
        c = c < 0 ? 0 : (c >= n_cls ? n_cls - 1 : c);      // (pred comes from doda_st_voxel_confidence: in range)
        store_cls[offset + i] = (uint8_t)c;
        store_conf[offset + i] = x;
        if (nh) atomicAdd(&sh[c * ST_BINS + (__float_as_uint(x) >> 24)], 1u);
    }
    if (nh) st_hist_flush(sh, nh, hist);
}

// one radix level: hist[c][bin of this level] over the points of class c whose higher key bits equal prefix[c]
__global__ __launch_bounds__(ST_BLOCK) void st_radix_hist(const uint8_t *__restrict__ store_cls, const float *__restrict__ store_conf,
                                                         long long n, int n_cls, int level, const int32_t *__restrict__ prefix,
                                                         int64_t *__restrict__ hist) {
    extern __shared__ unsigned sh[];
    __shared__ unsigned pre[DODA_ST_MAX_CLASSES];
    const int nh = n_cls * ST_BINS;
    const int shift = 8 * (DODA_ST_RADIX_LEVELS - 1 - level);
    if (threadIdx.x < n_cls) pre[threadIdx.x] = level == 0 ? 0u : (unsigned)prefix[threadIdx.x];
    st_hist_zero(sh, nh);
    for (long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * ST_BLOCK) {
        const int c = store_cls[i];
        if (c >= n_cls) continue;
        const unsigned key = __float_as_uint(store_conf[i]);
        // (level 0: no higher bits; a finished class's prefix, 0xffffffff, matches no key >> 8 or more)
        const unsigned hi = level == 0 ? 0u : key >> (shift + 8);
        if (hi == pre[c]) atomicAdd(&sh[c * ST_BINS + ((key >> shift) & (ST_BINS - 1))], 1u);
    }
    st_hist_flush(sh, nh, hist);
}

__global__ __launch_bounds__(ST_BLOCK) void st_label(const uint8_t *__restrict__ store_cls, const float *__restrict__ store_conf,
                                                    long long n, int n_cls, const float *__restrict__ thres, int ignore,
                                                    uint8_t *__restrict__ labels, int64_t *__restrict__ kept) {
    __shared__ float t[DODA_ST_MAX_CLASSES];
    __shared__ unsigned cnt[DODA_ST_MAX_CLASSES];
    if (threadIdx.x < n_cls) { t[threadIdx.x] = thres[threadIdx.x]; cnt[threadIdx.x] = 0u; }
    doda_sync();
    for (long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * ST_BLOCK) {
        const int c = store_cls[i];
        const bool keep = c < n_cls && store_conf[i] > t[c];
        labels[i] = keep ? (uint8_t)c : (uint8_t)ignore;
        if (keep) atomicAdd(&cnt[c], 1u);
    }
    doda_sync();
    if (threadIdx.x < n_cls && cnt[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long *>(kept + threadIdx.x), (unsigned long long)cnt[threadIdx.x]);
}
}  // namespace

extern "C" int32_t doda_st_abi_version(void) { return DODA_ST_ABI_VERSION; }

extern "C" int doda_st_point_store(const int32_t *pred, const float *conf, int32_t m, const int32_t *p2v, int64_t n_points,
                                   int32_t n_cls, uint8_t *store_cls, float *store_conf, int64_t store_len, int64_t offset,
                                   int64_t *hist, doda_stream_t stream) {
    if (m < 0 || n_points < 0 || offset < 0 || store_len < 0 || offset > store_len || n_points > store_len - offset)
        return DODA_ERR_INVALID;
    if (n_cls < 1 || n_cls > DODA_ST_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    if (n_points == 0) return DODA_OK;
    if (!pred || !conf || !p2v || !store_cls || !store_conf || m == 0) return DODA_ERR_INVALID;
    const size_t lds = hist ? (size_t)n_cls * ST_BINS * sizeof(unsigned) : 0;
    hipLaunchKernelGGL(st_point_store, dim3(st_blocks(n_points)), dim3(ST_BLOCK), lds, as_stream(stream), pred, conf, (int)m, p2v,
                       (long long)n_points, (int)n_cls, store_cls, store_conf, (long long)offset, hist);
    return doda_check_launch();
}

extern "C" int doda_st_radix_hist(const uint8_t *store_cls, const float *store_conf, int64_t n, int32_t n_cls, int32_t level,
                                  const int32_t *prefix, int64_t *hist, doda_stream_t stream) {
    if (n < 0 || level < 0 || level >= DODA_ST_RADIX_LEVELS || !hist || (level > 0 && !prefix)) return DODA_ERR_INVALID;
    if (n_cls < 1 || n_cls > DODA_ST_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    if (n == 0) return DODA_OK;
    if (!store_cls || !store_conf) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(st_radix_hist, dim3(st_blocks(n)), dim3(ST_BLOCK), (size_t)n_cls * ST_BINS * sizeof(unsigned),
                       as_stream(stream), store_cls, store_conf, (long long)n, (int)n_cls, (int)level, prefix, hist);
    return doda_check_launch();
}

extern "C" int doda_st_label(const uint8_t *store_cls, const float *store_conf, int64_t n, int32_t n_cls, const float *thres,
                             int32_t ignore, uint8_t *labels, int64_t *kept, doda_stream_t stream) {
    if (n < 0 || ignore < 0 || ignore > 255 || !thres || !kept) return DODA_ERR_INVALID;
    if (n_cls < 1 || n_cls > DODA_ST_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    if (n == 0) return DODA_OK;
    if (!store_cls || !store_conf || !labels) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(st_label, dim3(st_blocks(n)), dim3(ST_BLOCK), 0, as_stream(stream), store_cls, store_conf, (long long)n,
                       (int)n_cls, thres, (int)ignore, labels, kept);
    return doda_check_launch();
}

// The rest of the reference's PG_OP module (include/doda_pgops.h): clustering, segment pools, proposal IoU.
//
// Clustering.  The reference's bfs_cluster is host code: a sequential BFS over the ball-query lists (bfs_cluster.cpp:28-86), kept
// here as doda_pg_bfs_cluster_h for CPU tensors.  On the device the same clusters come from connected components by a lock-free
// union-find (doda_pg_components) in four launches — init, hook, flatten, count — with no convergence loop, no host read-back and
// no float atomic.  The invariant that bounds every loop: parent[x] <= x always (a hook links the LARGER root under the smaller,
// pointer jumping only lowers a parent), so every parent chain strictly decreases and ends, after at most x steps, in a root; and
// the root of a finished component is its smallest index, whatever the order in which the hooks landed.
//
// Every word of parent[] that the hook launch shares between workgroups is read and written with agent-scope atomics (the
// eight XCDs have private L2s and every CU a private L1: a plain load may return a line that is stale for the whole launch).
//
// Segment pools: one workgroup per segment; its threads are (row lane, channel lane) with as many channel lanes as the row has
// floats (up to 64), so a wave instruction reads whole rows of consecutive addresses and a long segment is covered by all row lanes
// of all waves together.  A lane keeps (value, row) with the reference's strict compare, lanes are combined by value, then by smaller row: the
// result is the sequential loop's, bit for bit (also for +0 / -0 and NaN, which a strict compare never lets win).
#include "common.hpp"
#include "../../include/doda_pgops.h"

#include <math.h>
#include <vector>

namespace {

constexpr int PG_BLOCK = 256;

__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------
// union-find
// ---------------------------------------------------------------------------------------------
// Root of x, halving the path on the way.
__device__ __forceinline__ int uf_find(int *parent, int x) {
    int p = ld_agent(parent + x);
    // Bound: p < x whenever the loop continues (parent[y] <= y for every y), so x strictly decreases: at most x iterations.
    while (p != x) {
        const int gp = ld_agent(parent + p);
        if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // only ever lowers it
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
    // Bound: an iteration ends the loop, or its CAS failed.  The CAS fails only if parent[hi] was no longer hi, i.e. another lane
    // hooked the root hi under a smaller one since uf_find returned it — progress by that lane, and a root is hooked once, so over
    // the whole launch fewer than n CAS fail.  After a failure the search goes on from the value the CAS returned (a current
    // ancestor, read at the L2), never from a cached word.
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = expected;   // < hi
        b = lo;
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_init(int *__restrict__ parent, int *__restrict__ size, int n) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i < n) {
        parent[i] = i;
        size[i] = 0;
    }
}

// the clamped range [s, e) of point i's list inside ball_query_idxs[0 .. n_active)
__device__ __forceinline__ void list_range(const int *__restrict__ start_len, int i, int n_active, int &s, int &e) {
    const long long st = start_len[2 * (size_t)i], ln = start_len[2 * (size_t)i + 1];
    const long long lo = st < 0 ? 0 : (st > n_active ? n_active : st);
    long long hi = st + ln;          // (two int32: no overflow in 64 bits)
    hi = hi > n_active ? n_active : hi;
    s = (int)lo;
    e = hi < lo ? (int)lo : (int)hi;
}

__device__ __forceinline__ void hook_edge(int *parent, const int *__restrict__ label, int i, int li, int j, int n) {
    if ((unsigned)j >= (unsigned)n || j == i) return;   // corrupt neighbour index / self entry
    if (label[j] != li) return;
    uf_union(parent, i, j);
}

// One lane per point for lists of up to DODA_PG_WAVE_LIST entries; the points of a wave with longer lists are then taken one at a
// time by the whole wave, 64 entries per step, so a hub with thousands of neighbours costs its wave len / 64 steps, not len.
__global__ __launch_bounds__(PG_BLOCK) void pg_hook(const int *__restrict__ label, const int *__restrict__ idxs,
                                                   const int *__restrict__ start_len, int n, int n_active, int *parent) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    int s = 0, e = 0, li = 0;
    if (i < n) {
        list_range(start_len, i, n_active, s, e);
        li = label[i];
    }
    const bool wide = e - s > DODA_PG_WAVE_LIST;
    if (!wide)
        for (int k = s; k < e; ++k) hook_edge(parent, label, i, li, idxs[k], n);   // at most DODA_PG_WAVE_LIST steps
    unsigned long long todo = __ballot(wide);
    // Bound: one set bit of `todo` is cleared per iteration: at most 64.
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pi = __shfl(i, src, 64), ps = __shfl(s, src, 64), pe = __shfl(e, src, 64), pl = __shfl(li, src, 64);
        for (int k = ps + lane_id(); k < pe; k += DODA_WAVE) hook_edge(parent, label, pi, pl, idxs[k], n);
    }
}

// parent[i] = root of i.  A word is only ever replaced by a smaller ancestor (here: by the root itself), so concurrent walks of
// other lanes through it stay on their chain whichever value they see.
__global__ __launch_bounds__(PG_BLOCK) void pg_flatten(int *parent, int n) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= n) return;
    int x = i, p = ld_agent(parent + x);
    // Bound: as in uf_find — p < x while the loop runs.
    while (p != x) {
        x = p;
        p = ld_agent(parent + x);
    }
    __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// size[root] = number of points below it: integer atomics, one per distinct root of a wave.
__global__ __launch_bounds__(PG_BLOCK) void pg_count(const int *__restrict__ root, int *__restrict__ size, int n) {
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    const int r = i < n ? root[i] : -1;
    unsigned long long todo = __ballot(r >= 0);
    // Bound: the lanes that share the first pending lane's root (that lane among them) leave `todo` each iteration: at most 64.
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(r, src, 64);
        const unsigned long long same = __ballot(r == r0) & todo;
        if (lane_id() == src) atomicAdd(size + r0, __popcll(same));
        todo &= ~same;
    }
}

// ---------------------------------------------------------------------------------------------
// segment pools
// ---------------------------------------------------------------------------------------------
enum { SEG_MEAN = 0, SEG_MIN = 1, SEG_MAX = 2 };

__device__ __forceinline__ void seg_range(const int *__restrict__ offsets, int s, int n_rows, int &lo, int &hi) {
    int a = offsets[s], b = offsets[s + 1];
    a = a < 0 ? 0 : (a > n_rows ? n_rows : a);
    b = b < 0 ? 0 : (b > n_rows ? n_rows : b);
    lo = a;
    hi = b < a ? a : b;
}

// does (v, r) beat (bv, br)?  r < 0: no candidate.  Strictly better value, or the same value in an earlier row.
template <int OP>
__device__ __forceinline__ bool seg_beats(float v, int r, float bv, int br) {
    if (r < 0) return false;
    if (br < 0) return true;
    const bool better = OP == SEG_MIN ? v < bv : v > bv;
    return better || (v == bv && r < br);
}

// One workgroup per segment (grid-stride).  cl = channel lanes (power of two, <= 64), BLOCK / cl row lanes; the row lanes of a wave
// are folded with shuffles, the waves through LDS in wave order.  BLOCK is 256, or 1024 where the segments are long on average
// (seg_long): the trip counts of both outer loops are the same for every thread of the workgroup, so every thread meets every barrier.
template <int OP, bool WITH_IDX, int BLOCK>
__global__ __launch_bounds__(BLOCK) void pg_seg_pool(const float *__restrict__ inp, const int *__restrict__ offsets,
                                                    float *__restrict__ out, int *__restrict__ maxidx, int n_rows, int n_seg,
                                                    int c, int cl) {
    constexpr int WAVES = BLOCK / DODA_WAVE;
    __shared__ float s_val[WAVES][DODA_WAVE];
    __shared__ int s_arg[WAVES][DODA_WAVE];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int ch0 = threadIdx.x & (cl - 1), row0 = threadIdx.x / cl, rl = BLOCK / cl;
    for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
        int lo, hi;
        seg_range(offsets, s, n_rows, lo, hi);
        const float count = (float)(hi - lo);
        for (int cb = 0; cb < c; cb += cl) {
            const int ch = cb + ch0;
            float acc = OP == SEG_MEAN ? 0.f : (OP == SEG_MIN ? INFINITY : -INFINITY);
            int arg = -1;
            if (ch < c) {
                for (int r = lo + row0; r < hi; r += rl) {
                    const float x = inp[(size_t)r * c + ch];
                    if (OP == SEG_MEAN) {
                        acc += x / count;
                    } else if (OP == SEG_MIN ? x < acc : x > acc) {   // the reference's strict compare: NaN never wins
                        acc = x;
                        arg = r;
                    }
                }
            }
            for (int d = cl; d < DODA_WAVE; d <<= 1) {   // fold the row lanes of a channel: lane ^ d has the same channel
                const float ov = __shfl_xor(acc, d, 64);
                const int oa = __shfl_xor(arg, d, 64);
                if (OP == SEG_MEAN) {
                    acc += ov;      // (both partners add the same two values: every row lane ends with the same sum)
                } else if (seg_beats<OP>(ov, oa, acc, arg)) {
                    acc = ov;
                    arg = oa;
                }
            }
            s_val[wave][lane] = acc;
            s_arg[wave][lane] = arg;
            doda_sync();
            if (wave == 0 && lane < cl && ch < c) {      // (lane < cl: lane == ch0, and wave w's entry `lane` is this channel's)
                for (int w = 1; w < WAVES; ++w) {
                    const float ov = s_val[w][lane];
                    const int oa = s_arg[w][lane];
                    if (OP == SEG_MEAN) {
                        acc += ov;
                    } else if (seg_beats<OP>(ov, oa, acc, arg)) {
                        acc = ov;
                        arg = oa;
                    }
                }
                out[(size_t)s * c + ch] = acc;
                if (WITH_IDX) maxidx[(size_t)s * c + ch] = arg;
            }
            doda_sync();     // the entries are read before the next channel block or segment overwrites them
        }
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void pg_sec_mean_bp(float *__restrict__ d_inp, const int *__restrict__ offsets,
                                                       const float *__restrict__ d_out, int n_rows, int n_seg, int c, int cl) {
    const int ch0 = threadIdx.x & (cl - 1), row0 = threadIdx.x / cl, rl = BLOCK / cl;
    for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
        int lo, hi;
        seg_range(offsets, s, n_rows, lo, hi);
        if (hi == lo) continue;
        const float count = (float)(hi - lo);
        for (int ch = ch0; ch < c; ch += cl) {
            const float g = d_out[(size_t)s * c + ch] / count;
            for (int r = lo + row0; r < hi; r += rl) d_inp[(size_t)r * c + ch] = g;
        }
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_roipool_bp(float *__restrict__ d_feats, const int *__restrict__ maxidx,
                                                         const float *__restrict__ d_out, int n_rows, long long total, int c) {
    const long long e = (long long)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int arg = maxidx[e];
    if ((unsigned)arg >= (unsigned)n_rows) return;   // -1: the segment had no maximum
    d_feats[(size_t)arg * c + (int)(e % c)] += d_out[e];
}

// ---------------------------------------------------------------------------------------------
// proposal IoU
// ---------------------------------------------------------------------------------------------
// One workgroup per proposal: an integer histogram of the proposal's instance labels (LDS, or this proposal's row of the
// workspace), then one quotient per instance.
template <bool IN_LDS>
__global__ __launch_bounds__(PG_BLOCK) void pg_get_iou(const int *__restrict__ proposals_idx, const int *__restrict__ proposals_offset,
                                                      const long long *__restrict__ instance_labels,
                                                      const int *__restrict__ instance_pointnum, float *__restrict__ iou,
                                                      int n_points, int sum_npoint, int n_instance, int *ws) {
    extern __shared__ int hist_lds[];
    const int p = blockIdx.x;
    int *hist = IN_LDS ? hist_lds : ws + (size_t)p * n_instance;
    for (int k = threadIdx.x; k < n_instance; k += PG_BLOCK) {
        if (IN_LDS) hist[k] = 0;
        else __hip_atomic_store(hist + k, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!IN_LDS) __threadfence();   // the zeroes have reached the L2 before another wave's atomic can
    doda_sync();
    int lo, hi;
    seg_range(proposals_offset, p, sum_npoint, lo, hi);
    for (int i = lo + threadIdx.x; i < hi; i += PG_BLOCK) {
        const int idx = proposals_idx[i];
        if ((unsigned)idx >= (unsigned)n_points) continue;
        const long long l = instance_labels[idx];
        if (l < 0 || l >= n_instance) continue;     // -100 and every other label without an instance
        atomicAdd(hist + (int)l, 1);
    }
    if (!IN_LDS) __threadfence();   // every wave's atomics are done before the counters are read back
    doda_sync();
    const int p_total = hi - lo;
    for (int k = threadIdx.x; k < n_instance; k += PG_BLOCK) {
        const int inter = IN_LDS ? hist[k] : ld_agent(hist + k);
        const float uni = (float)(p_total + instance_pointnum[k] - inter);
        iou[(size_t)p * n_instance + k] = (float)((double)(float)inter / ((double)uni + 1e-5));   // get_iou.cu:26, 1e-5 a double
    }
}

int seg_channel_lanes(int c) {
    int cl = 1;
    while (cl < c && cl < DODA_WAVE) cl <<= 1;
    return cl;
}

int seg_grid(int n_seg) { return n_seg < (1 << 20) ? n_seg : (1 << 20); }   // grid-stride above

// 1024-thread workgroups where a segment has DODA_PG_LONG_SEGMENT rows or more on average (the host knows the two counts, not the
// lengths): more row lanes per segment; the result does not depend on it for min / max / arg-max, and for the mean only the
// order of the additions does.
bool seg_long(int n_rows, int n_seg) { return (long long)n_rows >= (long long)DODA_PG_LONG_SEGMENT * n_seg; }

int seg_args_status(const void *inp, const void *offsets, const void *out, const void *extra, bool with_extra, int n_rows, int n_seg,
                    int c, bool *nothing) {
    *nothing = false;
    if (n_rows < 0 || n_seg < 0 || c < 0) return DODA_ERR_INVALID;
    if (n_seg == 0 || c == 0) {
        *nothing = true;
        return DODA_OK;
    }
    if (!offsets || !out || (with_extra && !extra) || (n_rows > 0 && !inp)) return DODA_ERR_INVALID;
    return DODA_OK;
}

template <int OP, bool WITH_IDX>
int seg_pool(const float *inp, const int32_t *offsets, float *out, int32_t *maxidx, int n_rows, int n_seg, int c,
             doda_stream_t stream) {
    bool nothing;
    const int st = seg_args_status(inp, offsets, out, maxidx, WITH_IDX, n_rows, n_seg, c, &nothing);
    if (st != DODA_OK || nothing) return st;
    const int cl = seg_channel_lanes(c);
    if (seg_long(n_rows, n_seg))
        pg_seg_pool<OP, WITH_IDX, 1024><<<seg_grid(n_seg), 1024, 0, as_stream(stream)>>>(inp, offsets, out, maxidx, n_rows, n_seg, c, cl);
    else
        pg_seg_pool<OP, WITH_IDX, PG_BLOCK><<<seg_grid(n_seg), PG_BLOCK, 0, as_stream(stream)>>>(inp, offsets, out, maxidx, n_rows, n_seg,
                                                                                             c, cl);
    return doda_check_launch();
}

}  // namespace

extern "C" {

int32_t doda_pgops_abi_version(void) { return DODA_PGOPS_ABI_VERSION; }

int doda_pg_components(const int32_t *semantic_label, const int32_t *ball_query_idxs, const int32_t *start_len, int32_t n,
                       int32_t n_active, int32_t *root, int32_t *size, doda_stream_t stream) {
    if (n < 0 || n_active < 0) return DODA_ERR_INVALID;
    if (n == 0) return DODA_OK;
    if (!semantic_label || !start_len || !root || !size || (n_active > 0 && !ball_query_idxs)) return DODA_ERR_INVALID;
    const int grid = div_up(n, PG_BLOCK);
    hipStream_t s = as_stream(stream);
    pg_init<<<grid, PG_BLOCK, 0, s>>>(root, size, n);
    pg_hook<<<grid, PG_BLOCK, 0, s>>>(semantic_label, ball_query_idxs, start_len, n, n_active, root);
    pg_flatten<<<grid, PG_BLOCK, 0, s>>>(root, n);
    pg_count<<<grid, PG_BLOCK, 0, s>>>(root, size, n);
    return doda_check_launch();
}

int doda_pg_bfs_cluster_h(const int32_t *semantic_label, const int32_t *ball_query_idxs, const int32_t *start_len, int32_t n,
                          int32_t n_active, int32_t threshold, int32_t *cluster_idxs, int32_t *cluster_offsets,
                          int32_t *sum_npoint, int32_t *n_cluster) {
    if (n < 0 || n_active < 0 || !sum_npoint || !n_cluster || !cluster_offsets) return DODA_ERR_INVALID;
    if (n > 0 && (!semantic_label || !start_len || !cluster_idxs)) return DODA_ERR_INVALID;
    if (n_active > 0 && !ball_query_idxs) return DODA_ERR_INVALID;
    std::vector<char> visited((size_t)n, 0);
    std::vector<int32_t> queue((size_t)n);   // a component's stretch of the queue is its points in first-visit order
    int32_t total = 0, clusters = 0;
    cluster_offsets[0] = 0;
    for (int32_t seed = 0; seed < n; ++seed) {
        if (visited[seed]) continue;
        size_t head = 0, tail = 0;
        queue[tail++] = seed;
        visited[seed] = 1;
        while (head < tail) {
            const int32_t cur = queue[head++];
            const long long st = start_len[2 * (size_t)cur], ln = start_len[2 * (size_t)cur + 1];
            long long lo = st < 0 ? 0 : (st > n_active ? n_active : st);
            long long hi = st + ln > n_active ? n_active : st + ln;
            const int32_t label = semantic_label[cur];
            for (long long k = lo; k < hi; ++k) {
                const int32_t j = ball_query_idxs[k];
                if (j < 0 || j >= n) continue;
                if (semantic_label[j] != label || visited[j]) continue;
                visited[j] = 1;
                queue[tail++] = j;
            }
        }
        if ((long long)tail < (long long)threshold) continue;
        for (size_t k = 0; k < tail; ++k) {
            cluster_idxs[2 * ((size_t)total + k)] = clusters;
            cluster_idxs[2 * ((size_t)total + k) + 1] = queue[k];
        }
        total += (int32_t)tail;
        cluster_offsets[++clusters] = total;
    }
    *sum_npoint = total;
    *n_cluster = clusters;
    return DODA_OK;
}

int doda_pg_sec_mean(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                     doda_stream_t stream) {
    return seg_pool<SEG_MEAN, false>(inp, offsets, out, nullptr, n_rows, n_seg, c, stream);
}

int doda_pg_sec_min(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                    doda_stream_t stream) {
    return seg_pool<SEG_MIN, false>(inp, offsets, out, nullptr, n_rows, n_seg, c, stream);
}

int doda_pg_sec_max(const float *inp, const int32_t *offsets, float *out, int32_t n_rows, int32_t n_seg, int32_t c,
                    doda_stream_t stream) {
    return seg_pool<SEG_MAX, false>(inp, offsets, out, nullptr, n_rows, n_seg, c, stream);
}

int doda_pg_roipool_fp(const float *feats, const int32_t *offsets, float *out, int32_t *maxidx, int32_t n_rows, int32_t n_seg,
                       int32_t c, doda_stream_t stream) {
    return seg_pool<SEG_MAX, true>(feats, offsets, out, maxidx, n_rows, n_seg, c, stream);
}

int doda_pg_sec_mean_bp(float *d_inp, const int32_t *offsets, const float *d_out, int32_t n_rows, int32_t n_seg, int32_t c,
                        doda_stream_t stream) {
    bool nothing;
    const int st = seg_args_status(d_inp, offsets, d_out, nullptr, false, n_rows, n_seg, c, &nothing);
    if (st != DODA_OK || nothing || n_rows == 0) return st;
    const int cl = seg_channel_lanes(c);
    if (seg_long(n_rows, n_seg))
        pg_sec_mean_bp<1024><<<seg_grid(n_seg), 1024, 0, as_stream(stream)>>>(d_inp, offsets, d_out, n_rows, n_seg, c, cl);
    else
        pg_sec_mean_bp<PG_BLOCK><<<seg_grid(n_seg), PG_BLOCK, 0, as_stream(stream)>>>(d_inp, offsets, d_out, n_rows, n_seg, c, cl);
    return doda_check_launch();
}

int doda_pg_roipool_bp(float *d_feats, const int32_t *maxidx, const float *d_out, int32_t n_rows, int32_t n_seg, int32_t c,
                       doda_stream_t stream) {
    bool nothing;
    const int st = seg_args_status(d_feats, maxidx, d_out, nullptr, false, n_rows, n_seg, c, &nothing);
    if (st != DODA_OK || nothing || n_rows == 0) return st;
    const long long total = (long long)n_seg * c;
    if (total > (long long)INT32_MAX * PG_BLOCK) return DODA_ERR_INVALID;
    pg_roipool_bp<<<div_up(total, PG_BLOCK), PG_BLOCK, 0, as_stream(stream)>>>(d_feats, maxidx, d_out, n_rows, total, c);
    return doda_check_launch();
}

size_t doda_pg_get_iou_workspace_bytes(int32_t n_proposal, int32_t n_instance) {
    if (n_proposal <= 0 || n_instance <= DODA_PG_IOU_LDS_INSTANCES) return 0;
    return (size_t)n_proposal * (size_t)n_instance * sizeof(int32_t);
}

int doda_pg_get_iou(const int32_t *proposals_idx, const int32_t *proposals_offset, const int64_t *instance_labels,
                    const int32_t *instance_pointnum, float *iou, int32_t n_points, int32_t sum_npoint, int32_t n_instance,
                    int32_t n_proposal, void *ws, size_t ws_bytes, doda_stream_t stream) {
    if (n_points < 0 || sum_npoint < 0 || n_instance < 0 || n_proposal < 0) return DODA_ERR_INVALID;
    if (n_proposal == 0 || n_instance == 0) return DODA_OK;
    if (!proposals_offset || !instance_pointnum || !iou || (sum_npoint > 0 && !proposals_idx) || (n_points > 0 && !instance_labels))
        return DODA_ERR_INVALID;
    const size_t need = doda_pg_get_iou_workspace_bytes(n_proposal, n_instance);
    if (need > 0) {
        if (!ws || ((uintptr_t)ws & 3)) return DODA_ERR_INVALID;
        if (ws_bytes < need) return DODA_ERR_WORKSPACE;
    }
    const long long *labels = reinterpret_cast<const long long *>(instance_labels);
    if (need == 0)
        pg_get_iou<true><<<n_proposal, PG_BLOCK, (size_t)n_instance * sizeof(int), as_stream(stream)>>>(
            proposals_idx, proposals_offset, labels, instance_pointnum, iou, n_points, sum_npoint, n_instance, nullptr);
    else
        pg_get_iou<false><<<n_proposal, PG_BLOCK, 0, as_stream(stream)>>>(
            proposals_idx, proposals_offset, labels, instance_pointnum, iou, n_points, sum_npoint, n_instance, static_cast<int *>(ws));
    return doda_check_launch();
}

}  // extern "C"

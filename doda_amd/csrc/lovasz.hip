// Lovasz-softmax loss fused with the Linear head at voxel level (include/doda_loss.h: doda_lovasz_fwd / _bwd).
//
// reference model/unet.py:109-111 -> util/lovasz_loss.py lovasz_softmax(softmax(scores), labels, ignore): per class a sort of all valid
// POINTS by |fg - p| and a dozen element-wise kernels over the [points, classes] matrix.  Every point of a voxel has its voxel's
// probabilities, so a class sees at most two distinct errors per voxel (p for the voxel's valid points of another label, 1 - p
// for those labelled with the class), and the Lovasz gradient of a run of tied errors telescopes to J(after) - J(before):
// loss and gradient are those of a weighted sort over 2 m items per class.
//   items    one thread per voxel: logits / softmax in registers (hd_logits: the head's bits), pred, the point counts; per class the
//            two keys 0x3f800000 - bits(error) (ascending key = descending error, below 2^30) and the two 16-bit weights
//   sort     per class, LSD radix, 3 passes x 10 bits, stable: a wave owns a tile of LV_WTILE consecutive items and a private
//            1024-counter LDS table (no workgroup barrier); histogram per (class, digit, tile) -> ONE exclusive scan over the whole
//            array (every class has exactly 2 m items, so the scan's value is the absolute output slot) -> scatter, the rank inside
//            a 64-item chunk from ten ballots (lanes with the same digit, in lane order = item order)
//   scan     per class in sorted order: integer prefix sums of the fg / bg weights (per-tile sums, one wave per class over the tiles,
//            per-tile rescan), J in fp64 before and after each item, g = J_after - J_before written to gitem[voxel, class, bg | fg];
//            the tile's sum error * g in fp64 (fixed tree), the class sums and the mean over the present classes by one workgroup
//   backward one thread per voxel: softmax recomputed, dp = (g_bg - g_fg) / n_present, dz = p (dp - <p, dp>), d_feats = dz W, the
//            per-workgroup column sums of dz (db); dz stored element by element (rows of an odd class count are not pair-aligned).
//            bf16: dz_lo = bf16(dz - bf16(dz)) next to it, a second operand for the head's weight-gradient kernel — rounding dz once
//            leaves dW up to 2^-8 off where few voxels carry it
// Zero-weight items stay in the lists: J does not move across them, so they get g = 0 — which the backward sweep reads, no memset.
#include "common.hpp"
#include "spconv_common.hpp"
#include "head_common.hpp"
#include "../../include/doda_loss.h"

namespace {
constexpr int LV_BLOCK = 256;
static_assert(LV_BLOCK == HD_BLOCK, "the items / backward sweeps use the head's workgroup: its dispatch, LDS columns and column sums");
constexpr int LV_WAVES = LV_BLOCK / 64;
constexpr int LV_BITS = 10, LV_BINS = 1 << LV_BITS, LV_PASSES = 3;   // 30 key bits
constexpr int LV_WTILE = 4096;          // sort: items of one class per wave
constexpr int LV_BATCH = 4;             // sort: 64-item chunks loaded ahead of their ranking
constexpr int LV_SITEMS = 8, LV_STILE = LV_BLOCK * LV_SITEMS;   // scan: consecutive items per thread / per workgroup
constexpr unsigned LV_ONE = 0x3f800000u;

__device__ __forceinline__ unsigned lv_key(float err) {      // ascending key = descending error; NaN -> error 0
    return LV_ONE - __float_as_uint(fminf(fmaxf(err, 0.f), 1.f));
}
__device__ __forceinline__ float lv_err(unsigned key) { return __uint_as_float(LV_ONE - key); }
__device__ __forceinline__ void lv_wave_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }   // wave-private LDS: in order after the wait

// ---- items ----------------------------------------------------------------------------------------------------------------------
// keys [n_cls][2 m], wt [n_cls][2 m]: item 2 v = the voxel's bg item (error p, weight nvalid - nfg), 2 v + 1 = its fg item (1 - p, nfg)
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(LV_BLOCK) void lovasz_items(const void *__restrict__ feats, int m, const float *__restrict__ weight,
                                                         const float *__restrict__ bias, int n_cls, const int32_t *__restrict__ v2p,
                                                         int v2p_ld, const long long *__restrict__ labels, long long ignore_index,
                                                         unsigned *__restrict__ keys, unsigned short *__restrict__ wt,
                                                         int32_t *__restrict__ pred) {
    __shared__ float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);
    const size_t seg = 2 * (size_t)m;
#pragma unroll 1
    for (long long v = (long long)blockIdx.x * LV_BLOCK + threadIdx.x; v < m; v += (long long)gridDim.x * LV_BLOCK) {
        asm volatile("" ::: "memory");      // (the staged weights stay in LDS, as in head_ce_fwd)
        float f[C], z[NK], mx;
        int arg;
        hd_load_row<ESZ, C>(feats, v, f);
        const int32_t *row = v2p + v * v2p_ld;
        const int np = row[0];
        hd_logits<C, NK>(w, b, n_cls, f, z, mx, arg);
        if (pred) pred[v] = arg;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) { z[k] = expf(z[k] - mx); s += z[k]; }      // (padding classes: exp(-inf) = 0)
        int nfg[NK], nvalid = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) nfg[k] = 0;
#pragma unroll 1
        for (int i = 0; i < np; ++i) {
            const long long lab = labels[row[1 + i]];
            if (lab != ignore_index && lab >= 0 && lab < n_cls) {
                ++nvalid;
#pragma unroll
                for (int k = 0; k < NK; ++k) nfg[k] += (int)lab == k ? 1 : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (k < n_cls) {
                const float p = fminf(z[k] / s, 1.f);
                const size_t at = (size_t)k * seg + 2 * (size_t)v;
                *reinterpret_cast<u32x2 *>(keys + at) = (u32x2){lv_key(p), lv_key(1.f - p)};
                *reinterpret_cast<unsigned *>(wt + at) = (unsigned)(nvalid - nfg[k]) | ((unsigned)nfg[k] << 16);
            }
        }
    }
}

// ---- sort -----------------------------------------------------------------------------------------------------------------------
// wave tile wt_id = class * tiles + tile: items [tile * LV_WTILE, min(seg, (tile + 1) * LV_WTILE)) of the class's segment
__global__ __launch_bounds__(LV_BLOCK) void lovasz_sort_hist(const unsigned *__restrict__ keys, long long seg, int tiles, int n_wt,
                                                             int shift, int32_t *__restrict__ hist) {
    __shared__ int cnt[LV_WAVES][LV_BINS];
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const int wt_id = blockIdx.x * LV_WAVES + wid;
    if (wt_id >= n_wt) return;              // (no workgroup barrier below: every table is its wave's own)
    const int c = wt_id / tiles, t = wt_id % tiles;
    for (int d = lane; d < LV_BINS; d += 64) cnt[wid][d] = 0;
    lv_wave_fence();
    const long long lo = (long long)t * LV_WTILE, hi = lo + LV_WTILE < seg ? lo + LV_WTILE : seg;
    const unsigned *kc = keys + (size_t)c * seg;
#pragma unroll 4
    for (long long i = lo + lane; i < hi; i += 64) atomicAdd(&cnt[wid][(kc[i] >> shift) & (LV_BINS - 1)], 1);
    lv_wave_fence();
    for (int d = lane; d < LV_BINS; d += 64) hist[((size_t)c * LV_BINS + d) * tiles + t] = cnt[wid][d];
}

// offs = the exclusive scan of hist over [class][digit][tile]: the output slot of the tile's first item with that digit.
// FIRST: the pass that attaches the item numbers (vals_in unused: item = its position in the class's segment)
template <bool FIRST>
__global__ __launch_bounds__(LV_BLOCK) void lovasz_sort_scatter(const unsigned *__restrict__ keys_in, const unsigned *__restrict__ vals_in,
                                                                long long seg, int tiles, int n_wt, int shift,
                                                                const int32_t *__restrict__ offs, long long total,
                                                                unsigned *__restrict__ keys_out, unsigned *__restrict__ vals_out) {
    __shared__ int off[LV_WAVES][LV_BINS];
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const int wt_id = blockIdx.x * LV_WAVES + wid;
    if (wt_id >= n_wt) return;
    const int c = wt_id / tiles, t = wt_id % tiles;
    for (int d = lane; d < LV_BINS; d += 64) off[wid][d] = offs[((size_t)c * LV_BINS + d) * tiles + t];
    lv_wave_fence();
    const long long lo = (long long)t * LV_WTILE, hi = lo + LV_WTILE < seg ? lo + LV_WTILE : seg;
    const unsigned *kc = keys_in + (size_t)c * seg;
    const unsigned *vc = FIRST ? nullptr : vals_in + (size_t)c * seg;
#pragma unroll 1
    for (long long i0 = lo; i0 < hi; i0 += 64 * LV_BATCH) {      // (wave-uniform bounds: every lane takes part in the ballots)
        unsigned key[LV_BATCH], val[LV_BATCH];
#pragma unroll
        for (int u = 0; u < LV_BATCH; ++u) {
            const long long i = i0 + u * 64 + lane;
            const bool ok = i < hi;
            key[u] = ok ? kc[i] : 0u;
            val[u] = FIRST ? (unsigned)i : (ok ? vc[i] : 0u);
        }
#pragma unroll
        for (int u = 0; u < LV_BATCH; ++u) {
            const bool ok = i0 + u * 64 + lane < hi;
            const int d = (int)((key[u] >> shift) & (LV_BINS - 1));
            unsigned long long peers = __ballot(ok);             // the chunk's lanes with this lane's digit
#pragma unroll
            for (int bit = 0; bit < LV_BITS; ++bit) {
                const bool on = (d >> bit) & 1;
                const unsigned long long mk = __ballot(on);
                peers &= on ? mk : ~mk;
            }
            const int rank = mask_rank(peers), npeers = __popcll(peers);
            int base = 0;
            if (ok) base = off[wid][d];
            lv_wave_fence();                                     // every peer has read the slot before its first lane advances it
            if (ok && rank == 0) off[wid][d] = base + npeers;
            lv_wave_fence();
            const long long at = (long long)base + rank;
            if (ok && at >= 0 && at < total) {
                keys_out[at] = key[u];
                vals_out[at] = val[u];
            }
        }
    }
}

// ---- scan -----------------------------------------------------------------------------------------------------------------------
// sum of (a, b) over the workgroup in a fixed tree; valid in every thread
template <typename T>
__device__ __forceinline__ void lv_block_sum2(T &a, T &b, T (*red)[LV_WAVES]) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    doda_sync();                                  // (red may still be read from the previous use)
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    doda_sync();
    a = red[0][0]; b = red[1][0];
#pragma unroll
    for (int q = 1; q < LV_WAVES; ++q) { a += red[0][q]; b += red[1][q]; }
}

// scan tile = class * stiles + tile; a thread's LV_SITEMS consecutive sorted items: (fg weight, bg weight) of each
__device__ __forceinline__ void lv_load_items(const unsigned *__restrict__ vals, const unsigned short *__restrict__ wt, long long seg,
                                              int c, long long first, unsigned (&val)[LV_SITEMS], int (&wgt)[LV_SITEMS]) {
    const unsigned *vc = vals + (size_t)c * seg;
    const unsigned short *wc = wt + (size_t)c * seg;
#pragma unroll
    for (int j = 0; j < LV_SITEMS; ++j) {
        const bool ok = first + j < seg;
        val[j] = ok ? vc[first + j] : 0u;
        wgt[j] = (ok && (long long)val[j] < seg) ? (int)wc[val[j]] : 0;
    }
}

__global__ __launch_bounds__(LV_BLOCK) void lovasz_tile_sums(const unsigned *__restrict__ vals, const unsigned short *__restrict__ wt,
                                                             long long seg, int stiles, int32_t *__restrict__ tsum) {
    __shared__ int red[2][LV_WAVES];
    const int c = blockIdx.x / stiles, t = blockIdx.x % stiles;
    unsigned val[LV_SITEMS];
    int wgt[LV_SITEMS];
    lv_load_items(vals, wt, seg, c, (long long)t * LV_STILE + threadIdx.x * LV_SITEMS, val, wgt);
    int fg = 0, bg = 0;
#pragma unroll
    for (int j = 0; j < LV_SITEMS; ++j) { fg += (val[j] & 1u) ? wgt[j] : 0; bg += (val[j] & 1u) ? 0 : wgt[j]; }
    lv_block_sum2(fg, bg, red);
    if (threadIdx.x == 0) { tsum[2 * blockIdx.x] = fg; tsum[2 * blockIdx.x + 1] = bg; }
}

// one wave per class: exclusive prefix of the tile sums, the class totals tot[c] = (G, valid points of another label)
__global__ __launch_bounds__(64) void lovasz_tile_scan(const int32_t *__restrict__ tsum, int stiles, int32_t *__restrict__ tpre,
                                                       int32_t *__restrict__ tot) {
    const int c = blockIdx.x, lane = lane_id();
    int cf = 0, cb = 0;
    for (int t0 = 0; t0 < stiles; t0 += 64) {
        const int t = t0 + lane;
        const int f = t < stiles ? tsum[2 * ((size_t)c * stiles + t)] : 0, g = t < stiles ? tsum[2 * ((size_t)c * stiles + t) + 1] : 0;
        const int fi = wave_inclusive_sum(f), gi = wave_inclusive_sum(g);
        if (t < stiles) { tpre[2 * ((size_t)c * stiles + t)] = cf + fi - f; tpre[2 * ((size_t)c * stiles + t) + 1] = cb + gi - g; }
        cf += __shfl(fi, 63, 64);
        cb += __shfl(gi, 63, 64);
    }
    if (lane == 0) { tot[2 * c] = cf; tot[2 * c + 1] = cb; }
}

__device__ __forceinline__ double lv_jaccard(int G, int cumfg, int cumbg) {      // 1 - |intersection| / |union| after the prefix
    return 1.0 - (double)(G - cumfg) / (double)(G + cumbg);
}

__global__ __launch_bounds__(LV_BLOCK) void lovasz_grad(const unsigned *__restrict__ keys, const unsigned *__restrict__ vals,
                                                        const unsigned short *__restrict__ wt, long long seg, int stiles, int n_cls,
                                                        const int32_t *__restrict__ tpre, const int32_t *__restrict__ tot,
                                                        float *__restrict__ gitem, double *__restrict__ tloss) {
    __shared__ int wsum[2][LV_WAVES];
    __shared__ double dred[2][LV_WAVES];
    const int c = blockIdx.x / stiles, t = blockIdx.x % stiles;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    const long long first = (long long)t * LV_STILE + threadIdx.x * LV_SITEMS;
    unsigned val[LV_SITEMS];
    int wgt[LV_SITEMS];
    lv_load_items(vals, wt, seg, c, first, val, wgt);
    int fg = 0, bg = 0;
#pragma unroll
    for (int j = 0; j < LV_SITEMS; ++j) { fg += (val[j] & 1u) ? wgt[j] : 0; bg += (val[j] & 1u) ? 0 : wgt[j]; }
    // exclusive prefix of the threads' sums across the workgroup, on top of the tile's
    const int fi = wave_inclusive_sum(fg), bi = wave_inclusive_sum(bg);
    if (lane == 63) { wsum[0][wid] = fi; wsum[1][wid] = bi; }
    doda_sync();
    int cf = tpre[2 * blockIdx.x] + fi - fg, cb = tpre[2 * blockIdx.x + 1] + bi - bg;
#pragma unroll
    for (int q = 0; q < LV_WAVES; ++q)
        if (q < wid) { cf += wsum[0][q]; cb += wsum[1][q]; }
    const int G = tot[2 * c];
    double loss = 0.0, unused = 0.0;
    if (G > 0) {
        const unsigned *kc = keys + (size_t)c * seg;
        double jb = lv_jaccard(G, cf, cb);
#pragma unroll
        for (int j = 0; j < LV_SITEMS; ++j) {
            if (first + j < seg) {
                if (val[j] & 1u) cf += wgt[j]; else cb += wgt[j];
                const double ja = lv_jaccard(G, cf, cb);
                const double g = ja - jb;
                jb = ja;
                loss += (double)lv_err(kc[first + j]) * g;
                if (gitem && (long long)val[j] < seg) gitem[((size_t)(val[j] >> 1) * n_cls + c) * 2 + (val[j] & 1u)] = (float)g;
            }
        }
    } else if (gitem) {         // an absent class: left out of the mean, no gradient
#pragma unroll
        for (int j = 0; j < LV_SITEMS; ++j)
            if (first + j < seg && (long long)val[j] < seg) gitem[((size_t)(val[j] >> 1) * n_cls + c) * 2 + (val[j] & 1u)] = 0.f;
    }
    lv_block_sum2(loss, unused, dred);
    if (threadIdx.x == 0) tloss[blockIdx.x] = loss;
}

// out[0] = mean over the present classes of their tile sums (fixed order, fp64), out[1] = the number of present classes
__global__ __launch_bounds__(1024) void lovasz_final(const double *__restrict__ tloss, const int32_t *__restrict__ tot, int stiles,
                                                     int n_cls, float *__restrict__ out) {
    __shared__ double closs[DODA_LOVASZ_MAX_CLASSES];
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    for (int c = wid; c < n_cls; c += 16) {
        double a = 0.0;
        for (int t = lane; t < stiles; t += 64) a += tloss[(size_t)c * stiles + t];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d, 64);
        if (lane == 0) closs[c] = a;
    }
    doda_sync();
    if (threadIdx.x == 0) {
        double a = 0.0;
        int present = 0;
        for (int c = 0; c < n_cls; ++c)
            if (tot[2 * c] > 0) { a += closs[c]; ++present; }
        out[0] = present > 0 ? (float)(a / present) : 0.f;
        out[1] = (float)present;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// The per-class values of a thread's voxel live in its LDS column, as in head_ce_bwd (head_common.hpp).
template <int ESZ, int C, int NK>
__global__ __launch_bounds__(LV_BLOCK) void lovasz_bwd(const void *__restrict__ feats, int m, const float *__restrict__ weight,
                                                       const float *__restrict__ bias, int n_cls, const float *__restrict__ gitem,
                                                       const float *__restrict__ out, const float *__restrict__ grad,
                                                       void *__restrict__ d_feats, void *__restrict__ dz_out, void *__restrict__ dz_lo_out,
                                                       float *__restrict__ db_partial) {
    __shared__ __attribute__((aligned(16))) float w[HD_MAX_K][HD_MAX_C], b[HD_MAX_K];
    __shared__ float sz[NK][LV_BLOCK];
    hd_stage_weights<ESZ>(weight, bias, n_cls, C, w, b);
    const float scale = out[1] > 0.f ? grad[0] / out[1] : 0.f;
    const int tid = threadIdx.x;
    const long long v = (long long)blockIdx.x * LV_BLOCK + tid;
#pragma unroll 1
    for (int k = 0; k < NK; ++k) sz[k][tid] = 0.f;      // (a thread past the last voxel contributes zeros to hd_db_colsums)
    if (v < m) {
        float f[C];
        hd_load_row<ESZ, C>(feats, v, f);
        const float mx = hd_logits_lds<C>(w, b, n_cls, f, sz, tid);
        float s = 0.f;
#pragma unroll 2
        for (int k = 0; k < n_cls; ++k) {
            const float e = expf(sz[k][tid] - mx);
            sz[k][tid] = e;
            s += e;
        }
        const float *gr = gitem + (size_t)v * n_cls * 2;
        float dot = 0.f;
#pragma unroll 2
        for (int k = 0; k < n_cls; ++k) {
            const float p = fminf(sz[k][tid] / s, 1.f);
            sz[k][tid] = p;
            dot += p * ((gr[2 * k] - gr[2 * k + 1]) * scale);
        }
        float df[C];
#pragma unroll
        for (int c = 0; c < C; ++c) df[c] = 0.f;
        char *dzr = (char *)dz_out + (size_t)v * n_cls * ESZ;
#pragma unroll 1
        for (int k = 0; k < n_cls; ++k) {
            const float g = sz[k][tid] * ((gr[2 * k] - gr[2 * k + 1]) * scale - dot);
            sz[k][tid] = g;
#pragma unroll
            for (int c = 0; c < C; ++c) df[c] = __builtin_fmaf(g, w[k][c], df[c]);
            HdRow<ESZ>::store(dzr + (size_t)k * ESZ, g);
            if constexpr (ESZ == 2) {      // what the bf16 rounding of dz dropped, itself in bf16 (exact difference, rounded once)
                if (dz_lo_out) {
                    char *lo = (char *)dz_lo_out + ((size_t)v * n_cls + k) * ESZ;
                    HdRow<ESZ>::store(lo, g - HdRow<ESZ>::load(dzr + (size_t)k * ESZ));
                }
            }
        }
        hd_store_dfeats<ESZ, C>(d_feats, v, df);
    }
    hd_db_colsums(sz, n_cls, db_partial);
}

// the workspace, cut into 256-byte aligned pieces
struct LvPlan {
    long long seg, total;          // items per class (2 m), items in all
    int tiles, n_wt, stiles, n_st; // sort tiles per class / in all (one wave each), scan tiles per class / in all (one workgroup each)
    int hist_len;
    size_t keys[2], vals[2], wt, hist, offs, scan_ws, tsum, tpre, tot, tloss, bytes;
};
inline bool lv_plan(int m, int n_cls, LvPlan *p) {
    if (m < 1 || n_cls < 2 || n_cls > DODA_LOVASZ_MAX_CLASSES) return false;
    p->seg = 2 * (long long)m;
    p->total = p->seg * n_cls;
    if (p->total >= (1ll << 31)) return false;      // (slots and their scan are int32)
    p->tiles = div_up(p->seg, LV_WTILE);
    p->n_wt = p->tiles * n_cls;
    p->stiles = div_up(p->seg, LV_STILE);
    p->n_st = p->stiles * n_cls;
    const long long hl = (long long)p->n_wt * LV_BINS;
    if (hl >= (1ll << 31)) return false;
    p->hist_len = (int)hl;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
    for (int q = 0; q < 2; ++q) { p->keys[q] = take((size_t)p->total * 4); p->vals[q] = take((size_t)p->total * 4); }
    p->wt = take((size_t)p->total * 2);
    p->hist = take((size_t)p->hist_len * 4);
    p->offs = take((size_t)p->hist_len * 4);
    p->scan_ws = take(scan_ws_ints(p->hist_len) * 4);
    p->tsum = take((size_t)p->n_st * 8);
    p->tpre = take((size_t)p->n_st * 8);
    p->tot = take((size_t)DODA_LOVASZ_MAX_CLASSES * 8);
    p->tloss = take((size_t)p->n_st * 8);
    p->bytes = at;
    return true;
}
}  // namespace

extern "C" int32_t doda_loss_abi_version(void) { return DODA_LOSS_ABI_VERSION; }

extern "C" size_t doda_lovasz_workspace_bytes(int32_t m, int32_t n_cls) {
    LvPlan p;
    return lv_plan(m > 0 ? m : 1, n_cls, &p) ? p.bytes : 0;
}

extern "C" int32_t doda_lovasz_blocks(int32_t m) { return hd_blocks(m > 0 ? m : 1); }

extern "C" int doda_lovasz_fwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                               int32_t n_cls, const int32_t *v2p, int32_t v2p_ld, const int64_t *labels, int64_t ignore_index,
                               float *out, int32_t *pred, float *gitem, void *ws, size_t ws_bytes, doda_stream_t stream) {
    if (!out || m < 0) return DODA_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (m == 0) { (void)hipMemsetAsync(out, 0, 8, s); return DODA_OK; }
    if (hd_args_bad(m, elem_bytes, v2p_ld, {feats, weight, v2p, labels, ws}) || ((uintptr_t)ws & 255) || ((uintptr_t)feats & 15))
        return DODA_ERR_INVALID;
    if (c != 16 || n_cls < 2 || n_cls > DODA_LOVASZ_MAX_CLASSES || v2p_ld - 1 > DODA_LOVASZ_MAX_POINTS_PER_VOXEL) return DODA_ERR_UNSUPPORTED;
    LvPlan p;
    if (!lv_plan(m, n_cls, &p)) return DODA_ERR_UNSUPPORTED;
    if (ws_bytes < p.bytes) return DODA_ERR_WORKSPACE;
    char *base = (char *)ws;
    unsigned *keys[2] = {(unsigned *)(base + p.keys[0]), (unsigned *)(base + p.keys[1])};
    unsigned *vals[2] = {(unsigned *)(base + p.vals[0]), (unsigned *)(base + p.vals[1])};
    unsigned short *wt = (unsigned short *)(base + p.wt);
    int32_t *hist = (int32_t *)(base + p.hist), *offs = (int32_t *)(base + p.offs), *scan_ws = (int32_t *)(base + p.scan_ws);
    int32_t *tsum = (int32_t *)(base + p.tsum), *tpre = (int32_t *)(base + p.tpre), *tot = (int32_t *)(base + p.tot);
    double *tloss = (double *)(base + p.tloss);

    HD_DISPATCH(lovasz_items, 16, hd_blocks(m), feats, m, weight, bias, n_cls, v2p, v2p_ld, (const long long *)labels, (long long)ignore_index,
                keys[0], wt, pred);
    const int sort_grid = div_up(p.n_wt, LV_WAVES);
    int cur = 0;
    for (int pass = 0; pass < LV_PASSES; ++pass, cur ^= 1) {
        const int shift = pass * LV_BITS;
        hipLaunchKernelGGL(lovasz_sort_hist, dim3(sort_grid), dim3(LV_BLOCK), 0, s, (const unsigned *)keys[cur], p.seg, p.tiles, p.n_wt,
                           shift, hist);
        const int st = exclusive_scan_i32(hist, offs, p.hist_len, nullptr, scan_ws, s);
        if (st != DODA_OK) return st;
        if (pass == 0)
            hipLaunchKernelGGL(lovasz_sort_scatter<true>, dim3(sort_grid), dim3(LV_BLOCK), 0, s, (const unsigned *)keys[cur],
                               (const unsigned *)nullptr, p.seg, p.tiles, p.n_wt, shift, (const int32_t *)offs, p.total, keys[cur ^ 1],
                               vals[cur ^ 1]);
        else
            hipLaunchKernelGGL(lovasz_sort_scatter<false>, dim3(sort_grid), dim3(LV_BLOCK), 0, s, (const unsigned *)keys[cur],
                               (const unsigned *)vals[cur], p.seg, p.tiles, p.n_wt, shift, (const int32_t *)offs, p.total, keys[cur ^ 1],
                               vals[cur ^ 1]);
    }
    hipLaunchKernelGGL(lovasz_tile_sums, dim3(p.n_st), dim3(LV_BLOCK), 0, s, (const unsigned *)vals[cur], (const unsigned short *)wt, p.seg,
                       p.stiles, tsum);
    hipLaunchKernelGGL(lovasz_tile_scan, dim3(n_cls), dim3(64), 0, s, (const int32_t *)tsum, p.stiles, tpre, tot);
    hipLaunchKernelGGL(lovasz_grad, dim3(p.n_st), dim3(LV_BLOCK), 0, s, (const unsigned *)keys[cur], (const unsigned *)vals[cur],
                       (const unsigned short *)wt, p.seg, p.stiles, n_cls, (const int32_t *)tpre, (const int32_t *)tot, gitem, tloss);
    hipLaunchKernelGGL(lovasz_final, dim3(1), dim3(1024), 0, s, (const double *)tloss, (const int32_t *)tot, p.stiles, n_cls, out);
    return doda_check_launch();
}

extern "C" int doda_lovasz_bwd(const void *feats, int32_t m, int32_t c, int32_t elem_bytes, const float *weight, const float *bias,
                               int32_t n_cls, const float *gitem, const float *out, const float *grad, void *d_feats, void *dz,
                               void *dz_lo, float *db_partial, int32_t n_blocks, doda_stream_t stream) {
    if (m < 0) return DODA_ERR_INVALID;
    if (m == 0) return DODA_OK;
    if (hd_args_bad(m, elem_bytes, 1, {feats, weight, gitem, out, grad, d_feats, dz, db_partial}) || ((uintptr_t)feats & 15) ||
        ((uintptr_t)d_feats & 15))
        return DODA_ERR_INVALID;
    if (c != 16 || n_cls < 2 || n_cls > DODA_LOVASZ_MAX_CLASSES) return DODA_ERR_UNSUPPORTED;
    if (n_blocks != doda_lovasz_blocks(m)) return DODA_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    HD_DISPATCH(lovasz_bwd, 16, n_blocks, feats, m, weight, bias, n_cls, gitem, out, grad, d_feats, dz, elem_bytes == 2 ? dz_lo : nullptr,
                db_partial);
    return doda_check_launch();
}

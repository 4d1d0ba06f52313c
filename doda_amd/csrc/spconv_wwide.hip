// wgrad_wide: weight gradient of the bf16 SubM K = 27 layers of 48 .. 224 channels over the rulebook's TILEBOOK
//     dw[o][ci][co] (+)= sum_t x[tbl[o][t]][ci] * dy[t][co]
// (spconv v1.2 indice_conv_backward's per-offset `Xg^T . dYg`), for every such layer of a doda_spconv_wgrad_multi call in
// one launch.
//
// The gather-table kernel (spconv_wgrad.hip) issues one global gather per (row, offset) slot: at level 3 it pulls
// 27 x 37 k rows x 96 B per layer out of L2 for ~20 MB of operands (coarse-level weight gradients).  Here a
// workgroup owns a (layer, input-channel slice, output-channel slice) and a range of 256-row tiles.  Per tile it stages
// ONCE in LDS its input-channel slice of the tile's distinct x rows (the tilebook's list), its output-channel slice of the
// 256 dy rows and the tile's ten planes of local indices, then serves all 27 offsets from there.  Both operands reach MFMA
// k-order through ds_read_b64_tr_b16 (as in wgrad_dma16): dy with dense addresses, x with per-lane addresses built from the
// local indices.  Slices are as wide as the register file allows: 16 waves, each holding the accumulators of two offsets
// for the whole slice (TA x TB 16 x 16 blocks, TA * TB <= 9: 72 accumulator floats per lane), so a gathered fragment feeds
// TB MFMAs and a dy fragment 2 TA.
// A tile whose list was not kept (more than TB_LMAX distinct rows) is served offset by offset: the 256 rows of one offset
// are gathered through the dense table into the row slots 1 .. 256 and the waves that own the offset multiply them.
// Same sums as the gather-table kernel, bit for bit: a workgroup's rows are one ROW CHUNK of that kernel's plan for the
// layer (make_plan: multiples of 64 rows, so a chunk starts and ends on a 32-row k-step of a tile), its k-steps run in
// ascending row order into the same v_mfma_f32_16x16x32_bf16 chains with the same operands (absent rows are zeros in both;
// an all-zero step adds +0 to an accumulator that started at +0), and wgrad_wide_reduce adds a slice's chunk partials with
// the fold wgrad_reduce_multi uses (wgrad_common.hpp wgrad_fold).  Switching a layer between the two kernels changes no bit
// of its dW.
#include "wgrad_common.hpp"
#include "tilebook.hpp"
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int WW_WAVES = 16;
constexpr int WW_MO = (TB_K + WW_WAVES - 1) / WW_WAVES;       // offsets per wave (2)
constexpr int WW_LIST_BYTES = TB_UMAX * 4;
// dy slice (TB_T rows of 32 TB bytes) and behind it the x rows (slot 0 = the zero row, then up to TB_LMAX rows of 32 TA
// bytes): at most 3 x 3 blocks -> 24 + 96 KB
constexpr int ww_stage_bytes(int ta, int tb) { return TB_T * 32 * tb + (TB_LMAX + 1) * 32 * ta; }
constexpr int WW_STAGE_MAX = ww_stage_bytes(3, 3);
constexpr int WW_SMEM = WW_LIST_BYTES + TB_LIDX_BYTES + WW_STAGE_MAX;
static_assert(WW_SMEM <= 160 * 1024, "one workgroup per CU");
static_assert(TB_T + 1 <= TB_LMAX + 1, "the dense fallback stages 256 rows into the row slots");

// one layer of the launch (also the reduce's descriptor)
struct WwJob {
    const unsigned short *x, *dy;
    const int32_t *tbl;
    const void *tb;
    float *dw, *part;          // part: [n_sa * n_sb][P][27 * 16 TA * 16 TB]
    int ca, cb, ld, n_rows, nt, ta, tb_, n_sb, P, rpc, accumulate;   // P row chunks of rpc rows
    int wg_end, red_end;       // inclusive prefixes of the launch's workgroups / the reduce's blocks
    int pad;
};

__device__ __forceinline__ s16x4 ww_tr(unsigned addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(uintptr_t)addr);
}
__device__ __forceinline__ bf16x8 ww_frag(unsigned a_lo, unsigned a_hi) {
    const s16x4 lo = ww_tr(a_lo), hi = ww_tr(a_hi);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int TA, int TB>
__device__ void ww_body(const WwJob &d, int local, unsigned char *smem) {
    constexpr int RA = 32 * TA, RB = 32 * TB;                  // LDS row bytes of the x / dy slices
    constexpr int CIS = 16 * TA, COS = 16 * TB, SLICE = TB_K * CIS * COS;
    const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, i = lane & 15, g = lane >> 4, q4 = i >> 2, c4 = i & 3;
    const int slice = local / d.P, p = local - slice * d.P;
    const int sa = slice / d.n_sb, sb = slice - sa * d.n_sb;
    const int ca0 = sa * CIS, cb0 = sb * COS;
    const int r_begin = p * d.rpc, r_end = min(d.n_rows, r_begin + d.rpc);        // this workgroup's row chunk
    const int tile_begin = r_begin / TB_T, tile_end = (r_end - 1) / TB_T + 1;
    static_assert(ww_stage_bytes(TA, TB) <= WW_STAGE_MAX, "staging buffers");
    // the tilebook's parts (tilebook.hpp tilebook_view)
    const int32_t *tb_ulist = (const int32_t *)d.tb;
    const uint32_t *tb_lidx = (const uint32_t *)(tb_ulist + (size_t)d.nt * TB_UMAX);
    const int32_t *tb_ucount = (const int32_t *)(tb_lidx + (size_t)d.nt * (TB_LIDX_BYTES / 4));

    int32_t *list_s = reinterpret_cast<int32_t *>(smem);
    const unsigned *lidx_s = reinterpret_cast<const unsigned *>(smem + WW_LIST_BYTES);
    unsigned char *dy_s = smem + WW_LIST_BYTES + TB_LIDX_BYTES;
    unsigned char *rows_s = dy_s + TB_T * RB;
    const unsigned dy_base = (unsigned)(uintptr_t)dy_s, rows_base = (unsigned)(uintptr_t)rows_s;

    f32x4 acc[WW_MO][TA][TB];
#pragma unroll
    for (int m = 0; m < WW_MO; ++m)
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b) acc[m][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the wave's k-step ks: B fragments (dy rows 32 ks + 8 g + 0..7, channel i of each block), then per owned offset the
    // A fragments (rows through the local indices, or slot t + 1 in the dense fallback for offset only_o)
    // (k-steps ks_begin .. ks_end - 1 of the tile: the chunk's rows)
    auto multiply = [&](bool dense, int only_o, int ks_begin, int ks_end) {
#pragma unroll 1
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            const int r = 32 * ks + 8 * g + q4;
            bf16x8 bf[TB];
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                const unsigned a0 = dy_base + (unsigned)(r * RB + b * 32 + c4 * 8);
                bf[b] = ww_frag(a0, a0 + 4u * RB);
            }
#pragma unroll
            for (int m = 0; m < WW_MO; ++m) {
                const int o = wid + WW_WAVES * m;
                if (o >= TB_K || (dense && o != only_o)) continue;      // (wave-uniform)
                unsigned s0, s1;
                if (dense) {
                    s0 = (unsigned)(r + 1);
                    s1 = (unsigned)(r + 5);
                } else {
                    const unsigned *pl = lidx_s + tb_lplane(o) * TB_T;
                    const unsigned sh = tb_lshift(o);
                    s0 = __builtin_amdgcn_ubfe(pl[tb_lpos(r)], sh, 10u);
                    s1 = __builtin_amdgcn_ubfe(pl[tb_lpos(r + 4)], sh, 10u);
                }
                const unsigned x0 = rows_base + s0 * RA + (unsigned)(c4 * 8), x1 = rows_base + s1 * RA + (unsigned)(c4 * 8);
#pragma unroll
                for (int a = 0; a < TA; ++a) {
                    const bf16x8 af = ww_frag(x0 + 32u * a, x1 + 32u * a);
#pragma unroll
                    for (int b = 0; b < TB; ++b)
                        acc[m][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[b], acc[m][a][b], 0, 0, 0);
                }
            }
        }
    };

    // zero row (slot 0)
    for (int e = tid; e < RA / 16; e += 1024) reinterpret_cast<u32x4 *>(rows_s)[e] = (u32x4){0u, 0u, 0u, 0u};
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const int t0 = tile * TB_T;
        const int ks_begin = max(0, (r_begin - t0) / 32), ks_end = min(TB_T / 32, (r_end - t0 + 31) / 32);
        const int ucount = tb_ucount[tile];
        const bool listed = ucount <= TB_LMAX;
        // ---- list, local-index planes, dy slice -> LDS ----
        if (listed) {
            // entry e is stored at tb_upos(e) (tilebook.hpp): thread tid reads position tid
            const int e = (tid & 3) * 256 + ((tid >> 7) & 7) * 32 + ((tid >> 2) & 31);
            list_s[e] = tb_ulist[(size_t)tile * TB_UMAX + tid];
            for (int v = tid; v < TB_LIDX_BYTES / 16; v += 1024)
                reinterpret_cast<u32x4 *>(smem + WW_LIST_BYTES)[v] =
                    reinterpret_cast<const u32x4 *>(tb_lidx + (size_t)tile * (TB_LIDX_BYTES / 4))[v];
        }
        for (int v = tid; v < TB_T * (RB / 16); v += 1024) {
            const int t = v / (RB / 16), f = v - t * (RB / 16);
            u32x4 val = (u32x4){0u, 0u, 0u, 0u};
            if (t0 + t < d.n_rows) val = *reinterpret_cast<const u32x4 *>(d.dy + (size_t)(t0 + t) * d.cb + cb0 + f * 8);
            *reinterpret_cast<u32x4 *>(dy_s + t * RB + f * 16) = val;
        }
        doda_sync();
        if (listed) {
            // ---- the tile's distinct x rows (input-channel slice) -> slots 1 .. ucount ----
            for (int v = tid; v < ucount * (RA / 16); v += 1024) {
                const int e = v / (RA / 16), f = v - e * (RA / 16);
                const int row = list_s[e];
                *reinterpret_cast<u32x4 *>(rows_s + (e + 1) * RA + f * 16) =
                    *reinterpret_cast<const u32x4 *>(d.x + (size_t)row * d.ca + ca0 + f * 8);
            }
            doda_sync();
            multiply(false, 0, ks_begin, ks_end);
            doda_sync();
        } else {
            // ---- no list: offset by offset through the dense table ----
            for (int o = 0; o < TB_K; ++o) {
                for (int v = tid; v < TB_T * (RA / 16); v += 1024) {
                    const int t = v / (RA / 16), f = v - t * (RA / 16);
                    const int row = t0 + t < d.n_rows ? d.tbl[(size_t)o * d.ld + t0 + t] : -1;
                    u32x4 val = (u32x4){0u, 0u, 0u, 0u};
                    if (row >= 0) val = *reinterpret_cast<const u32x4 *>(d.x + (size_t)row * d.ca + ca0 + f * 8);
                    *reinterpret_cast<u32x4 *>(rows_s + (t + 1) * RA + f * 16) = val;
                }
                doda_sync();
                multiply(true, o, ks_begin, ks_end);
                doda_sync();
            }
        }
    }

    // ---- the workgroup's partial: D[ci][co], lane (co = i, g) holds ci = 4 g + r ----
    float *dst = d.part + (size_t)local * SLICE;
#pragma unroll
    for (int m = 0; m < WW_MO; ++m) {
        const int o = wid + WW_WAVES * m;
        if (o >= TB_K) continue;
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    dst[((size_t)o * CIS + a * 16 + 4 * g + r) * COS + b * 16 + i] = acc[m][a][b][r];
    }
}

// one case per slice shape the plan can name (wgrad_plan.hpp WW_SHAPES)
__global__ __launch_bounds__(1024) void wgrad_wide(const WwJob *__restrict__ jobs, int n_jobs) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[WW_SMEM];
    const int j = find_job<WwJob, &WwJob::wg_end>(jobs, n_jobs, (int)blockIdx.x);
    const WwJob d = jobs[j];
    const int local = (int)blockIdx.x - (j == 0 ? 0 : jobs[j - 1].wg_end);
#define WW_CASE(A, B) if (d.ta == A && d.tb_ == B) { ww_body<A, B>(d, local, smem); return; }
    WW_SHAPES(WW_CASE)
#undef WW_CASE
}

// dw[o][ci][co] (+)= sum_p part[slice][p][o][ci'][co']: the shared fold over the P chunk partials of the quad's slice
__global__ __launch_bounds__(256) void wgrad_wide_reduce(const WwJob *__restrict__ jobs, int n_jobs) {
    const int j = find_job<WwJob, &WwJob::red_end>(jobs, n_jobs, (int)blockIdx.x);
    const WwJob d = jobs[j];
    const int CIS = 16 * d.ta, COS = 16 * d.tb_, SLICE = TB_K * CIS * COS;
    wgrad_fold((int)blockIdx.x - (j == 0 ? 0 : jobs[j - 1].red_end), d.P, (long long)TB_K * d.ca * d.cb / 4, SLICE / 4,
               reinterpret_cast<float4 *>(d.dw), d.accumulate, [&](long long q) {
        const long long e = 4 * q;
        const int co = (int)(e % d.cb), ci = (int)((e / d.cb) % d.ca), o = (int)(e / ((long long)d.ca * d.cb));
        const int slice = (ci / CIS) * d.n_sb + co / COS;
        return reinterpret_cast<const float4 *>(d.part + ((size_t)slice * d.P) * SLICE + ((size_t)o * CIS + ci % CIS) * COS + co % COS);
    });
}

}  // namespace

namespace doda_wwide {

// The launch's plan: jobs longest first (most rows), one workgroup per (channel slice, row chunk of the gather-table
// kernel's plan, plan_dense).  Identical inputs give an identical plan.
Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx) {
    Plan pl;
    pl.n = (int)idx.size();
    std::vector<int> order;
    for (int k = 0; k < pl.n; ++k) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return jobs[idx[a]].n_rows > jobs[idx[b]].n_rows; });
    std::vector<WwJob> desc;
    for (int kk : order) {
        const doda_wgrad_job &j = jobs[idx[kk]];
        WwJob d;
        d.x = (const unsigned short *)j.a; d.dy = (const unsigned short *)j.b; d.tbl = j.tbl; d.tb = j.tilebook;
        d.dw = j.dw;
        d.ca = j.ca; d.cb = j.cb; d.ld = j.ld; d.n_rows = j.n_rows; d.nt = (j.n_rows + TB_T - 1) / TB_T;
        const WideGeo g = wwide_geo(j, doda_wgrad::switches());
        d.ta = g.ta; d.tb_ = g.tb; d.rpc = g.rpc; d.P = g.P;
        d.n_sb = j.cb / (16 * d.tb_);
        d.accumulate = (j.flags & DODA_WGRAD_ACCUMULATE) ? 1 : 0;
        d.part = (float *)(uintptr_t)pl.partial_bytes;      // offset until write_desc()
        pl.partial_bytes += g.partial_bytes;
        pl.wgs += g.blocks;
        d.wg_end = pl.wgs;
        pl.red_blocks += doda_wgrad::reduce_blocks((long long)TB_K * j.ca * j.cb / 4, d.P);
        d.red_end = pl.red_blocks;
        d.pad = 0;
        desc.push_back(d);
    }
    pl.desc_bytes = desc.size() * sizeof(WwJob);
    pl.desc.resize(pl.desc_bytes);
    if (pl.desc_bytes) memcpy(pl.desc.data(), desc.data(), pl.desc_bytes);
    return pl;
}

size_t desc_bytes_per_job() { return sizeof(WwJob); }

void write_desc(const Plan &p, char *part, void *desc) {
    if (p.desc_bytes) memcpy(desc, p.desc.data(), p.desc_bytes);
    WwJob *d = (WwJob *)desc;
    for (int k = 0; k < p.n; ++k) d[k].part = (float *)(part + (uintptr_t)d[k].part);
}

int launch(const Plan &p, const void *desc_dev, hipStream_t s) {
    doda_wgrad::trace("wgrad_wide", p.wgs, 1024, p.n);
    hipLaunchKernelGGL(wgrad_wide, dim3(p.wgs), dim3(1024), 0, s, (const WwJob *)desc_dev, p.n);
    doda_wgrad::trace("wgrad_wide_reduce", p.red_blocks, 256, p.n);
    hipLaunchKernelGGL(wgrad_wide_reduce, dim3(p.red_blocks), dim3(256), 0, s, (const WwJob *)desc_dev, p.n);
    return doda_check_launch();
}

}  // namespace doda_wwide

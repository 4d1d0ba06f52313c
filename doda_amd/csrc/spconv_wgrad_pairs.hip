// Sparse-convolution weight gradient over PAIR LISTS:
//     dw[o][ci][co] (+)= sum_{p < n_o} a[in_o[p]][ci] * b[out_o[p]][co]
// (spconv v1.2 indice_conv_backward's per-offset `Xg^T . dYg` GEMMs over indice_pairs /
// indice_pair_num; reference call sites model/unet_block.py:26,29,48,70,78.)
//
// Why a second formulation next to spconv_wgrad.hip (dense gather table + LDS transpose):
//   * the dense table walks K * M (offset, row) slots of which ~36 % hold a pair at level 1 (and 1/8
//     for the strided convolutions); the pair lists hold the P present pairs only: 2.8x fewer gathers,
//     MFMAs and bytes, and the table (4*K*M bytes) is not read at all;
//   * the contraction runs over ROWS, so both MFMA operands need rows as their k dimension while
//     memory holds channels contiguously.  The dense kernel goes through LDS (16-byte stores +
//     ds_read_b64_tr_b16; PMC: bank conflicts 70 % of LDS-active cycles, the bound of that kernel).
//     Here the transposition is done by the matrix core itself: a gathered 16-byte row slice is the
//     natural A operand of v_mfma_f32_16x16x32_bf16 (lane = pair, registers = channels); multiplied
//     by a ONE-HOT B operand it comes back in D layout with lane = channel, registers = pairs —
//     exactly the k-order the contraction wants.  Products with 1.0 and sums with zeros are exact,
//     and the fp32 -> bf16 repack keeps the upper 16 bits of values that are bf16 already.
//     No LDS, no barriers in the loop, every wave independent.
// Per 32 pairs and 16x16 channel tile: 2 index reads (shared by two steps), 2 row gathers (16 B per
// lane), 4 transposing MFMAs, 1 contraction MFMA.  MFMA is still far from a bound.
// Deterministic: per-range partials, summed in fixed order by the call's shared reduction (wgrad_common.hpp wgrad_fold: the
// reductions join the gather-table jobs' in one wgrad_reduce_multi launch); no float atomics.
#include "wgrad_common.hpp"
#include <string.h>

namespace {

constexpr int RANGE_TILES = WP_RANGE_TILES, RANGE_ROWS = WP_RANGE_ROWS;   // a block's row range (wgrad_plan.hpp pairs_geo)
constexpr unsigned OOB = 0x80000000u;      // absent pair: beyond any buffer (operands are < 1 GB)
constexpr unsigned CH_OOB = 0x40000000u;   // channel block past the channel count (OOB + CH_OOB does not wrap)

// One layer inside a kernel-variant group.  Work item = (row range of the lists' `in` side, group of 4
// offsets, channel tile); the block's four waves take one offset each and walk that offset's pairs
// whose `in` row lies in the range: the segment [seg[o][t0], seg[o][t0 + RANGE_TILES]) of list o, read
// from the per-256-row-tile prefix the list export leaves behind.  All offsets of a row range touch the
// same neighbourhood of rows, and consecutive work items run on one XCD (xcd_work_item), so the rows
// are fetched from HBM once and served from L2 to the other offsets.  (Blocks split by OFFSET instead
// re-fetched every row into every XCD's L2: measured 63 us per level-1 layer at ~6 TB/s of fabric reads.)
struct PJob {
    const void *a, *b;
    const int32_t *pin, *pout, *pnum, *seg;   // seg: [K][seg_nt] exclusive prefix per tile, or NULL (identity lists)
    float *partial;      // [n_range][K][ca][cb]
    unsigned a_bytes, b_bytes;
    int ca, cb, ld, K, n_rows, n_range, n_og, n_tag, n_tbg, seg_nt, blk_end, pad;
};
// block -> job: the inclusive block prefixes travel in the kernel arguments (scalar cache), not in a
// dependent chain of global loads
constexpr int MAX_GROUP = 48;
struct Ends { int n; int end[MAX_GROUP]; };

__device__ __forceinline__ int find_end(const Ends &e, int blk) {
    int j = 0;
#pragma unroll 1
    for (int k = 0; k < e.n - 1; ++k) j += blk >= e.end[k] ? 1 : 0;
    return j;
}

// TA x TB 16-channel blocks of (a, b) per wave.
template <int TA, int TB>
__global__ __launch_bounds__(256) void wgrad_pairs_kernel(const PJob *__restrict__ jobs, const Ends ends) {
    const int jn = find_end(ends, (int)blockIdx.x);
    const PJob &d = jobs[jn];
    const int first = jn == 0 ? 0 : ends.end[jn - 1], n_items = ends.end[jn] - first;
    int lb = xcd_work_item((int)blockIdx.x - first, n_items);   // contiguous items per XCD
    const int tbg = lb % d.n_tbg; lb /= d.n_tbg;
    const int tag = lb % d.n_tag; lb /= d.n_tag;
    const int og = lb % d.n_og;
    const int range = lb / d.n_og;

    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int o = og * 4 + wid;
    if (o >= d.K) return;     // (no barrier in this kernel)
    // the wave's segment of list o.  readfirstlane: the values size buffer descriptors, which must be
    // provably wave-uniform (else hipcc wraps each load in a waterfall loop)
    int p_begin, p_end;
    if (d.seg) {
        const int t0 = range * RANGE_TILES, t1 = t0 + RANGE_TILES;
        const int n_o = d.pnum[o];
        p_begin = d.seg[(long long)o * d.seg_nt + t0];
        p_end = t1 < d.seg_nt ? d.seg[(long long)o * d.seg_nt + t1] : n_o;
    } else {                  // identity lists (1x1 convolution): pair p = (p, p)
        p_begin = range * RANGE_ROWS;
        p_end = p_begin + RANGE_ROWS < d.ld ? p_begin + RANGE_ROWS : d.ld;
    }
    p_begin = __builtin_amdgcn_readfirstlane(p_begin);
    p_end = __builtin_amdgcn_readfirstlane(p_end);

    // one-hot B operands: P[G][k = (g, q)][j = i] = 1 iff the lane group carries pair group G
    // (g >> 1 == G), the half-row of channel j (g & 1 == j >> 3) and q == j & 7
    bf16x8 P[2];
#pragma unroll
    for (int G = 0; G < 2; ++G) {
        u32x4 v = {0u, 0u, 0u, 0u};
        const bool mine = (g >> 1) == G && (i >> 3) == (g & 1);
        const int q = i & 7;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = (mine && (q >> 1) == w) ? ((q & 1) ? 0x3F800000u : 0x00003F80u) : 0u;
        P[G] = __builtin_bit_cast(bf16x8, v);
    }

    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void *)d.a, 0, d.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void *)d.b, 0, d.b_bytes, 0x00020000);
    const int32_t *pi = d.pin + (long long)o * d.ld, *po = d.pout + (long long)o * d.ld;
    const unsigned rb_a = (unsigned)d.ca * 2u, rb_b = (unsigned)d.cb * 2u;
    const unsigned half = (unsigned)(g & 1) * 16u;
    // channel blocks of this tile; a block past the channel count reads zeros
    unsigned ch_a[TA], ch_b[TB];
#pragma unroll
    for (int xa = 0; xa < TA; ++xa) {
        const int blk = tag * TA + xa;
        ch_a[xa] = blk * 16 < d.ca ? (unsigned)blk * 32u + half : CH_OOB;
    }
#pragma unroll
    for (int yb = 0; yb < TB; ++yb) {
        const int blk = tbg * TB + yb;
        ch_b[yb] = blk * 16 < d.cb ? (unsigned)blk * 32u + half : CH_OOB;
    }

    f32x4 acc[TA][TB];
#pragma unroll
    for (int xa = 0; xa < TA; ++xa)
#pragma unroll
        for (int yb = 0; yb < TB; ++yb) acc[xa][yb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // index registers of one double-step: lane l holds the pair p + l.  Raw buffer loads over the list
    // up to p_end: a lane past the end reads 0 and is masked when the rows are requested.  No branch
    // anywhere in the loop: with control flow inside it hipcc falls back to s_waitcnt vmcnt(0) in front
    // of every MFMA group and nothing stays in flight.
    const __amdgpu_buffer_rsrc_t rs_i = __builtin_amdgcn_make_buffer_rsrc((void *)pi, 0, (unsigned)p_end * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc((void *)po, 0, (unsigned)p_end * 4u, 0x00020000);
    auto load_idx = [&](int p, int &in_l, int &out_l) {
        const unsigned voff = (unsigned)(p + lane) * 4u;
        in_l = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_i, voff, 0, 0);
        out_l = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_o, voff, 0, 0);
    };
    // row slices of sub-step h (32 pairs) of the double-step whose indices are (in_l, out_l)
    auto load_rows = [&](int p, int h, int in_l, int out_l, u32x4 (&xr)[TA], u32x4 (&yr)[TB]) {
        const int src = 32 * h + 16 * (g >> 1) + i;
        const int in_s = __shfl(in_l, src, 64), out_s = __shfl(out_l, src, 64);
        const bool ok = p + src < p_end;
        const unsigned va = ok ? (unsigned)in_s * rb_a : OOB, vb = ok ? (unsigned)out_s * rb_b : OOB;
#pragma unroll
        for (int xa = 0; xa < TA; ++xa) xr[xa] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, va + ch_a[xa], 0, 0);
#pragma unroll
        for (int yb = 0; yb < TB; ++yb) yr[yb] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, vb + ch_b[yb], 0, 0);
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto compute = [&](const u32x4 (&xr)[TA], const u32x4 (&yr)[TB]) {
        bf16x8 at[TA], bt[TB];
#pragma unroll
        for (int xa = 0; xa < TA; ++xa) {
            const bf16x8 v = __builtin_bit_cast(bf16x8, xr[xa]);
            const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, P[0], zero, 0, 0, 0);
            const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, P[1], zero, 0, 0, 0);
            at[xa] = pack_hi16(d0, d1);
        }
#pragma unroll
        for (int yb = 0; yb < TB; ++yb) {
            const bf16x8 v = __builtin_bit_cast(bf16x8, yr[yb]);
            const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, P[0], zero, 0, 0, 0);
            const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, P[1], zero, 0, 0, 0);
            bt[yb] = pack_hi16(d0, d1);
        }
#pragma unroll
        for (int xa = 0; xa < TA; ++xa)
#pragma unroll
            for (int yb = 0; yb < TB; ++yb)
                acc[xa][yb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at[xa], bt[yb], acc[xa][yb], 0, 0, 0);
    };

    if (p_begin < p_end) {
        // Software pipeline over double-steps of 64 pairs, program order per iteration k:
        //   indices(k+2)  ->  rows(k+1) (needs indices(k+1), issued one iteration ago)  ->  MFMAs(k).
        // vmcnt retires in order, so requesting the indices FIRST means neither wait drains the queue:
        // rows(k+1) and indices(k+2) stay in flight under the MFMAs of k.  The scheduling barriers keep
        // hipcc from hoisting the MFMAs above the loads.  Loads past p_end are issued all the same
        // (index 0 / out-of-range row offset -> zeros).
        // Two iterations are written out with the buffer roles swapped: a register copy of a buffer
        // whose loads are in flight would wait for them.
        int in_c, out_c, in_n, out_n, in_f, out_f;
        u32x4 xa0[TA], ya0[TB], xa1[TA], ya1[TB], xb0[TA], yb0[TB], xb1[TA], yb1[TB];
        load_idx(p_begin, in_c, out_c);
        load_idx(p_begin + 64, in_n, out_n);
        load_rows(p_begin, 0, in_c, out_c, xa0, ya0);
        load_rows(p_begin, 1, in_c, out_c, xa1, ya1);
        for (int p = p_begin; p < p_end; p += 128) {
            load_idx(p + 128, in_f, out_f);
            __builtin_amdgcn_sched_barrier(0);
            load_rows(p + 64, 0, in_n, out_n, xb0, yb0);
            load_rows(p + 64, 1, in_n, out_n, xb1, yb1);
            __builtin_amdgcn_sched_barrier(0);
            compute(xa0, ya0);
            compute(xa1, ya1);
            __builtin_amdgcn_sched_barrier(0);
            load_idx(p + 192, in_n, out_n);
            __builtin_amdgcn_sched_barrier(0);
            load_rows(p + 128, 0, in_f, out_f, xa0, ya0);
            load_rows(p + 128, 1, in_f, out_f, xa1, ya1);
            __builtin_amdgcn_sched_barrier(0);
            compute(xb0, yb0);
            compute(xb1, yb1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- the wave owns (range, offset): it writes that partial itself (zeros for an empty segment) ----
    float *out = d.partial + ((long long)range * d.K + o) * d.ca * d.cb;
#pragma unroll
    for (int xa = 0; xa < TA; ++xa)
#pragma unroll
        for (int yb = 0; yb < TB; ++yb) {
            // D[i = ci][j = co]: lane (co = lane & 15, g) holds ci = 4g + r
            const int co = (tbg * TB + yb) * 16 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = (tag * TA + xa) * 16 + 4 * g + r;
                if (ci < d.ca && co < d.cb) out[(long long)ci * d.cb + co] = acc[xa][yb][r];
            }
        }
}

template <int TA, int TB>
void launch_variant(int blocks, const PJob *jobs_dev, const Ends &ends, hipStream_t s) {
    char name[32];
    snprintf(name, sizeof name, "wgrad_pairs_kernel<%d, %d>", TA, TB);
    doda_wgrad::trace(name, blocks, 256, ends.n);
    hipLaunchKernelGGL((wgrad_pairs_kernel<TA, TB>), dim3(blocks), dim3(256), 0, s, jobs_dev, ends);
}

}  // namespace

namespace doda_pairs {

size_t desc_bytes_per_job() { return sizeof(PJob) + sizeof(doda_wgrad::RJob); }

// descriptors grouped by kernel variant (at most MAX_GROUP per launch), the jobs of a variant in queue order
Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx) {
    Plan p;
    p.idx = idx;
    const int n = (int)idx.size();
    for (int k = 0; k < n; ++k) {
        p.part_off.push_back(p.partial_bytes);
        p.partial_bytes += pairs_geo(jobs[idx[k]]).partial_bytes;
        p.n_reduce += pairs_geo(jobs[idx[k]]).direct ? 0 : 1;
    }
    for (int ta = 1; ta <= 2; ++ta)
        for (int tb = 1; tb <= 2; ++tb) {
            Plan::Group grp{ta, tb, (int)p.order.size(), 0, 0};
            auto flush = [&]() {
                if (grp.count) p.groups.push_back(grp);
                grp = Plan::Group{ta, tb, (int)p.order.size(), 0, 0};
            };
            for (int k = 0; k < n; ++k) {
                const PairsGeo g = pairs_geo(jobs[idx[k]]);
                if (g.ta != ta || g.tb != tb) continue;
                if (grp.count == MAX_GROUP) flush();
                grp.blocks += (int)g.blocks;
                p.order.push_back(k);
                p.blk_end.push_back(grp.blocks);
                ++grp.count;
            }
            flush();
        }
    p.desc_bytes = p.order.size() * sizeof(PJob);
    return p;
}

void write_desc(const Plan &p, const doda_wgrad_job *jobs, char *part, void *desc, std::vector<doda_wgrad::RJob> &reduce,
                int *reduce_blocks) {
    PJob *pj = (PJob *)desc;
    for (size_t q = 0; q < p.order.size(); ++q) {
        const int k = p.order[q];
        const doda_wgrad_job &j = jobs[p.idx[k]];
        const PairsGeo g = pairs_geo(j);
        PJob d;
        memset(&d, 0, sizeof(d));
        d.a = j.a; d.b = j.b;
        d.pin = j.pair_in; d.pout = j.pair_out; d.pnum = j.pair_num; d.seg = j.pair_seg;
        d.partial = g.direct ? j.dw : (float *)(part + p.part_off[k]);
        d.a_bytes = (unsigned)((size_t)j.n_a * j.ca * 2);
        d.b_bytes = (unsigned)((size_t)j.n_rows * j.cb * 2);
        d.ca = j.ca; d.cb = j.cb; d.ld = j.pair_ld; d.K = j.K; d.n_rows = j.n_rows;
        d.n_range = g.n_range; d.n_og = g.n_og; d.n_tag = g.n_tag; d.n_tbg = g.n_tbg;
        d.seg_nt = j.pair_seg_nt;
        d.blk_end = p.blk_end[q];
        pj[q] = d;
    }
    for (size_t k = 0; k < p.idx.size(); ++k) {
        const doda_wgrad_job &j = jobs[p.idx[k]];
        const PairsGeo g = pairs_geo(j);
        if (!g.direct) doda_wgrad::push_reduce(reduce, reduce_blocks, part + p.part_off[k], j, g.n_range);
    }
}

int launch(const Plan &p, const void *desc_dev, hipStream_t s) {
    const PJob *pj = (const PJob *)desc_dev;
    for (const Plan::Group &g : p.groups) {
        Ends ends;
        memset(&ends, 0, sizeof(ends));
        ends.n = g.count;
        for (int k = 0; k < g.count; ++k) ends.end[k] = p.blk_end[g.first + k];
        // one case per shape pairs_geo can name (wgrad_plan.hpp WP_PAIR_SHAPES)
#define WP_CASE(A, B) if (g.ta == A && g.tb == B) launch_variant<A, B>(g.blocks, pj + g.first, ends, s);
        WP_PAIR_SHAPES(WP_CASE)
#undef WP_CASE
    }
    return doda_check_launch();
}

}  // namespace doda_pairs

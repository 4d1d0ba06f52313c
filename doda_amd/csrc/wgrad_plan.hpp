// Plan of doda_spconv_wgrad_multi: which of the four kernel classes takes a job, and for the gather-table class which
// wgrad_multi_kernel instantiation runs it over which row chunks, decided in pure host functions of the job list and the
// switches.  make_call_plan (spconv_wgrad.hip) classifies and plans with these; the classes' translation units hold their kernels,
// descriptors and launches and no decision of their own.  Plain C++17, no HIP header: tests/host/wgrad_plan_main.cpp compiles it
// with g++ and tests/test_wgrad_plan_host.py sweeps it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/doda_hip.h"

constexpr int WP_RT = 64;              // rows per step of the gather-table kernel
constexpr int WP_MAX_OGW = 7;          // its offsets per wave (4 waves x 7 >= 27)
constexpr int WP_TILE_ROWS = 256;      // tilebook.hpp TB_T
constexpr int WP_TILE_K = 27;          // tilebook.hpp TB_K
constexpr int WP_PAIRS_MAX_K = 28;
constexpr int WP_SEG_TILE = 256;       // rows per tile of the pair export's segment prefix (rulebook.hip PAIR_TILE)
constexpr int WP_RANGE_TILES = 8;      // a pair-kernel block's row range: 2048 rows of the lists' `in` side
constexpr int WP_RANGE_ROWS = WP_SEG_TILE * WP_RANGE_TILES;
// wgrad_wide's slice shapes TA x TB, at most 3 x 7 blocks of 16 channels and TA * TB <= 9
#define WW_SHAPES(X) X(3, 3) X(2, 4) X(2, 3) X(1, 5) X(1, 6) X(1, 7) X(1, 4) X(1, 3)
constexpr int WW_MAX_BLOCKS = 9, WW_MAX_TA = 3, WW_MAX_TB = 7;

// Every A/B switch and environment-derived threshold of the selection; one process-wide instance (spconv_wgrad.hip
// doda_wgrad::switches), filled at the first weight-gradient or option call.
struct WgradSwitches {
    // Rows per chunk of a gather-table job, at least.  Every chunk writes K*ca*cb*4 bytes of partials; with 512 blocks per job
    // the coarse levels (64..112 channels, a few thousand rows) wrote and re-read 5-28 MB per layer for a few hundred rows per
    // chunk, and the call holds ~40 other jobs to fill the chip with anyway
    int min_rows = 512;                // DODA_WGRAD_MIN_ROWS
    // 48-channel operands (level 3 of the U-Net): one 3 x 3 tile block gathers every row once instead of nine 1 x 1 blocks
    // gathering a third of it each (and reading the table nine times)
    bool no33 = false;                 // DODA_WGRAD_NO33
    int t33 = 128;                     // DODA_WGRAD_T33: blocks a 3 x 3 job aims at (a block does nine tiles' worth of work and its chunk writes all K*ca*cb partials)
    // OPT-IN (see gather_plan.hpp plan_gather): fp32 jobs of at least this many rows multiply bf16 head / tail splits (0: all of
    // them — one instantiation for every fp32 job keeps the layers of a step in shared launches; -1: none, the exact chain)
    long long f32_split_rows = -1;     // DODA_F32_WGRAD_SPLIT_ROWS
    // Rows from which a rulebook's tile jobs take the LDS-staged kernel even when pair lists are at hand.  Round 4 (block-major
    // chunks: one or two partials per workgroup whatever the number of layers): faster than the pair lists from ~40 k rows up —
    // 8 layers per call: 601 k rows 21.3 / 43.3 us per layer, 152 k rows 7.2 / 13.0, level 2 (154 k rows, 32 -> 32 as four
    // blocks) 21.3 / 23.7, 37 k rows 10.3 / 10.1 (tools/wl2.py).  Round 3's schedule (every workgroup walked every layer: a flush
    // per layer and workgroup) lost below 262 k rows.
    int wdma_min_rows = 32768;         // DODA_WDMA_MIN_ROWS (measurement aid)
    bool no_pairs = false;             // DODA_WGRAD_NO_PAIRS: every job with a table stays on the gather-table kernel (A/B measurements)
    bool wdma = true;                  // DODA_OPT_WDMA_KERNEL, DODA_NO_WDMA: the LDS-staged 16 x 16 tile kernel
    bool trace = false;                // DODA_TRACE_WGRAD: one stderr line per kernel launch of the call
};
inline WgradSwitches wgrad_switches_from_env() {
    const auto num = [](const char *e, long long dflt) { return e && *e ? atoll(e) : dflt; };   // unset or empty: the default
    const auto on = [](const char *e) { return e && e[0] == '1'; };
    const WgradSwitches d;
    return {(int)num(getenv("DODA_WGRAD_MIN_ROWS"), d.min_rows), on(getenv("DODA_WGRAD_NO33")), (int)num(getenv("DODA_WGRAD_T33"), d.t33),
            num(getenv("DODA_F32_WGRAD_SPLIT_ROWS"), d.f32_split_rows), (int)num(getenv("DODA_WDMA_MIN_ROWS"), d.wdma_min_rows),
            on(getenv("DODA_WGRAD_NO_PAIRS")), !on(getenv("DODA_NO_WDMA")), on(getenv("DODA_TRACE_WGRAD"))};
}

// wgrad_pairs_kernel's shapes TA x TB: blocks of 16 channels of (a, b) per wave (pairs_geo: two where the operand has two or more)
#define WP_PAIR_SHAPES(X) X(1, 1) X(2, 1) X(1, 2) X(2, 2)

constexpr size_t wp_align256(size_t x) { return (x + 255) / 256 * 256; }
constexpr int wp_div_up(long long a, long long b) { return (int)((a + b - 1) / b); }
inline bool wp_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool wp_accumulate(const doda_wgrad_job &j) { return (j.flags & DODA_WGRAD_ACCUMULATE) != 0; }

// ---- pair lists (spconv_wgrad_pairs.hip): a block = (row range of the lists' `in` side, group of 4 offsets, channel tile)
struct PairsGeo {
    int ta, tb, n_tag, n_tbg, n_og, n_range;
    bool direct;   // one range and no accumulation: the waves write dw themselves
    long long blocks;
    size_t partial_bytes;
};
inline PairsGeo pairs_geo(const doda_wgrad_job &j) {
    PairsGeo g;
    const int na = j.ca / 16, nb = j.cb / 16;
    g.ta = na >= 2 ? 2 : 1;
    g.tb = nb >= 2 ? 2 : 1;
    g.n_tag = wp_div_up(na, g.ta);
    g.n_tbg = wp_div_up(nb, g.tb);
    g.n_og = wp_div_up(j.K, 4);
    // rows of the lists' `in` side: the segment prefix covers pair_seg_nt tiles; identity lists: pair_ld pairs
    const long long rows = j.pair_seg ? (long long)j.pair_seg_nt * WP_SEG_TILE : (long long)j.pair_ld;
    g.n_range = wp_div_up(rows > 0 ? rows : 1, WP_RANGE_ROWS);
    g.direct = g.n_range == 1 && !wp_accumulate(j);
    g.blocks = (long long)g.n_range * g.n_og * g.n_tag * g.n_tbg;
    g.partial_bytes = g.direct ? 0 : wp_align256((size_t)g.n_range * j.K * j.ca * j.cb * 4);
    return g;
}
// bf16, 16-channel multiples, pair lists given or identity, operands inside the 4 GB hardware range check
inline bool pairs_eligible(const doda_wgrad_job &j) {
    if (j.elem_bytes != 2 || j.ca <= 0 || j.cb <= 0 || (j.ca % 16) || (j.cb % 16) || j.K <= 0 || j.n_rows <= 0) return false;
    if (!j.a || !j.b || !j.dw || j.K > WP_PAIRS_MAX_K) return false;
    if (!j.pair_in || !j.pair_out || j.pair_ld <= 0 || j.n_a <= 0) return false;
    // real lists come with their counts and segment prefix; the identity lists of a 1x1 conv with neither
    if (j.pair_num ? (!j.pair_seg || j.pair_seg_nt <= 0) : (j.pair_seg != nullptr || j.K != 1)) return false;
    if ((unsigned long long)j.n_a * j.ca * 2ull >= 0x3fffffffull) return false;
    if ((unsigned long long)j.n_rows * j.cb * 2ull >= 0x3fffffffull) return false;
    if (!wp_al16(j.a) || !wp_al16(j.b) || !wp_al16(j.dw)) return false;
    return pairs_geo(j).blocks <= 0x3fffffff;
}

// ---- LDS-staged 16 x 16 tile kernel (spconv_wdma.hip): persistent workgroups, a multiple of the 8 XCDs, one per CU at most
inline int wdma_groups(int n_rows) {
    const int groups = (wp_div_up(n_rows, WP_TILE_ROWS) + 7) / 8 * 8;
    return groups > 256 ? 256 : groups;
}
inline int wdma_blocks(const doda_wgrad_job &j) { return (j.ca / 16) * (j.cb / 16); }   // 16 x 16 channel blocks
inline size_t wdma_block_partial_bytes(int n_rows) { return wp_align256((size_t)wdma_groups(n_rows) * WP_TILE_K * 256 * sizeof(float)); }
// bf16, K = 27, a tilebook of the job's table; 16 -> 16, and — round 4 — 16 .. 64 channels on either side as 16 x 16 channel
// blocks over row-strided slices
inline bool wdma_eligible(const doda_wgrad_job &j, const WgradSwitches &sw) {
    return j.tilebook && j.tbl && j.elem_bytes == 2 && j.ca % 16 == 0 && j.ca <= 64 && j.cb % 16 == 0 && j.cb <= 64 &&
           j.K == WP_TILE_K && j.n_rows > 0 && j.a && j.b && j.dw && j.n_a == j.n_rows && j.ld >= j.n_rows &&
           (size_t)j.n_rows * 128 < 0x7ffffff0ull && (size_t)j.K * j.ld * 4 < 0xffffffffull &&
           !(((uintptr_t)j.a | (uintptr_t)j.b | (uintptr_t)j.tilebook) & 15) && sw.wdma;
}

// ---- wide tile kernel (spconv_wwide.hip).  Slice shape of a job: TB = the widest output-channel slice of at most 7 blocks
// dividing cb / 16, TA = the widest input slice of at most 3 blocks dividing ca / 16 with TA * TB <= 9
inline bool ww_shape(int ca, int cb, int *ta, int *tb) {
    const int A = ca / 16, B = cb / 16;
    int b = B;
    while (b > WW_MAX_TB || B % b) --b;
    int a = WW_MAX_TA;
    while (a > 1 && (A % a || a * b > WW_MAX_BLOCKS)) --a;
    bool known = false;
#define WW_KNOWN(X, Y) known |= (a == X && b == Y);
    WW_SHAPES(WW_KNOWN)
#undef WW_KNOWN
    *ta = a; *tb = b;
    return known;
}
// bf16 K = 27 layers of 48 .. 224 channels on both sides with a tilebook of the job's table
inline bool wwide_eligible(const doda_wgrad_job &j) {
    int ta, tb;
    return j.tilebook && j.tbl && j.elem_bytes == 2 && j.K == WP_TILE_K && j.n_rows > 0 && j.a && j.b && j.dw &&
           j.ca % 16 == 0 && j.cb % 16 == 0 && j.ca >= 48 && j.cb >= 48 && j.ca <= 224 && j.cb <= 224 &&
           j.n_a == j.n_rows && j.ld >= j.n_rows && !(((uintptr_t)j.a | (uintptr_t)j.b | (uintptr_t)j.tilebook | (uintptr_t)j.dw) & 15) &&
           ww_shape(j.ca, j.cb, &ta, &tb);
}

// ---- the class of a job
enum WgradClass { J_SKIP = 0, J_ZERO = 1, J_DENSE = 2, J_PAIRS = 3, J_TILE = 4, J_WIDE = 5 };
inline int classify(const doda_wgrad_job &j, const WgradSwitches &sw) {
    if (j.n_rows == 0 && j.dw && j.K > 0 && j.ca > 0 && j.cb > 0) return wp_accumulate(j) ? J_SKIP : J_ZERO;
    // a tilebook of the job's table and 48 .. 224 channels on both sides: the wide LDS-staged kernel.  It takes 48 / 64-channel
    // layers before wgrad_dma16, whose 16 x 16 blocks re-stage the tile once per block, and only jobs that would
    // otherwise run the gather-table kernel, whose sums it reproduces (jobs with pair lists keep them)
    if (wwide_eligible(j) && !pairs_eligible(j)) return J_WIDE;
    if (wdma_eligible(j, sw) && (j.n_rows >= sw.wdma_min_rows || !pairs_eligible(j))) return J_TILE;
    if (pairs_eligible(j) && (!sw.no_pairs || !j.tbl)) return J_PAIRS;
    return J_DENSE;
}

// ---- the gather-table class (spconv_wgrad.hip): wgrad_multi_kernel<policy, TA, TB, OGW, VOK>
enum WgradPolicy : uint8_t { WP_BF16, WP_F32, WP_F32S };   // F32S: fp32 rows multiplied as bf16 head / tail splits
struct DensePlan {
    int TA, TB, OGW, n_og, n_tag, n_tbg, R, rows_per_chunk, blocks;   // a block: TA x TB tiles of 16 x 16 channels x 4 OGW offsets x one of R row chunks
    WgradPolicy policy;
    bool vok;      // rows of both operands are 16-byte aligned multiples of 16 bytes
    int key;       // one launch per key
};
inline bool dense_valid(const doda_wgrad_job &j) {
    return j.ca > 0 && j.cb > 0 && j.K > 0 && j.K <= 4 * WP_MAX_OGW && j.n_rows > 0 && j.ld >= j.n_rows && j.a && j.b && j.tbl && j.dw &&
           (j.elem_bytes == 2 || j.elem_bytes == 4);
}
inline bool dense_vok(const doda_wgrad_job &j) {
    return (size_t)j.ca * j.elem_bytes % 16 == 0 && (size_t)j.cb * j.elem_bytes % 16 == 0 && wp_al16(j.a) && wp_al16(j.b);
}
// The job is one of many in a call — the other layers fill the chip, so a layer needs far fewer row chunks than a launch of its
// own would (each chunk costs K*ca*cb*4 bytes of partials to write and reduce).
inline DensePlan plan_dense(int K, int ca, int cb, int n_rows, int esz, bool vok, const WgradSwitches &sw) {
    DensePlan p;
    const int ta = (ca + 15) / 16, tb = (cb + 15) / 16;
    p.TA = (ta % 2 == 0) ? 2 : 1;
    p.TB = (tb % 2 == 0) ? 2 : 1;
    if (ta == 3 && tb == 3 && esz == 2 && K > 8 && !sw.no33) { p.TA = 3; p.TB = 3; }
    p.n_tag = ta / p.TA;
    p.n_tbg = tb / p.TB;
    // 2x2 accumulator tiles x 7 offsets would need 112 accumulator registers (1 wave/SIMD): give
    // such blocks 4 offsets per wave and spread the offsets over several block groups instead
    // offsets per wave for 1- and 2-tile blocks (rocprofv3, levels 1 / 3 / 5): bf16 7 -> 4 offsets
    // 54.8 -> 52.2, 39.6 -> 35.3, 19.0 -> 14.3 us (fewer registers, half the partials); fp32 the other
    // way round (91 vs 106 us at level 3): its 16 dY fragment reads per step amortise over more offsets
    p.OGW = (p.TA * p.TB == 4 || esz == 2) ? 4 : WP_MAX_OGW;
    if (p.TA * p.TB == 9 || K <= 8) p.OGW = 2;   // 3 x 3: 72 accumulator registers
    p.n_og = wp_div_up(K, 4 * p.OGW);
    const int gy = p.n_tag * p.n_tbg * p.n_og;
    const int rows = n_rows > 0 ? n_rows : 1;
    // blocks over the whole grid (whole U-Net step, wgrad + reduce): 1024 -> 1.86 ms, 512 -> 1.67, 256 -> 1.67, 128 -> 1.99
    int R = wp_div_up(p.TA * p.TB == 9 ? sw.t33 : 512, gy);
    const int max_r = rows / sw.min_rows > 1 ? rows / sw.min_rows : 1;
    if (R > max_r) R = max_r;
    if (R < 1) R = 1;
    p.rows_per_chunk = wp_div_up(wp_div_up(rows, R), WP_RT) * WP_RT;
    p.R = wp_div_up(rows, p.rows_per_chunk);
    p.blocks = p.R * gy;
    const bool split = esz == 4 && sw.f32_split_rows >= 0 && (long long)n_rows >= sw.f32_split_rows;
    p.policy = esz == 2 ? WP_BF16 : split ? WP_F32S : WP_F32;
    p.vok = vok;
    p.key = ((((esz * 4 + p.TA) * 4 + p.TB) * 8 + p.OGW) * 2 + (vok ? 1 : 0)) * 2 + (split ? 1 : 0);
    return p;
}
inline DensePlan plan_dense(const doda_wgrad_job &j, const WgradSwitches &sw) {
    return plan_dense(j.K, j.ca, j.cb, j.n_rows, j.elem_bytes, dense_vok(j), sw);
}
// partials unless the job's one row chunk can overwrite dw itself
inline bool dense_needs_partial(const DensePlan &p, const doda_wgrad_job &j) { return p.R > 1 || wp_accumulate(j); }
inline size_t dense_partial_bytes(const DensePlan &p, const doda_wgrad_job &j) {
    return dense_needs_partial(p, j) ? wp_align256((size_t)p.R * j.K * j.ca * j.cb * 4) : 0;
}

// wgrad_wide: one workgroup per (channel slice, row chunk of the gather-table plan), whose sums it reproduces bit for bit
struct WideGeo { int ta, tb, P, rpc, blocks; size_t partial_bytes; };   // P row chunks of rpc rows
inline WideGeo wwide_geo(const doda_wgrad_job &j, const WgradSwitches &sw) {
    WideGeo g;
    const DensePlan p = plan_dense(j, sw);
    ww_shape(j.ca, j.cb, &g.ta, &g.tb);
    g.P = p.R; g.rpc = p.rows_per_chunk;
    g.blocks = (j.ca / (16 * g.ta)) * (j.cb / (16 * g.tb)) * g.P;
    g.partial_bytes = wp_align256((size_t)g.blocks * WP_TILE_K * 256 * g.ta * g.tb * 4);
    return g;
}

// ---- The compiled set.  launch_multi_variant (spconv_wgrad.hip) instantiates a kernel under `if constexpr (dense_compiled(...))`
// and nothing else; dense_compiled admits exactly the (policy, TA, TB, OGW) plan_dense can return, for both VOK
// (tests/test_wgrad_plan_host.py: admitted = built = swept = probed).  The set of tiles defines what is compiled; their order only
// the order in which the compiler emits the kernels, kept as the if-ladder this table replaced had it.
template <int TA_, int TB_, int OGW_> struct WgradTile { static constexpr int TA = TA_, TB = TB_, OGW = OGW_; };
template <class... T> struct WgradTiles {};
typedef WgradTiles<WgradTile<3, 3, 2>, WgradTile<1, 1, 2>, WgradTile<2, 1, 2>, WgradTile<1, 2, 2>, WgradTile<2, 2, 2>, WgradTile<1, 1, 4>,
                   WgradTile<2, 1, 4>, WgradTile<1, 2, 4>, WgradTile<1, 1, 7>, WgradTile<2, 1, 7>, WgradTile<1, 2, 7>, WgradTile<2, 2, 4>> DenseTiles;
template <class... T>
constexpr bool wgrad_listed(WgradTiles<T...>, int ta, int tb, int ogw) { return ((T::TA == ta && T::TB == tb && T::OGW == ogw) || ...); }
// bf16: 4 offsets per wave, 2 for 3 x 3 blocks and for K <= 8.  fp32: 7, or 4 for 2 x 2 blocks, or 2 for K <= 8; no 3 x 3 blocks
constexpr bool dense_compiled(WgradPolicy p, int ta, int tb, int ogw) {
    return wgrad_listed(DenseTiles{}, ta, tb, ogw) && (p == WP_BF16 ? ogw != WP_MAX_OGW : ta * tb != 9 && (ogw == 2 || (ogw == 4) == (ta * tb == 4)));
}

// The instantiation as a kernel trace shows it, namespaces stripped.  Returns the length.
inline int dense_name(const DensePlan &p, char *buf, size_t n) {
    static const char *const pol[3] = {"BF16", "F32", "F32S"};
    return snprintf(buf, n, "wgrad_multi_kernel<%s, %d, %d, %d, %s>", pol[p.policy], p.TA, p.TB, p.OGW, p.vok ? "true" : "false");
}

// Route plan of doda_spconv_gather_ex: which kernel instantiation a call reaches, with which grid, decided in ONE pure host
// function.  doda_spconv_gather_ex (spconv_gather.hip) describes, plans, packs and launches what the route names; the launchers of the
// kernel families (spconv_gather.hip, spconv_tile.hip, spconv_wlds.hip) hold no decision of their own.  Plain C++17, no HIP
// header: tests/host/gather_plan_main.cpp compiles it with g++ and tests/test_gather_plan_host.py sweeps it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/doda_hip.h"

constexpr int GP_TILE_ROWS = 256;      // tilebook.hpp TB_T: output rows per tile
constexpr int GP_TILE_K = 27;          // tilebook.hpp TB_K
constexpr int GP_PRE_MAX_C = 256;      // spconv_common.hpp PRE_MAX_C: most channels a folded BatchNorm carries
constexpr int GP_TILE_MAX_GROUPS = 768;     // conv_tile: 3 workgroups per CU x 256 CUs
constexpr int GP_TILE16_GROUPS = 512;    // conv_tile16: 2 workgroups per CU

// Every fact of a call that the selection depends on.
struct GatherCall {
    int K, kc, nc, n_out, ld, esz;     // esz: bytes of a feature element (2 bf16, 4 fp32)
    long long n_in, pre_rows;          // rows of x; rows the prologue states
    bool out32, packed;                // fp32 output rows of a bf16 call; w_layout & 0x100: `w` holds fragment-packed weights
    int layout;                        // w_layout & 3
    size_t ws_bytes;                   // 0: no workspace
    int x_al, y_al;                    // address mod 16 (mod 4 * esz, the generic kernel's vector granule, follows)
    unsigned x_ld, y_ld, res_ld, bnx_ld;   // row strides in elements, 0: dense
    bool res_bcast, stats;
    int pre_kind;                      // folded BatchNorm: 0 none, 1 forward, 2 backward, 3 backward + skip gradient
    unsigned side_ld, aux_ld, add_ld;
    bool side, aux, add;               // operand present and 16-byte aligned
    bool saved, totals, running, affine;   // mean & invstd, tot.ta, running mean & variance, gamma & beta present
    bool tilebook;
    int tilebook_rows;                 // with `tilebook`: the rows it was built for
};

constexpr int GP_MAX_K = 27;           // spconv_gather.hip MAX_K: most kernel offsets of a table
constexpr int GP_MAX_CHANNELS = 4096;

// The call description of doda_spconv_gather_ex as a pure function of its arguments: every check of the entry point, in its
// order and with its statuses, and the normalisations of the row strides (a stride equal to the channel count is dense: 0;
// a broadcast residual has no stride).  Pointers are looked at for null-ness and their address mod 16 only; `epi` and its
// prologue are read as plain structs.  status != DODA_OK: the call returns it; status == DODA_OK with call.n_out == 0: the
// call has nothing to do; otherwise `call` is what plan_gather decides on.  (doda_layers_run asks the same question for a
// whole op list before its first launch: layers_plan.hpp.)
struct GatherDescription {
    int status;
    GatherCall call;
};
inline GatherDescription describe_gather(const void *x, int32_t n_in, int32_t kc, int32_t elem_bytes, const float *w, int32_t nc,
                                         const int32_t *tbl, int32_t ld, int32_t K, int32_t n_out, const void *y, int32_t y_is_f32,
                                         int32_t w_layout, const void *ws, size_t ws_bytes, const doda_conv_epilogue *epi) {
    GatherDescription d{};
    GatherCall &c = d.call;
    const auto al = [](const void *p) { return (int)((uintptr_t)p & 15); };
    d.status = DODA_ERR_INVALID;
    if (elem_bytes != 2 && elem_bytes != 4) return d;
    if (kc <= 0 || nc <= 0 || K <= 0 || n_out < 0 || ld < n_out || (w_layout & 3) > 2 || (w_layout & ~0x103)) return d;
    if (n_out == 0) { d.status = DODA_OK; return d; }
    if (!x || !w || !tbl || !y) return d;
    if (K > GP_MAX_K || nc > GP_MAX_CHANNELS || kc > GP_MAX_CHANNELS) { d.status = DODA_ERR_UNSUPPORTED; return d; }
    if (epi) {
        const bool res = epi->residual != nullptr;
        c.res_bcast = res && epi->residual_bcast;
        bool bn_x = false;
        if (epi->stats) {
            if (!epi->stats_rows_h) return d;
            c.stats = true;
            if (epi->bn_x) {
                if (!epi->bn_mean || !epi->bn_invstd || !epi->bn_gamma || !epi->bn_beta) return d;
                bn_x = true;
            }
        }
        if (epi->x_ld < 0 || epi->y_ld < 0 || epi->residual_ld < 0 || epi->bn_x_ld < 0) return d;
        c.x_ld = (unsigned)epi->x_ld; c.y_ld = (unsigned)epi->y_ld;
        c.res_ld = res ? (unsigned)epi->residual_ld : 0u; c.bnx_ld = bn_x ? (unsigned)epi->bn_x_ld : 0u;
        if ((c.x_ld && c.x_ld < (unsigned)kc) || (c.y_ld && c.y_ld < (unsigned)nc) || (c.res_ld && c.res_ld < (unsigned)nc) ||
            (c.bnx_ld && c.bnx_ld < (unsigned)nc))
            return d;
        if (c.x_ld == (unsigned)kc) c.x_ld = 0;      // dense
        if (c.y_ld == (unsigned)nc) c.y_ld = 0;
        if (c.res_ld == (unsigned)nc) c.res_ld = 0;
        if (c.bnx_ld == (unsigned)nc) c.bnx_ld = 0;
        if (c.res_bcast) c.res_ld = 0;
        if (const doda_conv_prologue *q = epi->prologue) {
            if (q->kind < 1 || q->kind > 3 || q->rows != n_in || q->side_ld < kc || (q->kind >= 2 && q->aux_ld < kc) ||
                (q->kind >= 3 && q->add_ld < kc) || (q->kind >= 2 && (!q->dgamma || !q->dbeta || !q->totals)) ||
                (q->kind == 1 && q->totals && (!q->mean || !q->invstd || (!q->running_mean != !q->running_var))) ||
                (q->kind == 1 && q->totals_b && (q->c_a <= 0 || q->c_a >= kc || q->c_a % 4 || !q->totals)))
                return d;
            c.pre_kind = q->kind; c.pre_rows = q->rows;
            c.side_ld = (unsigned)q->side_ld; c.aux_ld = (unsigned)q->aux_ld; c.add_ld = (unsigned)q->add_ld;
            c.side = q->side && al(q->side) == 0; c.aux = q->aux && al(q->aux) == 0; c.add = q->add && al(q->add) == 0;
            c.saved = q->mean && q->invstd; c.totals = q->totals != nullptr;
            c.running = q->kind == 1 && q->running_mean && q->running_var;   // (a backward prologue carries no running statistics)
            c.affine = q->gamma && q->beta;
        }
        c.tilebook = epi->tilebook != nullptr; c.tilebook_rows = epi->tilebook_rows;
    }
    c.K = K; c.kc = kc; c.nc = nc; c.n_out = n_out; c.ld = ld; c.esz = elem_bytes; c.n_in = n_in;
    c.out32 = elem_bytes == 2 && y_is_f32 != 0;
    c.layout = w_layout & 3; c.packed = (w_layout & 0x100) != 0; c.ws_bytes = ws ? ws_bytes : 0;
    c.x_al = al(x); c.y_al = al(y);
    d.status = DODA_OK;
    return d;
}

// Every A/B switch and environment-derived threshold of the selection; one process-wide instance (spconv_gather.hip).
struct GatherSwitches {
    long long f32_split_rows = -1;     // DODA_F32_SPLIT_ROWS: fp32 layers of at least this many rows take PF32S (-1: none)
    long long pre_small_blocks = 2048; // DODA_PRE_SMALL_BLOCKS: folded calls up to this many 16-row blocks take <1,1>
    bool f32_conv_tile = true;         // DODA_F32_CONV_TILE
    // conv_tile16 pays off from the point where conv_tile's workgroups run more than one tile each (a single tile per
    // workgroup has nothing to prefetch, and three shallow workgroups per CU then beat two)
    int tile16_min_tiles = GP_TILE_MAX_GROUPS + 1;   // DODA_TILE16_MIN_TILES (at least GP_TILE16_GROUPS: every workgroup must own a tile)
    bool tile = true;                  // DODA_OPT_TILE_KERNEL
    bool wlds = true;                  // DODA_OPT_WLDS_KERNEL
    bool tile_pipeline = true;         // DODA_OPT_TILE_PIPELINE: conv_tile16 for 16 -> 16 layers of many tiles
    bool tile_dual = true;             // DODA_OPT_TILE_DUAL, DODA_TILE_DUAL: both channel blocks of a 32-output-channel layer in one pass
    bool conv_up = true;               // DODA_OPT_CONV_UP, DODA_CONV_UP: conv_up32 for one-source-per-row tables
};

// Fragment packing the fast kernel uses for a layer: 0x10 wide (bf16, >= 32 input channels),
// 0x20 pair (bf16, exactly 16 input channels, more than one offset), 0 narrow.
inline int pack_mode(int K, int kc, int elem_bytes) {
    if (elem_bytes == 2 && kc >= 32 && kc % 8 == 0) return 0x10;
    if (elem_bytes == 2 && kc == 16 && K >= 2) return 0x20;
    return 0;
}

struct PackGeometry {
    int mode, n_chunk, NB;
    long long frags;                   // fragments (= threads of the pack kernel)
    size_t bytes;
};
// (`mode` differs from pack_mode() where a call cannot take the fast kernel: the generic kernel reads narrow fragments)
inline PackGeometry pack_geometry(int K, int kc, int nc, int esz, int mode) {
    PackGeometry g;
    g.mode = mode;
    g.n_chunk = mode == 0x10 ? (kc + 31) / 32 : (kc + 15) / 16;
    g.NB = (nc + 15) / 16;
    g.frags = mode == 0x20 ? (long long)K * g.NB * 32 : (long long)K * g.n_chunk * g.NB * 64;
    g.bytes = (size_t)g.frags * (mode != 0 ? 16 : 4 * (size_t)esz);
    return g;
}
inline PackGeometry pack_geometry(int K, int kc, int nc, int esz) { return pack_geometry(K, kc, nc, esz, pack_mode(K, kc, esz)); }

enum GatherFamily : uint8_t { GF_GENERIC, GF_FAST, GF_UP32, GF_TILE, GF_TILE16, GF_WLDS48 };
enum GatherPolicy : uint8_t { GP_NARROW, GP_WIDE, GP_PAIR, GP_F32_SPLIT };
constexpr int GP_RING_DEPTH = 3;       // conv_fast's D (launch_fast, spconv_gather.hip)

struct GatherRoute {
    int status;                        // DODA_OK, or the error the call returns (then nothing else is set)
    GatherFamily family;
    GatherPolicy policy;               // GENERIC / FAST, with NBW, S, split (FAST) and pre (FAST: PRE)
    uint8_t esz, NBW, S, pre, mode, maxnb;   // mode, maxnb, dual: TILE
    bool split, dual, out32, stats;    // out32, stats: the OUT32 / STATS template parameters
    bool vec_ok;                       // GENERIC: a kernel argument
    PackGeometry geo;
    unsigned grid, block;
    int n_part;                        // statistics rows
    unsigned x_bytes, y_bytes, tbl_bytes, w_bytes;   // buffer ranges handed to the kernel
};

inline GatherRoute plan_gather(const GatherCall &c, const GatherSwitches &sw) {
    const auto fail = [](int status) { GatherRoute e{}; e.status = status; return e; };
    const auto cdiv = [](long long a, long long b) { return (unsigned)((a + b - 1) / b); };
    const int K = c.K, kc = c.kc, nc = c.nc, n_out = c.n_out, esz = c.esz;
    const uint64_t n_in = (uint64_t)c.n_in, uesz = (uint64_t)esz;
    const int NB = (nc + 15) / 16;
    // all rows the table may reference must sit inside the 2 GB buffer window of the fast path
    const bool x_rows_bytes_ok = c.n_in > 0 && n_in * kc * uesz < 0x7ffffff0ull;
    // ABI 11: row strides (column slices of wider matrices) and the folded BatchNorm in conv_fast; ABI 12: the LDS-staged kernels
    // (conv_tile*, conv_up32, conv_wlds48) take strided OUTPUT-side operands (y, residual, BatchNorm input) — their gathered x stays dense
    const bool strided = (c.x_ld && c.x_ld != (unsigned)kc) || c.y_ld || c.res_ld || c.bnx_ld;
    const bool x_dense = !c.x_ld || c.x_ld == (unsigned)kc;
    const bool folded = c.pre_kind != 0;
    const uint64_t x_ld = c.x_ld ? c.x_ld : (uint64_t)kc, y_ld = c.y_ld ? c.y_ld : (uint64_t)nc;
    const bool ld_ok = x_ld % 4 == 0 && y_ld % 4 == 0 && c.res_ld % 4 == 0 && c.bnx_ld % 4 == 0 &&
                       n_in * x_ld * uesz < 0x7ffffff0ull && (uint64_t)n_out * y_ld * 4 < 0x7fffffffull &&
                       (uint64_t)n_out * (c.res_ld ? c.res_ld : (uint64_t)nc) * 4 < 0x7fffffffull &&
                       (uint64_t)n_out * (c.bnx_ld ? c.bnx_ld : (uint64_t)nc) * 4 < 0x7fffffffull;
    const bool fast = (kc % 4 == 0) && (nc % 4 == 0) && c.x_al == 0 && c.y_al == 0 && ((uint64_t)n_out * nc * 4 < 0x7fffffffull) &&
                      ((uint64_t)K * c.ld * 4 < 0xffffffffull) && x_rows_bytes_ok && ld_ok;
    if ((strided || folded) && !fast) return fail(DODA_ERR_UNSUPPORTED);
    if (c.out32 && esz != 4 && !fast) return fail(DODA_ERR_UNSUPPORTED);
    if (c.stats && !fast) return fail(DODA_ERR_UNSUPPORTED);   // the statistics ride in the fast kernel's epilogue only
    const int mode = pack_mode(K, kc, esz);
    const bool wide = fast && mode == 0x10, pair = fast && mode == 0x20;
    GatherRoute r{};
    r.status = DODA_OK;
    r.geo = pack_geometry(K, kc, nc, esz, fast ? mode : 0);
    if (c.packed) {   // `w` already holds fragment-packed weights (doda_spconv_pack_multi)
        if (mode != 0 && !fast) return fail(DODA_ERR_UNSUPPORTED);  // packed for a mode this call cannot take
    } else if (c.ws_bytes < r.geo.bytes) return fail(DODA_ERR_WORKSPACE);
    if (c.res_bcast && !fast) return fail(DODA_ERR_UNSUPPORTED);   // (the broadcast residual lives in conv_fast's epilogue)

    r.esz = (uint8_t)esz;
    r.stats = c.stats;
    r.out32 = c.out32 && esz != 4;
    r.block = 256;
    r.x_bytes = (unsigned)(((n_in - 1) * x_ld + kc) * uesz);
    r.tbl_bytes = (unsigned)((uint64_t)K * c.ld * 4);
    r.w_bytes = (unsigned)r.geo.bytes;
    r.y_bytes = (unsigned)((((uint64_t)n_out - 1) * y_ld + nc) * (r.out32 ? 4 : uesz));
    const long long wf = ((long long)n_out + 15) / 16;   // 16-row wave tiles
    const auto dense = [&](int nbw, int s, bool split) {   // conv_fast / conv_gather: a workgroup owns (4 or 1) x 16 S rows
        r.family = fast ? GF_FAST : GF_GENERIC;
        r.NBW = (uint8_t)nbw; r.S = (uint8_t)s; r.split = split;
        const unsigned row_blocks = cdiv(n_out, (split ? 1 : 4) * 16 * s);
        r.grid = row_blocks * cdiv(NB, nbw);
        r.n_part = fast ? (int)row_blocks : 0;
        r.vec_ok = (kc % 4 == 0) && (nc % 4 == 0) && c.x_al % (4 * esz) == 0 && c.y_al % (4 * esz) == 0;
        return r;
    };
    const auto staged = [&](GatherFamily f, unsigned grid, unsigned parts) {   // the LDS-staged families: `parts` statistics rows
        r.family = f; r.grid = grid; r.n_part = (int)parts;
        return r;
    };
    const unsigned n_tiles = cdiv(n_out, GP_TILE_ROWS);

    if (folded) {
        // the folded BatchNorm: 16-byte pieces of rows in the output's dtype (bf16 >= 32 channels, fp32), at most PRE_MAX_C
        // channels, every operand 16-byte aligned; split blocks — 16 rows x one channel block while the grid stays small,
        // 32 rows x four channel blocks above (the shapes the unfolded call would take at the coarse levels)
        const unsigned va16 = 16u / (unsigned)esz;
        const int pk = c.pre_kind;
        if (c.out32 || pair || (esz == 2 && !wide) || kc > GP_PRE_MAX_C || kc % (int)va16 != 0 || x_ld % va16 != 0 ||
            !c.side || c.side_ld % va16 != 0 || c.pre_rows != c.n_in ||
            (pk >= 2 && (!c.aux || c.aux_ld % va16 != 0 || !c.saved || !c.totals || n_in * c.aux_ld * uesz >= 0x7ffffff0ull)) ||
            (pk >= 3 && (!c.add || c.add_ld % va16 != 0 || n_in * c.add_ld * uesz >= 0x7ffffff0ull)) ||
            (pk == 1 && !c.totals && !c.running) || !c.affine)
            return fail(DODA_ERR_UNSUPPORTED);
        if (pk < 1 || pk > 3) return fail(DODA_ERR_INVALID);
        r.policy = wide ? GP_WIDE : GP_NARROW;
        r.pre = (uint8_t)pk;
        return wf * NB <= sw.pre_small_blocks ? dense(1, 1, true) : dense(4, 2, true);
    }
    // K <= 8, 32 input channels, fewer input rows than output rows (the k2 s2 rulebook read from the fine side: one source row
    // per output row): conv_up32 (spconv_tile.hip).  DODA_CONV_UP=0 / doda_set_option(DODA_OPT_CONV_UP, 0): conv_fast as before.
    if (sw.conv_up && wide && kc == 32 && K <= 8 && K > 1 && c.n_in < (long long)n_out && nc % 16 == 0 && !c.res_bcast && x_dense &&
        sw.tile)
        return staged(GF_UP32, n_tiles, n_tiles);   // one statistics row per 256 rows
    // A tilebook of this table and rows of 32 / 64 bytes: the LDS-staged tile kernel (spconv_tile.hip)
    if (!c.res_bcast && x_dense) {
        // (fp32 rows: the tile kernel's fp32 mode is bound by the fp32 matrix rate like the dense-table kernel and measured
        // within a few percent of it; DODA_F32_CONV_TILE=0 keeps fp32 forward / data-grad calls on conv_fast even when the
        // table carries a tilebook — the fp32 weight gradient uses the tilebook either way)
        const int tmode = pair ? 0 : (wide && kc == 32) ? 1 : (fast && esz == 4 && kc == 16 && sw.f32_conv_tile) ? 2 : -1;
        // (statistics: the tile kernels' per-lane accumulators hold up to two channel blocks, the dual-pass 64-byte-row kernel four)
        const bool stats_fit = !c.stats || NB <= 2 || (tmode == 1 && NB == 4 && sw.tile_dual);
        if (tmode >= 0 && c.tilebook && K == GP_TILE_K && c.tilebook_rows == n_out && sw.tile && stats_fit) {
            const int nt = (int)n_tiles;   // (tilebook.hpp tilebook_view: ceil(rows / TB_T))
            r.out32 = c.out32 || esz == 4;   // (MODE 2 is always OUT32)
            if (tmode == 0 && NB == 1 && sw.tile_pipeline && nt >= sw.tile16_min_tiles) return staged(GF_TILE16, GP_TILE16_GROUPS, GP_TILE16_GROUPS);
            r.mode = (uint8_t)tmode;
            // 32 output channels: both channel blocks in one pass; 64 output channels: two dual passes (the 32 -> 64 data
            // gradient of level 2) when statistics ride along, the 32-channel instantiation otherwise
            r.dual = tmode == 1 && (NB == 2 || NB == 4) && sw.tile_dual;
            if (r.dual) r.maxnb = (NB == 4 && c.stats) ? 4 : 2;
            else r.maxnb = (NB > 1 && c.stats) ? 2 : 1;   // statistics of a second channel block
            const unsigned groups = (n_tiles + 7) / 8 * 8;   // persistent: 3 (64-byte rows: 2) workgroups per CU, a multiple of the 8 XCDs
            const unsigned max_groups = tmode == 0 ? GP_TILE_MAX_GROUPS : GP_TILE_MAX_GROUPS * 2 / 3;
            const unsigned g = groups > max_groups ? max_groups : groups;
            return staged(GF_TILE, g, g);   // one statistics row per persistent workgroup
        }
    }
    // 48 -> 48 channels on a mid-size level: the layer's fragments in LDS, one workgroup per CU (spconv_wlds.hip)
    if (!c.res_bcast && x_dense && wide && kc == 48 && nc == 48 && K == 27 && !c.out32 && n_out >= 8192 && n_out <= 262144 && sw.wlds) {
        r.block = 512;
        return staged(GF_WLDS48, n_tiles < 256 ? n_tiles : 256, n_tiles);
    }
    r.policy = wide ? GP_WIDE : pair ? GP_PAIR : GP_NARROW;
    // OPT-IN: fp32 layers of at least DODA_F32_SPLIT_ROWS output rows (e.g. 65536; 0: all; unset / -1: none) multiply bf16
    // head / tail splits of both operands (spconv_common.hpp mma_f32_k16).  Measured (round 5): fp32 step 11.85 -> 11.1 ms
    // with every weight gradient and the >= 65536-row gathers split, every 1e-4 kernel test and the golden's gradient
    // NORMS (5e-3) still green — but the elementwise distance of the U-Net's gradients from the fp64 golden grows from
    // ~1e-3 to ~7e-3 (2^-16 products through 70 layers), and fp32 is this repository's PARITY precision: exact by default
    if (fast && esz == 4 && sw.f32_split_rows >= 0 && (long long)n_out >= sw.f32_split_rows) r.policy = GP_F32_SPLIT;
    // Tile choice: many rows -> more subtiles per wave and all channel blocks in one wave (x is
    // gathered once); few rows -> one subtile, channel blocks spread over the grid so the chip
    // still sees thousands of waves.
    if (fast && (long long)K * r.geo.n_chunk >= 12) {
        // few rows, long unit chains: split the offsets of a 16-row tile over the block's waves
        // measured (rocprofv3, per dispatch): 795 / 210 / 49 blocks 12.7 -> 9.5, 12.2 -> 6.1,
        // 16.0 -> 6.3 us; 2808 blocks (level 4) 18.0 -> 24.7 us, so only below ~1k blocks
        // (two channel blocks / 32-row tiles per split block were tried at level 4: 14.2 us against
        // 13.0 us for the unsplit <4,1> tile, so the split stays at one block, 16 rows)
        if (wf * NB <= 1024) return dense(1, 1, true);
        // mid levels, 3-4 channel blocks: 32-row split blocks load each weight fragment once per 32
        // rows instead of once per 16 (level 3, 46k rows x 48 ch: 22.0 -> 19.6 us; level 4, 11k x 64:
        // 13.9 -> 11.9 us); 64-row split blocks and 2-block layers lose (23.2 / 36.3 us)
        if (NB == 3 && wf >= 512 && wf < 8192) return dense(3, 2, true);
        if (NB == 4 && wf >= 512 && wf < 2048) return dense(4, 2, true);
    }
    if (NB == 1) return dense(1, wf >= 4096 ? 2 : 1, false);   // measured at M = 600k, 16 ch: S=2 51 us, S=4 56 us, S=1 56 us
    // level 2 (183k rows, 32 ch): bf16 <2,4> 27.7 us, <2,2> 30.2, <2,1> 35.0; fp32 98.8 / 93.6 / 92.8
    if (NB == 2) return wf >= 8192 ? dense(2, esz == 2 ? 4 : 2, false) : wf >= 2048 ? dense(2, 1, false) : dense(1, 1, false);
    // 48 channels: three channel blocks exactly (a <4,*> tile would load and multiply a zero block)
    if (NB == 3) return dense(wf >= 512 ? 3 : 1, 1, false);   // level 3 (46k rows): <3,1> 23.2 us, <4,1> 27.8, <3,2> 22.8 (fp32 74.6)
    // level 4 (11k rows, 64 ch): <4,1> 13.0 us, <2,1> 17.3, <2,2> 14.9
    if (NB == 4) return wf >= 8192 ? dense(4, 2, false) : dense(wf >= 512 ? 4 : 1, 1, false);
    return dense(wf >= 4096 ? 8 : wf >= 1024 ? 4 : wf >= 256 ? 2 : 1, 1, false);
}

// ---- The compiled set.  The launchers instantiate a kernel under `if constexpr` of these predicates and nothing else; each admits
// exactly the names plan_gather returns for its family (tests/test_gather_plan_host.py: admitted = built = swept = probed).
// conv_tile16 and conv_up32 exist for every (OUT32, STATS), conv_wlds48 for both STATS.
// The legal (NBW, S, SPLIT) triples of conv_fast; conv_gather takes the unsplit ones.  The set of triples defines what is compiled;
// their order only the order in which the compiler emits the kernels (the last entry first).  With this order every kernel's
// instruction stream equalled the one under the ladders this table replaced; another order may schedule a kernel differently.
template <int NBW_, int S_, bool SPLIT_> struct Shape { static constexpr int NBW = NBW_, S = S_; static constexpr bool SPLIT = SPLIT_; };
template <class... Sh> struct Shapes {};
typedef Shapes<Shape<8, 1, false>, Shape<4, 1, false>, Shape<4, 2, false>, Shape<3, 1, false>, Shape<2, 1, false>, Shape<2, 2, false>,
               Shape<2, 4, false>, Shape<1, 1, false>, Shape<1, 2, false>, Shape<3, 2, true>, Shape<4, 2, true>, Shape<1, 1, true>> FastShapes;
template <class... Sh>
constexpr bool listed(Shapes<Sh...>, int nbw, int s, bool split) { return ((Sh::NBW == nbw && Sh::S == s && Sh::SPLIT == split) || ...); }
// the triples dense() names for rows of `esz` bytes: two channel blocks from 8192 wave tiles on take <2, 2> in fp32 and <2, 4> in bf16
constexpr bool dense_shape(int esz, int nbw, int s, bool split) { return listed(FastShapes{}, nbw, s, split) && !(nbw == 2 && s == (esz == 2 ? 2 : 4)); }
constexpr bool generic_compiled(int esz, int nbw, int s, bool split) { return !split && dense_shape(esz, nbw, s, split); }
// conv_fast<policy, NBW, S, D, OUT32, SPLIT, STATS, PRE>, for both STATS.  OUT32 is fp32 output rows of a bf16 call.  The folded
// BatchNorm (PRE, PreArgs): 16-byte pieces of same-dtype rows (bf16 >= 32 channels, fp32), split blocks of 16 rows x one or 32
// rows x four channel blocks — the shapes of the coarse U-Net levels, where a BatchNorm sweep of its own is a launch-floor kernel
constexpr bool fast_compiled(int esz, GatherPolicy p, int nbw, int s, bool split, bool out32, int pre) {
    const bool policy = esz == 2 ? p != GP_F32_SPLIT : (p == GP_NARROW || p == GP_F32_SPLIT);
    const bool folded = pre >= 1 && pre <= 3 && split && ((nbw == 1 && s == 1) || (nbw == 4 && s == 2)) && !out32 &&
                        p == (esz == 2 ? GP_WIDE : GP_NARROW);
    return policy && dense_shape(esz, nbw, s, split) && !(out32 && esz == 4) && (pre == 0 || folded);
}
// conv_tile<MODE, OUT32, STATS, MAXNB, DUAL>: MODE 2 (fp32 rows) is always OUT32; the dual kernel (64-byte rows) serves 32 and 64
// output channels with MAXNB 2, and 64 with their statistics with MAXNB 4; without it a second channel block per pass exists only
// for the statistics
constexpr bool tile_compiled(int mode, bool out32, bool stats, int maxnb, bool dual) {
    return mode >= 0 && mode <= 2 && (mode != 2 || out32) &&
           (dual ? mode == 1 && (maxnb == 2 || (maxnb == 4 && stats)) : maxnb == 1 || (maxnb == 2 && stats));
}

// The instantiation as a kernel trace shows it, namespaces stripped; "none" for an error route.  Returns the length.
inline int route_name(const GatherRoute &r, char *buf, size_t n) {
    const auto b = [](bool v) { return v ? "true" : "false"; };
    static const char *const pol[2][4] = {{"PBF16", "PBF16W", "PBF16P", "PBF16"}, {"PF32", "PF32", "PF32", "PF32S"}};
    if (r.status != DODA_OK) return snprintf(buf, n, "none");
    switch (r.family) {
    case GF_GENERIC: return snprintf(buf, n, "conv_gather<%s, %d, %d>", r.esz == 4 ? "F32" : "BF16", r.NBW, r.S);
    case GF_FAST:
        return snprintf(buf, n, "conv_fast<%s, %d, %d, %d, %s, %s, %s, %d>", pol[r.esz == 4][r.policy], r.NBW, r.S, GP_RING_DEPTH,
                        b(r.out32), b(r.split), b(r.stats), r.pre);
    case GF_UP32: return snprintf(buf, n, "conv_up32<%s, %s>", b(r.out32), b(r.stats));
    case GF_TILE: return snprintf(buf, n, "conv_tile<%d, %s, %s, %d, %s>", r.mode, b(r.out32), b(r.stats), r.maxnb, b(r.dual));
    case GF_TILE16: return snprintf(buf, n, "conv_tile16<%s, %s>", b(r.out32), b(r.stats));
    case GF_WLDS48: return snprintf(buf, n, "conv_wlds48<%s>", b(r.stats));
    }
    return snprintf(buf, n, "none");
}

// Stand-alone driver of doda_amd/csrc/wgrad_plan.hpp for tests/test_wgrad_plan_host.py: one single-job list per line of stdin as
// `key=value` words (the job's fields; `sw.` + a field of WgradSwitches), one line of stdout per job:
//   class=<skip|zero|dense|pairs|tile|wide> route=<kernel> blocks=<b> R=<row chunks> rows_per_chunk=<r> partial_bytes=<workspace>
//   ta=<t> tb=<t> n_sa=<s> n_sb=<s> n_range=<r> n_og=<g> n_tag=<g> n_tbg=<g> direct=<0|1> wdma_blocks=<b> wdma_groups=<g>
// R and rows_per_chunk are the gather-table plan's (the wide class sums over the same chunks), 0 for the other classes.
// ta, tb: the slice shape of a wide job (ww_shape) or the channel blocks per wave of a pair job (pairs_geo); n_sa, n_sb: a wide
// job's slices per side; n_range .. direct: the other PairsGeo fields; wdma_blocks, wdma_groups: a tile job's 16 x 16 channel
// blocks and workgroups.  Each is 0 for the classes it does not describe.
// Absent keys: a bf16 16 -> 16 job of K = 27 offsets with a table, no tilebook and no pair lists, ld = n_a = n_rows, every
// operand 16-byte aligned (a_al, b_al, dw_al: address mod 16).  pairs=1: real lists with their counts and a segment prefix over
// n_a rows; pairs=2: identity lists.  The addresses are fake and never read.
// With the argument `--compiled`: no stdin; one line per instantiation that dense_compiled admits, as dense_name writes it, from a
// walk over the whole parameter grid.
// With the argument `--shapes`: no stdin; one line `wide <ta> <tb>` per entry of WW_SHAPES and one line `pairs <ta> <tb>` per entry
// of WP_PAIR_SHAPES, in the header's order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../doda_amd/csrc/wgrad_plan.hpp"

static void print_compiled() {
    for (int pol = WP_BF16; pol <= WP_F32S; ++pol)
        for (int ta = 0; ta <= 4; ++ta)
            for (int tb = 0; tb <= 4; ++tb)
                for (int ogw = 0; ogw <= 8; ++ogw)
                    for (int vok = 1; vok >= 0; --vok) {
                        if (!dense_compiled((WgradPolicy)pol, ta, tb, ogw)) continue;
                        DensePlan p{};
                        p.policy = (WgradPolicy)pol; p.TA = ta; p.TB = tb; p.OGW = ogw; p.vok = vok;
                        char name[64];
                        dense_name(p, name, sizeof name);
                        puts(name);
                    }
}

static void print_shapes() {
#define SHAPE_LINE(A, B) printf("wide %d %d\n", A, B);
    WW_SHAPES(SHAPE_LINE)
#undef SHAPE_LINE
#define SHAPE_LINE(A, B) printf("pairs %d %d\n", A, B);
    WP_PAIR_SHAPES(SHAPE_LINE)
#undef SHAPE_LINE
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--compiled")) { print_compiled(); return 0; }
    if (argc > 1 && !strcmp(argv[1], "--shapes")) { print_shapes(); return 0; }
    static const char *const cls_name[] = {"skip", "zero", "dense", "pairs", "tile", "wide"};
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        doda_wgrad_job j{};
        WgradSwitches sw;
        j.K = 27; j.ca = j.cb = 16; j.n_rows = 1; j.elem_bytes = 2;
        long long ld = -1, n_a = -1, pair_ld = -1, seg_nt = -1;
        int a_al = 0, b_al = 0, dw_al = 0, tilebook = 0, tbl = 1, pairs = 0, acc = 0;
        bool any = false;
        for (char *tok = strtok(line, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
            char *eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "bad word '%s'\n", tok); return 2; }
            *eq = 0;
            const long long v = atoll(eq + 1);
            any = true;
#define F(name, dst) if (!strcmp(tok, name)) { dst = (decltype(dst))v; continue; }
            F("K", j.K) F("ca", j.ca) F("cb", j.cb) F("n_rows", j.n_rows) F("esz", j.elem_bytes) F("ld", ld) F("n_a", n_a)
            F("a_al", a_al) F("b_al", b_al) F("dw_al", dw_al) F("tilebook", tilebook) F("tbl", tbl) F("pairs", pairs)
            F("pair_ld", pair_ld) F("seg_nt", seg_nt) F("acc", acc)
            F("sw.min_rows", sw.min_rows) F("sw.no33", sw.no33) F("sw.t33", sw.t33) F("sw.f32_split_rows", sw.f32_split_rows)
            F("sw.wdma_min_rows", sw.wdma_min_rows) F("sw.no_pairs", sw.no_pairs) F("sw.wdma", sw.wdma)
#undef F
            fprintf(stderr, "unknown key '%s'\n", tok);
            return 2;
        }
        if (!any) continue;
        const auto fake = [](uintptr_t at) { return (void *)at; };
        j.a = fake(0x10000000u + a_al); j.b = fake(0x20000000u + b_al); j.dw = (float *)fake(0x40000000u + dw_al);
        j.tbl = tbl ? (const int32_t *)fake(0x30000000u) : nullptr;
        j.tilebook = tilebook ? fake(0x90000000u) : nullptr;
        j.ld = ld >= 0 ? (int)ld : j.n_rows;
        j.n_a = n_a >= 0 ? (int)n_a : j.n_rows;
        j.flags = acc ? DODA_WGRAD_ACCUMULATE : 0;
        if (pairs) {
            j.pair_in = (const int32_t *)fake(0x50000000u); j.pair_out = (const int32_t *)fake(0x60000000u);
            j.pair_ld = pair_ld >= 0 ? (int)pair_ld : j.n_rows;
            if (pairs == 1) {
                j.pair_num = (const int32_t *)fake(0x70000000u); j.pair_seg = (const int32_t *)fake(0x80000000u);
                j.pair_seg_nt = seg_nt >= 0 ? (int)seg_nt : (j.n_a + 255) / 256;
            }
        }
        const int cls = classify(j, sw);
        char route[64] = "none";
        long long blocks = 0;
        size_t bytes = 0;
        DensePlan p{};
        int ta = 0, tb = 0, n_sa = 0, n_sb = 0, n_range = 0, n_og = 0, n_tag = 0, n_tbg = 0, direct = 0, blocks16 = 0, groups = 0;
        if (cls == J_DENSE || cls == J_WIDE) p = plan_dense(j, sw);
        if (cls == J_DENSE) {
            if (!dense_valid(j)) snprintf(route, sizeof route, "invalid");
            else {
                dense_name(p, route, sizeof route);
                blocks = p.blocks;
                bytes = dense_partial_bytes(p, j);
            }
        } else if (cls == J_PAIRS) {
            const PairsGeo g = pairs_geo(j);
            snprintf(route, sizeof route, "wgrad_pairs_kernel<%d, %d>", g.ta, g.tb);
            blocks = g.blocks;
            bytes = g.partial_bytes;
            ta = g.ta; tb = g.tb; n_range = g.n_range; n_og = g.n_og; n_tag = g.n_tag; n_tbg = g.n_tbg; direct = g.direct ? 1 : 0;
        } else if (cls == J_TILE) {
            snprintf(route, sizeof route, "wgrad_dma16");
            blocks = wdma_groups(j.n_rows);
            bytes = (size_t)wdma_blocks(j) * wdma_block_partial_bytes(j.n_rows);
            blocks16 = wdma_blocks(j); groups = wdma_groups(j.n_rows);
        } else if (cls == J_WIDE) {
            snprintf(route, sizeof route, "wgrad_wide");
            const WideGeo g = wwide_geo(j, sw);
            blocks = g.blocks;
            bytes = g.partial_bytes;
            ta = g.ta; tb = g.tb; n_sa = j.ca / (16 * g.ta); n_sb = j.cb / (16 * g.tb);
        }
        const bool chunks = (cls == J_DENSE && dense_valid(j)) || cls == J_WIDE;
        printf("class=%s route=%s blocks=%lld R=%d rows_per_chunk=%d partial_bytes=%zu ta=%d tb=%d n_sa=%d n_sb=%d n_range=%d n_og=%d "
               "n_tag=%d n_tbg=%d direct=%d wdma_blocks=%d wdma_groups=%d\n", cls_name[cls], route, blocks, chunks ? p.R : 0,
               chunks ? p.rows_per_chunk : 0, bytes, ta, tb, n_sa, n_sb, n_range, n_og, n_tag, n_tbg, direct, blocks16, groups);
    }
    return 0;
}

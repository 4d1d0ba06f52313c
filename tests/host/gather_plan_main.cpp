// Stand-alone driver of doda_amd/csrc/gather_plan.hpp for tests/test_gather_plan_host.py: one call per line of stdin as
// `key=value` words (fields of GatherCall, and of GatherSwitches with the prefix `sw.`), one line of stdout per call:
//   status=<s> route=<route_name> grid=<g> block=<b> parts=<n_part> frags=<pack fragments> wbytes=<pack bytes>
// Absent keys: a dense, aligned bf16 call with a large enough workspace, n_in = ld = n_out, no epilogue options; a prologue's
// operands all present, aligned and dense.
// With the argument `--compiled`: no stdin; one line per instantiation that the predicates of gather_plan.hpp admit, as route_name
// writes it, from a walk over the whole parameter grid.
// With the argument `--constants`: no stdin; the tilebook's constants (tilebook.hpp) as `name=value` lines, TB_BITMAP_BITS — the
// widest span of row numbers a tile may have and still take the builder's bitmap form — among them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../doda_amd/csrc/gather_plan.hpp"
#include "../../doda_amd/csrc/tilebook.hpp"

static void admit(bool yes, GatherRoute r) {
    if (!yes) return;
    char name[96];
    r.status = DODA_OK;
    route_name(r, name, sizeof name);
    puts(name);
}

static void print_compiled() {
    for (int esz = 2; esz <= 4; esz += 2)
        for (int nbw = 0; nbw <= 9; ++nbw)
            for (int s = 0; s <= 5; ++s)
                for (int split = 0; split < 2; ++split) {
                    GatherRoute r{};
                    r.esz = (uint8_t)esz; r.NBW = (uint8_t)nbw; r.S = (uint8_t)s; r.split = split;
                    r.family = GF_GENERIC;
                    admit(generic_compiled(esz, nbw, s, split), r);
                    r.family = GF_FAST;
                    for (int p = GP_NARROW; p <= GP_F32_SPLIT; ++p)
                        for (int o32 = 0; o32 < 2; ++o32)
                            for (int st = 0; st < 2; ++st)
                                for (int pre = -1; pre <= 4; ++pre) {
                                    r.policy = (GatherPolicy)p; r.out32 = o32; r.stats = st; r.pre = (uint8_t)pre;
                                    admit(fast_compiled(esz, r.policy, nbw, s, split, o32, pre), r);
                                }
                }
    for (int o32 = 0; o32 < 2; ++o32)
        for (int st = 0; st < 2; ++st) {
            GatherRoute r{};
            r.out32 = o32; r.stats = st;
            for (int mode = -1; mode <= 3; ++mode)
                for (int maxnb = 0; maxnb <= 5; ++maxnb)
                    for (int dual = 0; dual < 2; ++dual) {
                        r.family = GF_TILE; r.mode = (uint8_t)mode; r.maxnb = (uint8_t)maxnb; r.dual = dual;
                        admit(tile_compiled(mode, o32, st, maxnb, dual), r);
                    }
            r.family = GF_TILE16; admit(true, r);     // conv_tile16, conv_up32: every (OUT32, STATS); conv_wlds48: both STATS
            r.family = GF_UP32; admit(true, r);
            r.family = GF_WLDS48; admit(!o32, r);
        }
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--compiled")) { print_compiled(); return 0; }
    if (argc > 1 && !strcmp(argv[1], "--constants")) {
        printf("TB_T=%d\nTB_UMAX=%d\nTB_LMAX=%d\nTB_CAP64=%d\nTB_K=%d\nTB_LW=%d\nTB_BITMAP_BITS=%d\n", TB_T, TB_UMAX, TB_LMAX, TB_CAP64, TB_K, TB_LW,
               TB_BITMAP_BITS);
        printf("GP_TILE_MAX_GROUPS=%d\nGP_TILE16_GROUPS=%d\n", GP_TILE_MAX_GROUPS, GP_TILE16_GROUPS);
        return 0;
    }
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        GatherCall c{};
        GatherSwitches sw;
        c.K = 27; c.kc = 16; c.nc = 16; c.n_out = 1; c.esz = 2;
        c.ws_bytes = (size_t)-1;
        c.side = c.aux = c.add = c.saved = c.totals = c.running = c.affine = true;
        long long n_in = -1, ld = -1, pre_rows = -1, tb_rows = -1, side_ld = -1, aux_ld = -1, add_ld = -1;
        bool any = false;
        for (char *tok = strtok(line, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
            char *eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "bad word '%s'\n", tok); return 2; }
            *eq = 0;
            const long long v = atoll(eq + 1);
            any = true;
#define F(name, dst) if (!strcmp(tok, name)) { dst = (decltype(dst))v; continue; }
            F("K", c.K) F("kc", c.kc) F("nc", c.nc) F("n_out", c.n_out) F("esz", c.esz) F("n_in", n_in) F("ld", ld)
            F("out32", c.out32) F("layout", c.layout) F("packed", c.packed) F("ws_bytes", c.ws_bytes) F("x_al", c.x_al) F("y_al", c.y_al)
            F("x_ld", c.x_ld) F("y_ld", c.y_ld) F("res_ld", c.res_ld) F("bnx_ld", c.bnx_ld) F("res_bcast", c.res_bcast)
            F("stats", c.stats) F("pre_kind", c.pre_kind) F("pre_rows", pre_rows) F("side_ld", side_ld) F("aux_ld", aux_ld)
            F("add_ld", add_ld) F("side", c.side) F("aux", c.aux) F("add", c.add) F("saved", c.saved) F("totals", c.totals)
            F("running", c.running) F("affine", c.affine) F("tilebook", c.tilebook) F("tilebook_rows", tb_rows)
            F("sw.f32_split_rows", sw.f32_split_rows) F("sw.pre_small_blocks", sw.pre_small_blocks) F("sw.f32_conv_tile", sw.f32_conv_tile)
            F("sw.tile16_min_tiles", sw.tile16_min_tiles) F("sw.tile", sw.tile) F("sw.wlds", sw.wlds)
            F("sw.tile_pipeline", sw.tile_pipeline) F("sw.tile_dual", sw.tile_dual) F("sw.conv_up", sw.conv_up)
#undef F
            fprintf(stderr, "unknown key '%s'\n", tok);
            return 2;
        }
        if (!any) continue;
        c.n_in = n_in >= 0 ? n_in : c.n_out;
        c.ld = ld >= 0 ? (int)ld : c.n_out;
        c.pre_rows = pre_rows >= 0 ? pre_rows : c.n_in;
        c.tilebook_rows = tb_rows >= 0 ? (int)tb_rows : c.n_out;
        c.side_ld = (unsigned)(side_ld >= 0 ? side_ld : c.kc);
        c.aux_ld = (unsigned)(aux_ld >= 0 ? aux_ld : c.kc);
        c.add_ld = (unsigned)(add_ld >= 0 ? add_ld : c.kc);
        const GatherRoute r = plan_gather(c, sw);
        char name[96];
        route_name(r, name, sizeof name);
        printf("status=%d route=%s grid=%u block=%u parts=%d frags=%lld wbytes=%zu\n", r.status, name, r.grid, r.block, r.n_part,
               r.geo.frags, r.geo.bytes);
    }
    return 0;
}

// Stand-alone driver of doda_amd/csrc/gather_plan.hpp for tests/test_gather_plan_host.py: one call per line of stdin as
// `key=value` words (fields of GatherCall, and of GatherSwitches with the prefix `sw.`), one line of stdout per call:
//   status=<s> route=<route_name> grid=<g> block=<b> parts=<n_part> frags=<pack fragments> wbytes=<pack bytes>
// Absent keys: a dense, aligned bf16 call with a large enough workspace, n_in = ld = n_out, no epilogue options; a prologue's
// operands all present, aligned and dense.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../doda_amd/csrc/gather_plan.hpp"

int main() {
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

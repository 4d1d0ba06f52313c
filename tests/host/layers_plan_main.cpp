// Stand-alone driver of doda_amd/csrc/layers_plan.hpp (and of describe_gather, gather_plan.hpp) for tests/test_layers_plan_host.py.
// stdin, one record per line of `key=value` words; pointer fields are integers (0: null, else the address, looked at for its
// alignment only); absent keys are zero.
//   op <fields of doda_cx_op>            appends an op to the current list
//   run esz=<2|4> [n_ops=<n>] [null=1] [sw.<field of LayerSwitches>=..] [gsw.pre_small_blocks=..]
//                                        plans the list and clears it.  n_ops overrides the count; null=1 passes no array.
//       -> `list status=<s> steps=<n>` and, per step, `step first=<op> n=<ops> route=<kernel> grid=<g> block=<b> parts=<p>`
//          (grid / block of a `bn_fwd_totals` / `bn_bwd_totals` step are bn.hip's to choose: printed as 0)
//   gather <arguments of doda_spconv_gather_ex; epi=1 with e.<field of doda_conv_epilogue>; pre=1 with p.<field of doda_conv_prologue>>
//       -> `gather status=<s> n_out=<call.n_out> x_ld= y_ld= res_ld= bnx_ld= res_bcast= stats= pre_kind= route=<plan_gather's>`
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../doda_amd/csrc/layers_plan.hpp"

template <class T> static void put(T &dst, long long v) { dst = (T)v; }
template <class T> static void put(T *&dst, long long v) { dst = (T *)(uintptr_t)v; }
static void put(float &dst, long long) { dst = 0.f; }

// A step's launch as the traces of DODA_TRACE_GATHER / DODA_TRACE_BN name its kernel; the totals sweeps of bn.hip, whose kernel
// that entry point chooses, by their entry point ("bn_fwd_totals" / "bn_bwd_totals": not trace names).
static int step_name(const LayerStep &s, const doda_cx_op *ops, int esz, char *buf, size_t n) {
    switch (s.route) {
    case LR_GEMM: case LR_GEMM_FOLD: return route_name(s.gather, buf, n);
    case LR_LAY_BN: return snprintf(buf, n, "lay_bn<%d, %d>", esz, (int)s.kind);
    case LR_BN_TOTALS: return snprintf(buf, n, ops[s.first].kind == DODA_CX_BNFWD ? "bn_fwd_totals" : "bn_bwd_totals");
    case LR_LAY_STATS: return snprintf(buf, n, "lay_stats<%d>", esz);
    }
    return snprintf(buf, n, "none");
}

int main() {
    std::vector<doda_cx_op> ops;
    std::vector<LayerStep> steps;
    char line[8192];
    while (fgets(line, sizeof line, stdin)) {
        char *rec = strtok(line, " \t\r\n");
        if (!rec) continue;
        doda_cx_op o;
        memset(&o, 0, sizeof o);
        LayerSwitches sw;
        GatherSwitches gsw;
        long long esz = 2, n_ops = 1LL << 40, null_ops = 0;   // (n_ops: unset)
        doda_conv_epilogue e;
        doda_conv_prologue p;
        memset(&e, 0, sizeof e);
        memset(&p, 0, sizeof p);
        struct { const void *x, *y, *ws; const float *w; const int32_t *tbl; long long n_in, kc, esz, nc, ld, K, n_out, y_is_f32, w_layout, ws_bytes, epi, pre; } g;
        memset(&g, 0, sizeof g);
        for (char *tok = strtok(nullptr, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) {
            char *eq = strchr(tok, '=');
            if (!eq) { fprintf(stderr, "bad word '%s'\n", tok); return 2; }
            *eq = 0;
            const long long v = atoll(eq + 1);
#define F(name, dst) if (!strcmp(tok, name)) { put(dst, v); continue; }
            if (!strcmp(rec, "op")) {
                F("kind", o.kind) F("flags", o.flags) F("rows", o.rows) F("rows_in", o.rows_in) F("c_in", o.c_in) F("c_out", o.c_out)
                F("K", o.K) F("tbl_ld", o.tbl_ld) F("x_ld", o.x_ld) F("y_ld", o.y_ld) F("res_ld", o.res_ld) F("aux_ld", o.aux_ld)
                F("y2_ld", o.y2_ld) F("n_part", o.n_part) F("c_split", o.c_split) F("x", o.x) F("w", o.w) F("tbl", o.tbl) F("y", o.y)
                F("y2", o.y2) F("res", o.res) F("aux", o.aux) F("stats", o.stats) F("stats_b", o.stats_b) F("gamma", o.gamma)
                F("beta", o.beta) F("mean", o.mean) F("invstd", o.invstd) F("running_mean", o.running_mean)
                F("running_var", o.running_var) F("nbt", o.nbt) F("dgamma", o.dgamma) F("dbeta", o.dbeta) F("tilebook", o.tilebook)
                F("eps", o.eps) F("momentum", o.momentum)
            } else if (!strcmp(rec, "run")) {
                F("esz", esz) F("n_ops", n_ops) F("null", null_ops) F("sw.pre_fwd_rows", sw.pre_fwd_rows) F("sw.pre_bwd_rows", sw.pre_bwd_rows)
                F("sw.lay_bn_grid", sw.lay_bn_grid) F("sw.tuned_rows_bf16", sw.tuned_rows_bf16) F("gsw.pre_small_blocks", gsw.pre_small_blocks)
            } else if (!strcmp(rec, "gather")) {
                F("x", g.x) F("y", g.y) F("ws", g.ws) F("w", g.w) F("tbl", g.tbl) F("n_in", g.n_in) F("kc", g.kc) F("esz", g.esz) F("nc", g.nc)
                F("ld", g.ld) F("K", g.K) F("n_out", g.n_out) F("y_is_f32", g.y_is_f32) F("w_layout", g.w_layout) F("ws_bytes", g.ws_bytes)
                F("epi", g.epi) F("pre", g.pre)
                F("e.residual", e.residual) F("e.stats", e.stats) F("e.stats_rows_h", e.stats_rows_h) F("e.bn_x", e.bn_x)
                F("e.bn_mean", e.bn_mean) F("e.bn_invstd", e.bn_invstd) F("e.bn_gamma", e.bn_gamma) F("e.bn_beta", e.bn_beta)
                F("e.tilebook_rows", e.tilebook_rows) F("e.tilebook", e.tilebook) F("e.residual_bcast", e.residual_bcast)
                F("e.x_ld", e.x_ld) F("e.y_ld", e.y_ld) F("e.residual_ld", e.residual_ld) F("e.bn_x_ld", e.bn_x_ld)
                F("p.kind", p.kind) F("p.rows", p.rows) F("p.c_a", p.c_a) F("p.totals", p.totals) F("p.totals_b", p.totals_b)
                F("p.gamma", p.gamma) F("p.beta", p.beta) F("p.running_mean", p.running_mean) F("p.running_var", p.running_var)
                F("p.mean", p.mean) F("p.invstd", p.invstd) F("p.side", p.side) F("p.side_ld", p.side_ld) F("p.aux_ld", p.aux_ld)
                F("p.add_ld", p.add_ld) F("p.aux", p.aux) F("p.add", p.add) F("p.dgamma", p.dgamma) F("p.dbeta", p.dbeta)
            }
#undef F
            fprintf(stderr, "unknown key '%s' of record '%s'\n", tok, rec);
            return 2;
        }
        if (!strcmp(rec, "op")) { ops.push_back(o); continue; }
        if (!strcmp(rec, "gather")) {
            if (g.pre) e.prologue = &p;
            const GatherDescription d = describe_gather(g.x, (int32_t)g.n_in, (int32_t)g.kc, (int32_t)g.esz, g.w, (int32_t)g.nc, g.tbl, (int32_t)g.ld,
                                                        (int32_t)g.K, (int32_t)g.n_out, g.y, (int32_t)g.y_is_f32, (int32_t)g.w_layout, g.ws,
                                                        (size_t)g.ws_bytes, g.epi ? &e : nullptr);
            char name[96] = "none";
            if (d.status == DODA_OK && d.call.n_out) route_name(plan_gather(d.call, gsw), name, sizeof name);
            printf("gather status=%d n_out=%d x_ld=%u y_ld=%u res_ld=%u bnx_ld=%u res_bcast=%d stats=%d pre_kind=%d route=%s\n", d.status,
                   d.call.n_out, d.call.x_ld, d.call.y_ld, d.call.res_ld, d.call.bnx_ld, (int)d.call.res_bcast, (int)d.call.stats, d.call.pre_kind,
                   name);
            continue;
        }
        if (strcmp(rec, "run")) { fprintf(stderr, "unknown record '%s'\n", rec); return 2; }
        const int st = plan_layers(null_ops ? nullptr : ops.data(), n_ops != 1LL << 40 ? (int)n_ops : (int)ops.size(), (int)esz, sw, gsw, steps);
        printf("list status=%d steps=%zu\n", st, steps.size());
        for (const LayerStep &s : steps) {
            char name[96];
            step_name(s, ops.data(), (int)esz, name, sizeof name);
            const bool gemm = s.route == LR_GEMM || s.route == LR_GEMM_FOLD;
            printf("step first=%d n=%d route=%s grid=%u block=%u parts=%d\n", s.first, s.n_ops, name, gemm ? s.gather.grid : s.grid,
                   gemm ? s.gather.block : s.block, gemm ? s.gather.n_part : 0);
        }
        ops.clear();
    }
    return 0;
}

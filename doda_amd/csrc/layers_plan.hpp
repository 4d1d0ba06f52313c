// Plan of doda_layers_run: which launches an op list becomes — which BatchNorm ops ride in the next convolution's gather, which
// kernel every other op reaches, with which grid — decided for the WHOLE list in one pure host function before the first launch.
// doda_layers_run (layers.hip) plans, then walks the steps; a list with a defect anywhere is refused with nothing enqueued (no
// running statistics updated, no totals consumed, no parameter gradient accumulated by the ops in front of the defect).
// Plain C++17, no HIP header: tests/host/layers_plan_main.cpp compiles it with g++ and tests/test_layers_plan_host.py sweeps it.
#pragma once
#include <string.h>
#include <vector>
#include "bn_totals.hpp"
#include "gather_plan.hpp"

constexpr int LAY_BLOCK = 256;                    // threads of lay_bn / lay_stats
constexpr int LAY_MAX_C = 256;                    // spconv_common.hpp PRE_MAX_C: the LDS channel vectors of lay_bn
constexpr long long LAY_PRE_FWD_ROWS = 16384;     // defaults of LayerSwitches: measurements in layers.hip
constexpr long long LAY_PRE_BWD_ROWS = 0;
constexpr long long LAY_BN_GRID = 2048;
constexpr long long LAY_TUNED_ROWS_BF16 = 32768;
// fp32: bn.hip's sweeps have the operation order of lay_bn / the folded gather, so they take over where they are faster; bf16:
// bn.hip rounds in a different order than the fused-multiply-add form of pre_piece, so only above any fold limit, where "folded
// == unfolded" has nothing to compare (the finest levels, where the sweep is an HBM-bound kernel)
constexpr long long LAY_TUNED_ROWS_F32 = 4096;
constexpr int LAY_STATS_ROWS_PER_LANE = 8;
constexpr int LAY_STATS_GRID = 1024;
constexpr int LAY_STATS_MAX_C = 1024;
constexpr int LAY_FOLD_MIN_C_BF16 = 32;           // a folded BatchNorm works on 16-byte pieces of wide-packed bf16 rows

// The row thresholds of the list; one process-wide instance (layers.hip), filled from the environment once.
struct LayerSwitches {
    long long pre_fwd_rows = LAY_PRE_FWD_ROWS;    // DODA_PRE_FWD_ROWS, DODA_OPT_PRE_FWD_ROWS: a BNFWD op of at most this many rows may fold
    long long pre_bwd_rows = LAY_PRE_BWD_ROWS;    // DODA_PRE_BWD_ROWS, DODA_OPT_PRE_BWD_ROWS: the same for BNBWD (0: never)
    long long lay_bn_grid = LAY_BN_GRID;          // DODA_LAY_BN_GRID: most workgroups of lay_bn
    long long tuned_rows_bf16 = LAY_TUNED_ROWS_BF16;   // DODA_LAY_TUNED_ROWS: rows from which a dense bf16 BatchNorm op takes bn.hip's sweeps
};

enum LayerRoute : uint8_t {
    LR_GEMM,          // doda_spconv_gather_ex's route `gather`
    LR_GEMM_FOLD,     // the same with ops[first] (a BatchNorm op) as the prologue of ops[first + 1]
    LR_LAY_BN,        // lay_bn<esz, kind>
    LR_BN_TOTALS,     // doda_bn_relu_fwd_totals / doda_bn_relu_bwd_totals (bn.hip chooses the sweep's grid)
    LR_LAY_STATS      // lay_stats<esz>
};
struct LayerStep {
    int first, n_ops;             // ops[first .. first + n_ops): 2 for a fold
    LayerRoute route;
    uint8_t kind;                 // LR_LAY_BN: the KIND of lay_bn (1 forward, 2 backward, 3 backward + skip gradient)
    unsigned grid, block;         // LR_LAY_BN, LR_LAY_STATS
    GatherCall call;              // the two GEMM routes
    GatherRoute gather;
};

inline bool lay_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool lay_chan_ok(int c, int esz) { return c > 0 && c <= LAY_MAX_C && c % (16 / esz) == 0; }
// columns a BatchNorm op's first producer (BNFWD: `stats`) / first output (BNBWD: `y`) covers
inline int lay_split(const doda_cx_op &o) { return o.c_split > 0 && o.c_split < o.c_in ? o.c_split : o.c_in; }

// The doda_spconv_gather_ex call of a GEMM op, with the BatchNorm op `bn` (or null) folded into its gather: the epilogue and
// prologue structs the call takes.  *x: the rows the call gathers.  (The plan describes this call; the launch loop issues it.)
inline void gemm_call(const doda_cx_op &o, const doda_cx_op *bn, doda_conv_epilogue *ep, doda_conv_prologue *q, int32_t *stats_rows_h,
                      const void **x) {
    memset(ep, 0, sizeof(*ep));
    ep->residual = o.res;
    ep->residual_ld = o.res ? o.res_ld : 0;
    ep->x_ld = o.x_ld;
    ep->y_ld = o.y_ld;
    ep->tilebook = o.tilebook;
    ep->tilebook_rows = o.tilebook ? o.rows : 0;
    if (o.stats) {
        ep->stats = (float *)o.stats;             // (non-NULL selects the statistics epilogue; the sums go to the totals)
        ep->stats_totals = (double *)o.stats;
        ep->stats_rows_h = stats_rows_h;
        if (o.aux) {
            ep->bn_x = o.aux; ep->bn_x_ld = o.aux_ld;
            ep->bn_mean = o.mean; ep->bn_invstd = o.invstd; ep->bn_gamma = o.gamma; ep->bn_beta = o.beta;
            ep->bn_relu = (o.flags & DODA_CX_F_RELU) ? 1 : 0;
        }
    }
    *x = o.x;
    if (!bn) return;
    memset(q, 0, sizeof(*q));
    const bool fwd = bn->kind == DODA_CX_BNFWD;
    q->kind = fwd ? 1 : (bn->res ? 3 : 2);
    q->relu = (bn->flags & DODA_CX_F_RELU) ? 1 : 0;
    q->rows = bn->rows;
    q->eps = bn->eps; q->momentum = bn->momentum;
    q->gamma = bn->gamma; q->beta = bn->beta;
    q->mean = bn->mean; q->invstd = bn->invstd;
    q->side = bn->y; q->side_ld = bn->y_ld;
    if (fwd) {
        if (bn->flags & DODA_CX_F_TRAINING) {
            const int split = lay_split(*bn);
            q->totals = (const double *)bn->stats;
            q->totals_b = split < bn->c_in ? (const double *)bn->stats_b : nullptr;
            q->c_a = split;
            q->num_batches_tracked = bn->nbt;
        }
        q->running_mean = bn->running_mean; q->running_var = bn->running_var;
    } else {
        q->totals = (const double *)bn->stats;
        q->aux = bn->aux; q->aux_ld = bn->aux_ld;
        q->add = bn->res; q->add_ld = bn->res ? bn->res_ld : 0;
        q->dgamma = bn->dgamma; q->dbeta = bn->dbeta;
        q->accumulate = (bn->flags & DODA_CX_F_ACCUM) ? 1 : 0;
    }
    ep->prologue = q;
    *x = bn->x;                 // the conv gathers the BatchNorm's INPUT rows
    ep->x_ld = bn->x_ld;
}

// may the BatchNorm op b ride in the gather of g, the op behind it?  (Whether the folded kernels take the shape: plan_gather.)
inline bool lay_foldable(const doda_cx_op &b, const doda_cx_op &g, int esz, long long max_rows) {
    if (g.kind != DODA_CX_GEMM || g.x != b.y || g.x_ld != b.y_ld || g.c_in != b.c_in || g.rows_in != b.rows || b.rows > max_rows ||
        b.y_ld != b.c_in)   // (the side output is the weight gradient's dense operand)
        return false;
    if (b.kind == DODA_CX_BNBWD && lay_split(b) < b.c_in) return false;   // two outputs: its own launch
    if (esz == 2 && b.c_in < LAY_FOLD_MIN_C_BF16) return false;
    return lay_chan_ok(b.c_in, esz);
}

// A GEMM op (with `bn` folded): the status of the call and, for DODA_OK, its description and route in *s.
inline int plan_gemm(const doda_cx_op &o, const doda_cx_op *bn, int esz, const GatherSwitches &gsw, LayerStep *s) {
    if (!o.x || !o.w || !o.y || !o.tbl) return DODA_ERR_INVALID;
    doda_conv_epilogue ep;
    doda_conv_prologue q;
    int32_t stats_rows = 0;
    const void *x;
    gemm_call(o, bn, &ep, &q, &stats_rows, &x);
    const GatherDescription d = describe_gather(x, o.rows_in, o.c_in, esz, (const float *)o.w, o.c_out, o.tbl, o.tbl_ld, o.K, o.rows, o.y, 0,
                                                0x100, nullptr, 0, &ep);
    if (d.status != DODA_OK) return d.status;
    s->call = d.call;
    s->gather = GatherRoute{};
    if (d.call.n_out != 0) s->gather = plan_gather(d.call, gsw);   // (no output rows: the call returns DODA_OK, nothing launched)
    return s->gather.status;
}

// A BatchNorm op on its own: lay_bn, or bn.hip's register-resident sweeps for dense ops of many rows.
inline int plan_bn(const doda_cx_op &o, int esz, const LayerSwitches &sw, LayerStep *s) {
    const bool fwd = o.kind == DODA_CX_BNFWD, training = (o.flags & DODA_CX_F_TRAINING) != 0;
    const int c = o.c_in, split = lay_split(o), va = 16 / esz;
    if (fwd) {
        if (training ? (!o.stats || (split < c && !o.stats_b) || !o.mean || !o.invstd || split % 4) : (!o.running_mean || !o.running_var))
            return DODA_ERR_INVALID;
        if (!o.gamma || !o.beta || !o.y) return DODA_ERR_INVALID;
    } else if (!o.stats || !o.gamma || !o.beta || !o.mean || !o.invstd || !o.aux || !o.y || !o.dgamma || !o.dbeta)
        return DODA_ERR_INVALID;
    if (!lay_chan_ok(c, esz) || !o.x || o.x_ld % va || o.y_ld % va || !lay_al16(o.x) || !lay_al16(o.y)) return DODA_ERR_UNSUPPORTED;
    const long long tuned = esz == 4 ? LAY_TUNED_ROWS_F32 : sw.tuned_rows_bf16;
    s->route = LR_LAY_BN;
    if (fwd) {
        if (o.y_ld < c || o.x_ld < c) return DODA_ERR_INVALID;
        s->kind = 1;
        if (training && o.x_ld == c && o.y_ld == c && o.rows >= tuned) {
            s->route = LR_BN_TOTALS;
            return bn_fwd_totals_status(o.x, o.rows, c, esz, (const double *)o.stats, split < c ? (const double *)o.stats_b : nullptr, split,
                                        o.gamma, o.beta, o.running_mean, o.running_var, o.y, o.mean, o.invstd);
        }
    } else {
        if (split % va || (split < c && (!o.y2 || o.y2_ld % va || !lay_al16(o.y2))) || o.aux_ld % va || !lay_al16(o.aux) ||
            (o.res && (o.res_ld % va || !lay_al16(o.res))))
            return DODA_ERR_UNSUPPORTED;
        s->kind = o.res ? 3 : 2;
        if (split == c && o.x_ld == c && o.y_ld == c && o.aux_ld == c && !(o.flags & DODA_CX_F_ACCUM) && o.rows >= tuned) {
            s->route = LR_BN_TOTALS;
            return bn_bwd_totals_status(o.aux, o.x, o.rows, c, esz, (const double *)o.stats, o.mean, o.invstd, o.gamma, o.beta, o.res,
                                        o.res ? o.res_ld : 0, o.y, o.dgamma, o.dbeta);
        }
    }
    const int ppr = c / va, rpb = LAY_BLOCK / ppr;              // (c <= LAY_MAX_C = 256: ppr <= 64)
    long long grid = ((long long)o.rows + rpb - 1) / rpb;       // one row per thread, then four
    if (grid > sw.lay_bn_grid) grid = sw.lay_bn_grid;
    if (grid < 1) grid = 1;
    s->grid = (unsigned)grid; s->block = LAY_BLOCK;
    return DODA_OK;
}

inline int plan_stats(const doda_cx_op &o, LayerStep *s) {
    if (!o.x || !o.stats || o.c_in % 4 || o.c_in <= 0 || o.c_in > LAY_STATS_MAX_C || o.x_ld % 4 || o.x_ld < o.c_in) return DODA_ERR_INVALID;
    const int nf = o.c_in / 4, rpb = LAY_BLOCK / nf > 0 ? LAY_BLOCK / nf : 1;
    const long long per = (long long)rpb * LAY_STATS_ROWS_PER_LANE;
    long long grid = ((long long)o.rows + per - 1) / per;
    if (grid > LAY_STATS_GRID) grid = LAY_STATS_GRID;
    if (grid < 1) grid = 1;
    s->route = LR_LAY_STATS;
    s->grid = (unsigned)grid; s->block = LAY_BLOCK;
    return DODA_OK;
}

// The steps of a list, or the status of the first op that cannot run (then no steps).  Ops of no rows give no step.
inline int plan_layers(const doda_cx_op *ops, int n_ops, int esz, const LayerSwitches &sw, const GatherSwitches &gsw,
                       std::vector<LayerStep> &steps) {
    steps.clear();
    if (n_ops == 0) return DODA_OK;
    if (n_ops < 0 || !ops || (esz != 2 && esz != 4)) return DODA_ERR_INVALID;
    for (int k = 0; k < n_ops; ++k) {
        const doda_cx_op &o = ops[k];
        int st = DODA_ERR_INVALID;
        if (o.rows < 0 || o.n_part != 0) { steps.clear(); return st; }   // (n_part != 0: a list built for the executor's partial rows)
        if (o.rows == 0) continue;
        steps.emplace_back();              // (planned in place: a step carries a GatherCall and a GatherRoute)
        LayerStep &s = steps.back();
        s.first = k; s.n_ops = 1;
        switch (o.kind) {
        case DODA_CX_GEMM:
            s.route = LR_GEMM;
            st = plan_gemm(o, nullptr, esz, gsw, &s);
            break;
        case DODA_CX_BNFWD:
        case DODA_CX_BNBWD:
            st = DODA_ERR_UNSUPPORTED;
            if (k + 1 < n_ops && lay_foldable(o, ops[k + 1], esz, o.kind == DODA_CX_BNFWD ? sw.pre_fwd_rows : sw.pre_bwd_rows)) {
                s.route = LR_GEMM_FOLD; s.n_ops = 2;
                st = plan_gemm(ops[k + 1], &o, esz, gsw, &s);
            }
            if (st == DODA_ERR_UNSUPPORTED) {   // no fold, or a shape the folded kernels do not take: a launch of its own
                s.n_ops = 1;
                st = plan_bn(o, esz, sw, &s);
            }
            break;
        case DODA_CX_STATS:
            st = plan_stats(o, &s);
            break;
        default:
            break;
        }
        if (st != DODA_OK) { steps.clear(); return st; }
        k += s.n_ops - 1;
    }
    return DODA_OK;
}

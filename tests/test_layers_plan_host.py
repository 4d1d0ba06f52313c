"""doda_amd/csrc/layers_plan.hpp on the CPU: doda_layers_run plans its whole op list in one pure host function before the first
launch, so which launches a list becomes — folds, kernels, grids — and which status a defective list returns, with zero steps, is
checked without a GPU.  A stand-alone program (tests/host/layers_plan_main.cpp, g++ -Wall -Wextra -Werror, once more with
-fsanitize=address,undefined) answers for the probe set of tools/layersplan.py: every threshold from both sides, the lists of
tests/test_gpu_layers.py at its smallest shapes — asserted against tests/data/layers_plan_parent.json, the traces recorded on an
MI355X from the code that decided while it launched — and for tables of defects whose statuses are read off that code (the line
numbers in the tables are those of the commit the record was taken at)."""
import importlib.util
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))      # (its expected() imports tools/bnnumerics.py)
    spec = importlib.util.spec_from_file_location("layersplan", os.path.join(ROOT, "tools", "layersplan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lp = _tool()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def planner(request, tmp_path_factory):
    return lp.planner(str(tmp_path_factory.mktemp("layers_plan") / ("plan_" + request.param)), request.param == "sanitized")


@pytest.fixture(scope="module")
def host_lists():
    return lp.host_lists()


@pytest.fixture(scope="module")
def planned(planner, host_lists):
    """{probe name: (op list, esz, answer)} of the whole probe set"""
    got = planner([l for _, _, _, text in host_lists for l in text])
    return {name: (lst, esz, g) for (name, esz, lst, _), g in zip(host_lists, got)}


def _routes(planned, name):
    lst, esz, g = planned[name]
    assert g["status"] == OK, (name, g)
    return [(s["first"], s["n"], s["route"], s["grid"]) for s in g["steps"]]


def test_every_threshold_from_both_sides(planned):
    fold = {2: "conv_fast<PBF16W, 1, 1, 3, false, true, false, %d>", 4: "conv_fast<PF32, 1, 1, 3, false, true, false, %d>"}
    for esz, t in ((2, "bf16"), (4, "fp32")):
        R = lambda name: _routes(planned, "%s_%s" % (name, t))
        kinds = lambda name: [(f, n, re.match(r"[\w]+(<%d, \d>)?" % esz, r).group(0)) for f, n, r, _ in R(name)]
        # forward fold: DODA_PRE_FWD_ROWS = 16384 rows and one more
        assert [(f, n, r) for f, n, r, _ in R("fwd_fold_rows_16384")] == [(0, 2, fold[esz] % 1)]
        assert kinds("fwd_fold_rows_16385") == [(0, 1, "lay_bn<2, 1>" if esz == 2 else "bn_fwd_totals"), (1, 1, "conv_fast")]
        # backward fold: never at the default 0; both sides of 4096
        assert kinds("bwd_fold_default") == [(0, 1, "lay_bn<%d, 2>" % esz if esz == 2 else "bn_bwd_totals"), (1, 1, "conv_fast")]
        assert [(f, n, r) for f, n, r, _ in R("bwd_fold_rows_4096")] == [(0, 2, fold[esz] % 2)]
        assert [s[1] for s in R("bwd_fold_rows_4097")] == [1, 1]
        # the tuned sweeps of bn.hip: from 32768 rows (bf16) / 4096 rows (fp32), and each of their other conditions turned off once
        tuned = 32768 if esz == 2 else 4096
        assert kinds("tuned_fwd_%d" % (tuned - 1)) == [(0, 1, "lay_bn<%d, 1>" % esz)] and kinds("tuned_fwd_%d" % tuned) == [(0, 1, "bn_fwd_totals")]
        assert kinds("tuned_bwd_%d" % (tuned - 1)) == [(0, 1, "lay_bn<%d, 3>" % esz)] and kinds("tuned_bwd_%d" % tuned) == [(0, 1, "bn_bwd_totals")]
        for name, kind in (("x_strided", 1), ("y_strided", 1), ("eval", 1), ("split", 2), ("accum", 2), ("aux_strided", 2)):
            assert kinds("tuned_off_" + name) == [(0, 1, "lay_bn<%d, %d>" % (esz, kind))], name
        # lay_bn's grid: ceil(rows / rows per workgroup) up to 2048 workgroups
        for c in (32, 256):
            rpb = 256 // (c // (16 // esz))
            assert [R("lay_bn_cap_%d_%d" % (c, n))[0][3] for n in (2047 * rpb, 2048 * rpb, 2048 * rpb + 1)] == [2047, 2048, 2048]
        assert [R("lay_stats_cap_%d" % n)[0][3] for n in (1023 * 256, 1024 * 256, 1024 * 256 + 1)] == [1023, 1024, 1024]
        # a folded BatchNorm needs 16-byte pieces of wide-packed rows: bf16 from 32 channels, fp32 from 4
        assert [len(R("fold_channels_%d" % c)) for c in (16, 24, 32)] == ([2, 2, 1] if esz == 2 else [1, 1, 1])
        assert len(R("bn_channels_256")) == 2 and planned["bn_channels_264_" + t][2] == dict(status=UNSUPPORTED, steps=[], n_steps=0)
        # one list per clause of the fold rule that says no
        for name in ("other_x", "rows_in", "side_strided", "c_in", "x_ld", "split_bwd"):
            assert [s[1] for s in R("nofold_" + name)] == [1, 1], name
        assert kinds("nofold_next_is_bn") == [(k, 1, "lay_bn<%d, 1>" % esz) for k in (0, 1)] and kinds("nofold_last_op") == [(0, 1, "lay_bn<%d, 1>" % esz)]


def test_fold_falls_back_to_two_launches_where_the_folded_kernels_refuse(planned):
    """30 output channels: the folded plan is DODA_ERR_UNSUPPORTED (no fast kernel), fp32 takes the BatchNorm's own launch and the
    generic kernel; bf16 has no generic kernel for wide-packed weights, so the list is refused."""
    assert [(s[1], s[2]) for s in _routes(planned, "fold_fallback_fp32")] == [(1, "lay_bn<4, 1>"), (1, "conv_gather<F32, 1, 1>")]
    assert planned["fold_fallback_bf16"][2] == dict(status=UNSUPPORTED, steps=[], n_steps=0)


def test_a_tilebook_reaches_the_tile_kernels_and_a_fold_ignores_it(planned):
    """An op's tilebook goes into the call's description with the op's rows: the LDS-staged kernels for 16 / 32 input channels
    (fp32: 16), conv_fast where the tile kernels do not take the rows, and the folded gather in front of a tilebook."""
    first = lambda name: _routes(planned, name)[0][2]
    assert first("tile_16_bf16").startswith("conv_tile<0,") and first("tile_32_bf16").startswith("conv_tile<1,")
    assert first("tile_16_fp32").startswith("conv_tile<2,") and first("tile_32_fp32").startswith("conv_fast<PF32,")
    for t, pol in (("bf16", "PBF16W"), ("fp32", "PF32")):
        assert [(s[1], s[2].split(",")[0]) for s in _routes(planned, "tile_fold_32_" + t)] == [(2, "conv_fast<" + pol)]


def test_steps_are_the_launches_recorded_before_the_plan(planned):
    """tests/data/layers_plan_parent.json (tools/layersplan.py --record on an MI355X, at the commit before the plan): per probe the
    status, the launch count and the trace lines of DODA_TRACE_GATHER / DODA_TRACE_BN.  The plan's steps name exactly those
    launches, kernel, grid and block (and statistics rows), in order.  A refused list has the recorded status — and no step, where
    the recorded code had launched the ops in front of the defect."""
    record = json.load(open(os.path.join(ROOT, "tests", "data", "layers_plan_parent.json")))["probes"]
    assert [r["name"] for r in record] == list(planned)
    refused = 0
    for r in record:
        lst, esz, g = planned[r["name"]]
        assert g["status"] == r["status"], (r["name"], g)
        if r["status"] != OK:
            assert g["steps"] == []
            refused += 1
            continue
        assert r["launches"] == len(g["steps"]) == len(lp.launched(r["trace"])), (r["name"], g, r)
        assert lp.expected(lst, esz, g["steps"]) == lp.parse_trace(r["trace"]), (r["name"], g, r)
    assert refused == 3 and len(record) >= 120


# ---- atomic errors: a valid list of seven ops with a fold; each defect inserted as ops of its own in front, in the middle, at the end.
# `status`: what the code that decided while it launched returned for the defective op (layers.hip / spconv_gather.hip / bn.hip @ a917f1b)
def _valid(A):
    x = A.feat(300, 32)
    b = lp.bnfwd(A, 300, 32, x=x)
    u = A.feat(300, 32)
    g1 = lp.gemm(A, 300, 32, 32, A.feat(300, 32), layout=2, aux=u, flags=lp.F_RELU)
    bb = lp.bnbwd(A, 300, 32, x=g1["y"], aux=u, stats=g1["stats"])
    return [lp.stats(A, x, 32), b, lp.gemm(A, 300, 32, 32, b["y"]), g1, bb, lp.gemm(A, 300, 32, 32, bb["y"], layout=2),
            lp.bnfwd(A, 300, 32, training=False)]


def _off(t, elems=1):
    """the tensor's address moved by `elems` elements (a misaligned operand)"""
    return t.view(-1)[elems:]


def _defects(A):
    fwd = lambda **kw: [dict(lp.bnfwd(A, 300, 32), **kw)]
    ev = lambda **kw: [dict(lp.bnfwd(A, 300, 32, training=False), **kw)]
    bwd = lambda **kw: [dict(lp.bnbwd(A, 300, 32, res=A.feat(300, 32)), **kw)]
    bwd2 = lambda **kw: [dict(lp.bnbwd(A, 300, 32, split=16), **kw)]
    st = lambda **kw: [dict(lp.stats(A, A.feat(300, 32), 32), **kw)]
    gm = lambda **kw: [dict(lp.gemm(A, 300, 32, 32, A.feat(300, 48)[:, :32], res=A.feat(300, 32), aux=A.feat(300, 32)), **kw)]
    big = lambda f, **kw: [dict(f(A, 32768, 32), **kw)]       # the tuned sweeps' row count (bf16)

    def pair(bwd_=False, **kw):     # a BatchNorm op and the convolution it folds into
        l = lp.fold_pair(A, 300, 32, bwd=bwd_, **({"res": A.feat(300, 32)} if bwd_ else {}))
        l[0].update(kw)
        return l
    D = [   # main loop
        ("rows<0", st(rows=-1), INVALID),                       # layers.hip:304
        ("n_part", st(n_part=1), INVALID),                      # :304
        ("kind 0", st(kind=0), INVALID), ("kind 5", st(kind=5), INVALID),   # :326
        # pre_of
        ("fwd !stats", fwd(stats=None), INVALID), ("fwd !stats_b", fwd(c_split=16), INVALID), ("fwd !mean", fwd(mean=None), INVALID),
        ("fwd !invstd", fwd(invstd=None), INVALID), ("fwd split%4", fwd(c_split=18, stats_b=A.totals(16)), INVALID),   # :116
        ("eval !running_mean", ev(running_mean=None), INVALID), ("eval !running_var", ev(running_var=None), INVALID),   # :123
        ("fwd !gamma", fwd(gamma=None), INVALID), ("fwd !beta", fwd(beta=None), INVALID), ("fwd !y", fwd(y=None), INVALID),   # :131
    ] + [("bwd !" + k, bwd(**{k: None}), INVALID) for k in ("stats", "gamma", "beta", "mean", "invstd", "aux", "y", "dgamma", "dbeta")] + [  # :143
        # run_bn
        ("bn c=0", fwd(c_in=0, c_split=0), UNSUPPORTED),
        ("bn c=264", fwd(c_in=264, x_ld=264, y_ld=264, c_split=264), UNSUPPORTED), ("bn c=36", fwd(c_in=36, c_split=36, x_ld=40, y_ld=40), UNSUPPORTED),
        ("bn !x", fwd(x=None), UNSUPPORTED), ("bn x_ld%8", fwd(x_ld=36), UNSUPPORTED), ("bn y_ld%8", fwd(y_ld=36), UNSUPPORTED),
        ("bn x&15", fwd(x=_off(A.feat(301, 32))), UNSUPPORTED), ("bn y&15", fwd(y=_off(A.feat(301, 32))), UNSUPPORTED),   # :177
        ("fwd y_ld<c", fwd(y_ld=24), INVALID), ("fwd x_ld<c", fwd(x_ld=24), INVALID),   # :179
        ("bwd split%8", bwd2(c_split=4), UNSUPPORTED), ("bwd !y2", bwd2(y2=None), UNSUPPORTED), ("bwd y2_ld%8", bwd2(y2_ld=20), UNSUPPORTED),
        ("bwd y2&15", bwd2(y2=_off(A.feat(301, 16))), UNSUPPORTED), ("bwd aux_ld%8", bwd(aux_ld=36), UNSUPPORTED),
        ("bwd aux&15", bwd(aux=_off(A.feat(301, 32))), UNSUPPORTED), ("bwd res_ld%8", bwd(res_ld=36), UNSUPPORTED),
        ("bwd res&15", bwd(res=_off(A.feat(301, 32))), UNSUPPORTED),   # :190-192
        # the totals entry points behind run_bn (bn.hip): what their checks can still meet
        ("tuned fwd rm without rv", big(lp.bnfwd, running_var=None), INVALID),   # bn.hip:1088
        ("tuned bwd res_ld<c", big(lp.bnbwd, res=A.feat(32768, 32), res_ld=24), INVALID),   # bn.hip:1101
        # run_stats
        ("stats !x", st(x=None), INVALID), ("stats !stats", st(stats=None), INVALID), ("stats c%4", st(c_in=30), INVALID),
        ("stats c=0", st(c_in=0), INVALID), ("stats c>1024", st(c_in=1028, x_ld=1028), INVALID), ("stats x_ld%4", st(x_ld=34), INVALID),
        ("stats x_ld<c", st(x_ld=28), INVALID),   # :200
        # run_gemm
    ] + [("gemm !" + k, gm(**{k: None}), INVALID) for k in ("x", "w", "y", "tbl")] + [   # :214
        # doda_spconv_gather_ex behind run_gemm
        ("gemm c_in=0", gm(c_in=0), INVALID), ("gemm c_out=0", gm(c_out=0), INVALID), ("gemm K=0", gm(K=0), INVALID),
        ("gemm tbl_ld<rows", gm(tbl_ld=299), INVALID),   # spconv_gather.hip:1044
        ("gemm K=28", gm(K=28), UNSUPPORTED), ("gemm c_out>4096", gm(c_out=4100, y_ld=4100, res_ld=4100, aux_ld=4100), UNSUPPORTED),
        ("gemm c_in>4096", gm(c_in=4100, x_ld=4100), UNSUPPORTED),   # :1050
    ] + [("gemm !" + k, gm(**{k: None}), INVALID) for k in ("mean", "invstd", "gamma", "beta")] + [   # :1151
        ("gemm x_ld<0", gm(x_ld=-48), INVALID), ("gemm y_ld<0", gm(y_ld=-32), INVALID), ("gemm res_ld<0", gm(res_ld=-32), INVALID),
        ("gemm aux_ld<0", gm(aux_ld=-32), INVALID),   # :1161
        ("gemm x_ld<c_in", gm(x_ld=24), INVALID), ("gemm y_ld<c_out", gm(y_ld=24), INVALID), ("gemm res_ld<c_out", gm(res_ld=24), INVALID),
        ("gemm aux_ld<c_out", gm(aux_ld=24), INVALID),   # :1164
        # plan_gather: statistics, strides and aligned operands need the fast kernel
        ("gemm c_out%4", gm(c_out=30), UNSUPPORTED), ("gemm x&15", gm(x=_off(A.feat(301, 48))), UNSUPPORTED),
        ("gemm y&15", gm(y=_off(A.feat(301, 32))), UNSUPPORTED), ("gemm y_ld%4", gm(y_ld=34), UNSUPPORTED),   # gather_plan.hpp:112-114 @ a917f1b
        # the folded call: its prologue's checks refuse what the BatchNorm's own launch would have taken
        ("fold rm without rv", pair(running_var=None), INVALID),   # spconv_gather.hip:1175
        ("fold aux_ld<c", pair(True, aux_ld=24), INVALID), ("fold add_ld<c", pair(True, res_ld=24), INVALID),   # :1173-1174
    ]
    return D


def test_a_defect_anywhere_refuses_the_list_with_no_step(planner):
    A = lp.Alloc(2, lp.torch.device("cpu"))
    valid = _valid(A)
    pre = (16384, 16384)
    base = planner(lp.lines(valid, 2, pre))[0]
    assert base["status"] == OK and [s["n"] for s in base["steps"]] == [1, 2, 1, 2, 1] and len(valid) >= 6
    defects = _defects(A)
    assert len(defects) == 80
    text = []
    for _, ops, _ in defects:
        for pos in (0, 3, len(valid)):       # first, middle (between two steps), last
            text += lp.lines(valid[:pos] + ops + valid[pos:], 2, pre)
    got = planner(text)
    for k, (name, _, status) in enumerate(defects):
        for g in got[3 * k:3 * k + 3]:
            assert g == dict(status=status, steps=[], n_steps=0), (name, g)
    # the entry point's own checks (layers.hip:297-298)
    one = lp.lines(valid, 2, pre)
    got = planner(one[:-1] + [one[-1] + " n_ops=0"] + one[:-1] + [one[-1] + " n_ops=-1"] + one[:-1] + [one[-1] + " null=1"] +
                  one[:-1] + [one[-1].replace("esz=2", "esz=3")])
    assert [(g["status"], g["n_steps"]) for g in got] == [(OK, 0), (INVALID, 0), (INVALID, 0), (INVALID, 0)]
    # ops of no rows give no step
    empty = [dict(o, rows=0) for o in valid[:1]] + valid[1:]
    assert [s["first"] for s in planner(lp.lines(empty, 2, pre))[0]["steps"]] == [1, 3, 4, 6]


# ---- doda_spconv_gather_ex's argument checks through describe_gather: the statuses of spconv_gather.hip:1128-1177 @ a917f1b, in order
GATHER_OK = dict(x=4096, w=8192, tbl=12288, y=16384, n_in=100, kc=32, esz=2, nc=32, ld=100, K=27, n_out=100, w_layout=0x100, epi=1, pre=1)
GATHER_OK.update({"e.residual": 64, "e.stats": 64, "e.stats_rows_h": 64, "e.bn_x": 64, "e.bn_mean": 64, "e.bn_invstd": 64, "e.bn_gamma": 64,
                  "e.bn_beta": 64, "e.x_ld": 48, "e.y_ld": 32, "e.residual_ld": 48, "e.bn_x_ld": 32,
                  "p.kind": 1, "p.rows": 100, "p.totals": 64, "p.mean": 64, "p.invstd": 64, "p.gamma": 64, "p.beta": 64, "p.side": 4096,
                  "p.side_ld": 32, "p.running_mean": 64, "p.running_var": 64})
BWD = {"p.kind": 3, "p.aux": 64, "p.add": 64, "p.aux_ld": 32, "p.add_ld": 32, "p.dgamma": 64, "p.dbeta": 64}
GATHER_DEFECTS = [
    (dict(esz=3), INVALID),                                                                     # :1133
    (dict(kc=0), INVALID), (dict(nc=0), INVALID), (dict(K=0), INVALID), (dict(n_out=-1), INVALID), (dict(ld=99), INVALID),
    (dict(w_layout=3), INVALID), (dict(w_layout=0x200), INVALID),                               # bad_args :1044
    (dict(n_out=0, ld=0, x=0), OK),                                                             # :1048 (before the null tests)
    (dict(x=0), INVALID), (dict(w=0), INVALID), (dict(tbl=0), INVALID), (dict(y=0), INVALID),   # :1049
    (dict(K=28), UNSUPPORTED), (dict(nc=4100), UNSUPPORTED), (dict(kc=4100), UNSUPPORTED),      # :1050
    ({"e.stats_rows_h": 0}, INVALID),                                                           # :1147
    ({"e.bn_mean": 0}, INVALID), ({"e.bn_invstd": 0}, INVALID), ({"e.bn_gamma": 0}, INVALID), ({"e.bn_beta": 0}, INVALID),   # :1151
    ({"e.x_ld": -1}, INVALID), ({"e.y_ld": -1}, INVALID), ({"e.residual_ld": -1}, INVALID), ({"e.bn_x_ld": -1}, INVALID),   # :1161
    ({"e.x_ld": 31}, INVALID), ({"e.y_ld": 31}, INVALID), ({"e.residual_ld": 31}, INVALID), ({"e.bn_x_ld": 31}, INVALID),   # :1164
    ({"p.kind": 0}, INVALID), ({"p.kind": 4}, INVALID), ({"p.rows": 99}, INVALID), ({"p.side_ld": 31}, INVALID),            # :1173
    (dict(BWD, **{"p.aux_ld": 31}), INVALID), (dict(BWD, **{"p.add_ld": 31}), INVALID),                                     # :1173-1174
    (dict(BWD, **{"p.dgamma": 0}), INVALID), (dict(BWD, **{"p.dbeta": 0}), INVALID), (dict(BWD, **{"p.totals": 0}), INVALID),   # :1174
    ({"p.mean": 0}, INVALID), ({"p.invstd": 0}, INVALID), ({"p.running_var": 0}, INVALID), ({"p.running_mean": 0}, INVALID),    # :1175
    ({"p.totals_b": 64, "p.c_a": 0}, INVALID), ({"p.totals_b": 64, "p.c_a": 32}, INVALID), ({"p.totals_b": 64, "p.c_a": 18}, INVALID),
    ({"p.totals_b": 64, "p.c_a": 16, "p.totals": 0}, INVALID),                                                               # :1176
    # accepted: the same fields where the checks do not look (no statistics: bn_x unread; no residual: its stride unread; ...)
    ({"e.stats": 0, "e.stats_rows_h": 0, "e.bn_mean": 0, "e.bn_x_ld": 31}, OK), ({"e.residual": 0, "e.residual_ld": 31}, OK),
    ({"p.totals": 0, "p.mean": 0, "p.running_var": 0}, OK), (BWD, OK), ({"p.totals_b": 64, "p.c_a": 16}, OK), (dict(epi=0), OK),
]


def test_gather_argument_defects_give_the_entry_points_statuses(planner):
    line = lambda d: "gather " + " ".join("%s=%d" % kv for kv in dict(GATHER_OK, **d).items())
    got = planner([line({})] + [line(d) for d, _ in GATHER_DEFECTS] +
                  [line({"e.residual_bcast": 1}), line({"e.x_ld": 32, "e.residual_ld": 32, "p.kind": 1})])
    # strides equal to the channel count are dense; the statistics and the prologue are seen
    assert got[0] == dict(status=OK, n_out=100, x_ld=48, y_ld=0, res_ld=48, bnx_ld=0, res_bcast=0, stats=1, pre_kind=1,
                          route="conv_fast<PBF16W, 1, 1, 3, false, true, true, 1>", steps=[], n_steps=0)
    for (d, status), g in zip(GATHER_DEFECTS, got[1:]):
        assert g["status"] == status, (d, g)
        assert (g["n_out"] == 100) == (status == OK and d.get("n_out", 100) != 0), (d, g)
    assert (got[-2]["res_bcast"], got[-2]["res_ld"]) == (1, 0)     # a broadcast residual has no stride
    assert (got[-1]["x_ld"], got[-1]["res_ld"]) == (0, 0)

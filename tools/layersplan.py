"""The probe set of the op list's host plan (csrc/layers_plan.hpp) and its record on the GPU.

A probe is an op list of doda_layers_run with the switches it runs under: the lists tests/test_gpu_layers.py builds by hand, at its
smallest shapes (420 x 96, 83 x 112), and one list on each side of every threshold of the plan (fold limits, the tuned sweeps'
row counts, the grid caps of lay_bn / lay_stats, the channel limits), in bf16 and fp32.  Tables are synthetic (a band of
neighbours): the plan never reads one, the kernels only need valid rows.

  lines(probe)        the list as the text tests/host/layers_plan_main.cpp reads (pointers as addresses; built on the CPU)
  expected(probe, steps)   the trace lines the plan's steps stand for (tests/test_layers_plan_host.py)
  --run OUT.json      on an MI355X: every probe through doda_layers_run in one fresh child process with DODA_TRACE_GATHER=1
                      DODA_TRACE_BN=1; per probe the status, n_launches and the trace lines; then UBlock(7) over 83 voxels, forward
                      and backward, as the compiled extension lists it (SUBTREES): its trace lines and launch count
  --record            the same into tests/data/layers_plan_parent.json (run at the commit the plan must equal)
"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORD = os.path.join(ROOT, "tests", "data", "layers_plan_parent.json")
GEMM, BNFWD, BNBWD, STATS = 1, 2, 3, 4
F_RELU, F_TRAINING, F_ACCUM, F_IDENTITY = 4, 8, 16, 2
BIG = 1 << 30
PTRS = ("x", "w", "tbl", "y", "y2", "res", "aux", "stats", "stats_b", "gamma", "beta", "mean", "invstd", "running_mean", "running_var",
        "nbt", "dgamma", "dbeta")


_KEEP = []     # tilebooks: an op holds their address only


class Alloc:
    """Operands of a probe: device tensors with real contents on the GPU, CPU tensors (addresses only) for the host plan."""

    def __init__(self, esz, device):
        self.esz, self.dev = esz, device
        self.dtype = torch.bfloat16 if esz == 2 else torch.float32
        self.gpu = device.type == "cuda"
        self.g = torch.Generator().manual_seed(5)

    def feat(self, rows, c):
        if not self.gpu:
            return torch.empty((rows, c), dtype=self.dtype)
        return torch.randn((rows, c), generator=self.g).to(self.dtype).to(self.dev)

    def vec(self, c, value=None):
        if not self.gpu:
            return torch.empty(c)
        return (torch.rand(c, generator=self.g) + 0.5).to(self.dev) if value is None else torch.full((c,), value, device=self.dev)

    def totals(self, c):
        return torch.zeros((8, 2, c // 4, 16), dtype=torch.float64, device=self.dev)

    def nbt(self):
        return torch.zeros(1, dtype=torch.int64, device=self.dev)

    def band(self, K, rows, rows_in):
        """tbl [K][rows]: output row t reads the input rows t * rows_in // rows + o - K // 2 that exist."""
        t = torch.arange(rows, dtype=torch.int64).view(1, rows) * rows_in // max(rows, 1)
        src = t + torch.arange(K, dtype=torch.int64).view(K, 1) - K // 2
        src[(src < 0) | (src >= rows_in)] = -1
        return src.to(torch.int32).contiguous().to(self.dev)

    def tilebook(self, tbl):
        """The address of the tilebook of a K = 27 table (doda_tilebook_build), as a GEMM op carries it."""
        if self.gpu:
            from doda_amd import ops
            tb = ops.tilebook_build(tbl)
            assert tb is not None
        else:
            tb = torch.empty(64)
        _KEEP.append(tb)
        return tb.data_ptr()

    def packed(self, K, cin, cout, layout):
        if not self.gpu:
            return torch.empty(16)
        from doda_amd import ops
        w = (torch.randn(K, cin, cout, generator=self.g) * (1.0 / (cin * 9)) ** 0.5).to(self.dev)
        plan = ops.PackPlan([(w, K, cin, cout, layout, self.esz)], self.dev)
        plan.run()
        return plan.outputs[0]


# ------------------------------------------------------------------------------------------------------------- list builders
def bnfwd(A, n, c, x=None, y=None, split=None, training=True, y_ld=None, running=True, **kw):
    x = A.feat(n, c) if x is None else x
    y = A.feat(n, c) if y is None else y
    ca = split or c
    o = dict(kind=BNFWD, flags=F_RELU | (F_TRAINING if training else 0), rows=n, c_in=c, x_ld=x.stride(0), y_ld=y_ld or y.stride(0), x=x, y=y,
             eps=1e-4, momentum=0.1, gamma=A.vec(c), beta=A.vec(c), c_split=ca)
    if training:
        o.update(stats=A.totals(ca), stats_b=A.totals(c - ca) if ca < c else None, mean=A.vec(c), invstd=A.vec(c))
    if running or not training:
        o.update(running_mean=A.vec(c, 0.0), running_var=A.vec(c, 1.0), nbt=A.nbt())
    o.update(kw)
    return o


def bnbwd(A, n, c, x=None, y=None, res=None, split=None, flags=F_RELU, aux=None, **kw):
    x = A.feat(n, c) if x is None else x
    aux = A.feat(n, c) if aux is None else aux
    ca = split or c
    y = A.feat(n, ca) if y is None else y
    o = dict(kind=BNBWD, flags=flags, rows=n, c_in=c, c_split=ca, x_ld=x.stride(0), y_ld=y.stride(0), aux_ld=aux.stride(0), x=x, aux=aux, y=y,
             stats=A.totals(c), mean=A.vec(c, 0.1), invstd=A.vec(c), gamma=A.vec(c), beta=A.vec(c), dgamma=A.vec(c, 0.0), dbeta=A.vec(c, 0.0))
    if res is not None:
        o.update(res=res, res_ld=res.stride(0))
    if ca < c:
        y2 = A.feat(n, c - ca)
        o.update(y2=y2, y2_ld=y2.stride(0))
    o.update(kw)
    return o


def gemm(A, n, cin, cout, x, K=27, rows_in=None, layout=0, y=None, res=None, stats=True, aux=None, flags=0, **kw):
    rows_in = n if rows_in is None else rows_in
    y = A.feat(n, cout) if y is None else y
    o = dict(kind=GEMM, flags=flags, rows=n, rows_in=rows_in, c_in=cin, c_out=cout, K=K, tbl_ld=n, x_ld=x.stride(0), y_ld=y.stride(0), x=x,
             w=A.packed(K, cin, cout, layout), tbl=A.band(K, n, rows_in), y=y, stats=A.totals(cout) if stats else None)
    if res is not None:
        o.update(res=res, res_ld=res.stride(0))
    if aux is not None:
        o.update(aux=aux, aux_ld=aux.stride(0), mean=A.vec(cout, 0.1), invstd=A.vec(cout), gamma=A.vec(cout), beta=A.vec(cout))
    o.update(kw)
    return o


def stats(A, x, c):
    return dict(kind=STATS, flags=0, rows=x.shape[0], c_in=c, x_ld=x.stride(0), x=x, stats=A.totals(c))


def forward_fold(A, n, cin, cout):
    """STATS ; [STATS] ; BNFWD ; GEMM (tests/test_gpu_layers.py test_forward_fold_vs_torch_oracle_and_unfolded)"""
    x = A.feat(n, cin)
    ca = cin // 2 if cin == 2 * cout else cin
    lst = [stats(A, x, ca)] + ([stats(A, x[:, ca:], cin - ca)] if ca < cin else [])
    b = bnfwd(A, n, cin, x=x, split=ca)
    b.update(stats=lst[0]["stats"], stats_b=lst[1]["stats"] if ca < cin else None)
    return lst + [b, gemm(A, n, cin, cout, b["y"], res=A.feat(n, cout))]


def backward_fold(A, n, c, with_add):
    """GEMM(data gradient) ; BNBWD ; GEMM (test_backward_fold_vs_autograd_and_unfolded)"""
    u = A.feat(n, c)
    g1 = gemm(A, n, c, c, A.feat(n, c), layout=2, aux=u, flags=F_RELU)
    b = bnbwd(A, n, c, x=g1["y"], aux=u, res=A.feat(n, 2 * c)[:, c:] if with_add else None, stats=g1["stats"])
    return [g1, b, gemm(A, n, c, c, b["y"], layout=2)]


def accum_strided(A, n, c):
    """BNBWD(accumulate, aux = the left half of a concatenation) ; GEMM (test_fold_accumulates_parameter_gradients_...)"""
    b = bnbwd(A, n, c, aux=A.feat(n, 2 * c)[:, :c], flags=F_RELU | F_ACCUM)
    return [b, gemm(A, n, c, c, b["y"], layout=2, stats=False)]


def batchnorm_ops(A, n, c):
    """The standalone BatchNorm ops of test_batchnorm_ops_vs_torch in one list."""
    C2 = 2 * c
    x = A.feat(n, C2)
    s = [stats(A, x, c), stats(A, x[:, c:], c)]
    return s + [bnfwd(A, n, C2, x=x, split=c, stats=s[0]["stats"], stats_b=s[1]["stats"]),
                bnfwd(A, n, C2, x=x, y=A.feat(n, C2 + 16)[:, 16:], split=c, stats=s[0]["stats"], stats_b=s[1]["stats"]),
                bnbwd(A, n, C2, res=A.feat(n, C2), split=c),
                bnfwd(A, n, C2, x=x, training=False)]


def down_up_1x1(A, n, c):
    """k2 s2 convolution both ways and the 1x1 convolution over column slices (test_gemm_down_up_and_1x1_with_strided_operands)"""
    m, c2 = (n + 7) // 8, c + 16
    cat, out = A.feat(n, 2 * c), A.feat(n, 2 * c)
    return [gemm(A, m, c, c2, cat[:, :c], K=8, rows_in=n),
            gemm(A, n, c2, c, A.feat(m, c2), K=8, rows_in=m, y=out[:, c:], stats=False),
            gemm(A, n, 2 * c, c, cat, K=1, res=out[:, c:], stats=False, flags=F_IDENTITY)]


def fold_pair(A, n, c, bwd=False, **kw):
    b = bnbwd(A, n, c, **kw) if bwd else bnfwd(A, n, c, **kw)
    return [b, gemm(A, n, c, c, b["y"], layout=2 if bwd else 0, stats=False)]


def tiled(A, n, c, fold=False):
    """A convolution whose table comes with its tilebook (the LDS-staged tile kernels), alone or behind a BatchNorm op that folds
    (the folded gather does not take the tilebook)."""
    b = bnfwd(A, n, c) if fold else None
    g = gemm(A, n, c, c, b["y"] if fold else A.feat(n, c), res=A.feat(n, c))
    g["tilebook"] = A.tilebook(g["tbl"])
    return ([b] if fold else []) + [g]


def other_stride(A):
    """BNFWD ; GEMM reading the BatchNorm's output address with another row stride (every second row of a taller matrix)"""
    y = A.feat(600, 32)[:300]
    g = gemm(A, 300, 32, 32, y, stats=False)
    g["x_ld"] = 64
    return [bnfwd(A, 300, 32, y=y), g]


def probes():
    """[(name, esz, (pre_fwd_rows, pre_bwd_rows) or None for the defaults, builder(A))]"""
    P = []
    for esz in (2, 4):
        t = "bf16" if esz == 2 else "fp32"
        add = lambda name, build, pre=None: P.append(("%s_%s" % (name, t), esz, pre, build))
        for n, c in ((420, 96), (83, 112)):
            for pre, tag in (((BIG, BIG), "fold"), ((0, 0), "nofold"), (None, "default")):
                add("forward_%d_%s" % (n, tag), lambda A, n=n, c=c: forward_fold(A, n, c, c), pre)
                add("forward_cat_%d_%s" % (n, tag), lambda A, n=n, c=c: forward_fold(A, n, 2 * c, c), pre)
                for wa in (0, 1):
                    add("backward_%d_add%d_%s" % (n, wa, tag), lambda A, n=n, c=c, wa=wa: backward_fold(A, n, c, wa), pre)
            add("accum_strided_%d" % n, lambda A, n=n, c=c: accum_strided(A, n, c), (BIG, BIG))
            add("batchnorm_ops_%d" % n, lambda A, n=n, c=c: batchnorm_ops(A, n, c))
            add("down_up_1x1_%d" % n, lambda A, n=n, c=c: down_up_1x1(A, n, c))
        # ---- thresholds, 32 channels: one list on each side
        for n in (16384, 16385):
            add("fwd_fold_rows_%d" % n, lambda A, n=n: fold_pair(A, n, 32))
        for n in (4096, 4097):
            add("bwd_fold_rows_%d" % n, lambda A, n=n: fold_pair(A, n, 32, bwd=True), (16384, 4096))
        add("bwd_fold_default", lambda A: fold_pair(A, 4096, 32, bwd=True))
        tuned = 32768 if esz == 2 else 4096
        for n in (tuned - 1, tuned):
            add("tuned_fwd_%d" % n, lambda A, n=n: [bnfwd(A, n, 32)], (0, 0))
            add("tuned_bwd_%d" % n, lambda A, n=n: [bnbwd(A, n, 32, res=A.feat(n, 32))], (0, 0))
        n = tuned
        add("tuned_off_x_strided", lambda A, n=n: [bnfwd(A, n, 32, x=A.feat(n, 48)[:, :32])], (0, 0))
        add("tuned_off_y_strided", lambda A, n=n: [bnfwd(A, n, 32, y=A.feat(n, 48)[:, 16:])], (0, 0))
        add("tuned_off_eval", lambda A, n=n: [bnfwd(A, n, 32, training=False)], (0, 0))
        add("tuned_off_split", lambda A, n=n: [bnbwd(A, n, 32, split=16)], (0, 0))
        add("tuned_off_accum", lambda A, n=n: [bnbwd(A, n, 32, flags=F_RELU | F_ACCUM)], (0, 0))
        add("tuned_off_aux_strided", lambda A, n=n: [bnbwd(A, n, 32, aux=A.feat(n, 48)[:, :32])], (0, 0))
        for c in (32, 256):     # the lay_bn grid at its cap of 2048 workgroups of 256 / (c / (16 / esz)) rows (a strided y keeps lay_bn)
            rpb = 256 // (c // (16 // esz))
            at = 2048 * rpb
            for n in (at - rpb, at, at + 1):
                add("lay_bn_cap_%d_%d" % (c, n), lambda A, n=n, c=c: [bnfwd(A, n, c, y=A.feat(n, c + 16)[:, 16:])], (0, 0))
        for n in (1023 * 256, 1024 * 256, 1024 * 256 + 1):   # lay_stats: 1024 workgroups x 32 row lanes x 8 rows at 32 channels
            add("lay_stats_cap_%d" % n, lambda A, n=n: [stats(A, A.feat(n, 32), 32)])
        for c in (16, 24, 32):
            add("fold_channels_%d" % c, lambda A, c=c: fold_pair(A, 300, c))
        for c in (256, 264):
            add("bn_channels_%d" % c, lambda A, c=c: [bnfwd(A, 64, 32), bnfwd(A, 64, c)], (0, 0))
        # ---- one list per clause of the fold rule that says no
        def unfold(A, **edit):
            lst = fold_pair(A, 300, 32)
            lst[1].update({k: (v(A, lst) if callable(v) else v) for k, v in edit.items()})
            return lst
        add("nofold_other_x", lambda A: unfold(A, x=lambda A, l: A.feat(300, 32)))
        add("nofold_rows_in", lambda A: unfold(A, rows_in=301, x=lambda A, l: A.feat(301, 32)))
        add("nofold_side_strided", lambda A: (lambda b: [b, gemm(A, 300, 32, 32, b["y"], stats=False)])(bnfwd(A, 300, 32, y=A.feat(300, 48)[:, 16:])))
        add("nofold_next_is_bn", lambda A: [bnfwd(A, 300, 32), bnfwd(A, 300, 32)])
        add("nofold_last_op", lambda A: [bnfwd(A, 300, 32)])
        add("nofold_c_in", lambda A: unfold(A, c_in=16))
        add("nofold_x_ld", other_stride)
        add("nofold_split_bwd", lambda A: fold_pair(A, 300, 32, bwd=True, split=16, y=A.feat(300, 32)), (BIG, BIG))
        # the folded kernels refuse 30 output channels; fp32: the BatchNorm's own launch and the generic kernel take the pair
        add("fold_fallback", lambda A: (lambda b: [b, gemm(A, 300, 32, 30, b["y"], stats=False)])(bnfwd(A, 300, 32)))
        # ---- tilebooks: 700 rows are three tiles, the last one ragged
        add("tile_16", lambda A: tiled(A, 700, 16))
        add("tile_32", lambda A: tiled(A, 700, 32))
        add("tile_fold_32", lambda A: tiled(A, 700, 32, fold=True))
    return P


SUBTREES = [(7, 83, 2), (7, 83, 4)]     # (level, voxels, esz): the smallest subtree of tests/test_gpu_layers.py, as the extension lists it


# --------------------------------------------------------------------------------------------------------- the list as text
def lines(lst, esz, pre):
    out = []
    for o in lst:
        words = ["op"]
        for k, v in o.items():
            if k in PTRS:
                words.append("%s=%d" % (k, 0 if v is None else v.data_ptr()))
            elif k not in ("eps", "momentum"):
                words.append("%s=%d" % (k, v))
        out.append(" ".join(words))
    out.append("run esz=%d" % esz + ("" if pre is None else " sw.pre_fwd_rows=%d sw.pre_bwd_rows=%d" % pre))
    return out


def host_lists():
    """[(name, esz, op list built on the CPU, its text)] of every probe"""
    return [(name, esz, lst, lines(lst, esz, pre)) for name, esz, pre, build in probes()
            for lst in [build(Alloc(esz, torch.device("cpu")))]]


def planner(exe, sanitized=False):
    """tests/host/layers_plan_main.cpp built with g++ (-Wall -Wextra -Werror) as `exe`; returns ask(lines) -> one dict per `run` /
    `gather` record: its status and fields, and the steps of a list."""
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, os.path.join(ROOT, "tests", "host", "layers_plan_main.cpp"),
                    "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = []
        for l in r.stdout.splitlines():
            kind, rest = l.split(" ", 1)
            if kind == "step":
                m = re.match(r"first=(\d+) n=(\d+) route=(.*) grid=(\d+) block=(\d+) parts=(\d+)$", rest)
                out[-1]["steps"].append(dict(first=int(m[1]), n=int(m[2]), route=m[3], grid=int(m[4]), block=int(m[5]), parts=int(m[6])))
            else:
                d = {k: (v if k == "route" else int(v)) for k, v in re.findall(r"(\w+)=(.*?)(?= \w+=|$)", rest)}
                n_steps = d.pop("steps", 0)
                out.append(dict(d, steps=[], n_steps=n_steps))
        assert len(out) == sum(l.startswith(("run", "gather")) for l in lines)
        assert all(len(o["steps"]) == o["n_steps"] for o in out)
        return out
    return ask


def expected(lst, esz, steps):
    """The trace lines (kernel, grid, block[, parts]) a list's planned steps stand for; the totals sweeps' kernel and grid are
    bn.hip's choice: tools/bnnumerics.py's copy of its geometry."""
    import bnnumerics as bn
    out = []
    for s in steps:
        o = lst[s["first"]]
        if s["route"] in ("bn_fwd_totals", "bn_bwd_totals"):
            p = dict(c=o["c_in"], esz=esz, m=o["rows"], add="dense", group="standalone")
            out.append(tuple(bn._apply(p, s["route"] == "bn_bwd_totals", True)))
        elif s["route"].startswith("conv_"):
            out.append((s["route"], s["grid"], s["block"], s["parts"]))
        else:
            out.append((s["route"], s["grid"], s["block"]))
    return out


def launched(trace):
    """A record's trace lines without those of a folded call that was tried and refused (`route=none`, then two launches): the
    plan asks that question on the host, where nothing is called and nothing traced."""
    return [l for l in trace if " route=none " not in l]


def parse_trace(trace):
    """The launches of a record's trace lines as the tuples of expected()."""
    out = []
    for l in launched(trace):
        m = re.match(r"doda_gather .* route=(.*) grid=(\d+) block=(\d+) parts=(\d+)$", l)
        if m:
            out.append((m[1], int(m[2]), int(m[3]), int(m[4])))
            continue
        m = re.match(r"bn route=(.*) grid=(\d+) block=(\d+)$", l)
        assert m, l
        out.append((m[1], int(m[2]), int(m[3])))
    return out


# ------------------------------------------------------------------------------------------------------------------ the GPU
def child():
    """Every probe through doda_layers_run; stderr carries `probe <name>` / `result <status> <launches>` around each list's trace."""
    import ctypes as C
    from doda_amd import ops
    from doda_amd._lib import lib
    d = torch.device("cuda:0")
    for name, esz, pre, build in probes():
        lst = build(Alloc(esz, d))
        old = ops.set_pre_rows(*pre) if pre else None
        torch.cuda.synchronize()
        sys.stderr.write("probe %s\n" % name)
        sys.stderr.flush()
        arr = ops._cx_array(lst, 0)
        launches = C.c_int32(-1)
        st = lib().doda_layers_run(C.cast(arr, C.c_void_p), len(lst), esz, C.byref(launches), ops._stream())
        torch.cuda.synchronize()
        sys.stderr.write("result %d %d\n" % (st, launches.value))
        sys.stderr.flush()
        if old:
            ops.set_pre_rows(*old)
    # UBlock(level) forward + backward as the compiled extension lists it (one doda_layers_run per direction)
    from doda_amd._ext import ext
    from tests.test_gpu_layers import _bf, _run_subtree, _subtree
    for level, n, esz in SUBTREES:
        net, ub, ind, shape, batch = _subtree(level, n, 23)
        g = torch.Generator().manual_seed(level * 100 + n)
        c = 16 * level
        dt = torch.bfloat16 if esz == 2 else torch.float32
        x0, gout = (_bf(torch.randn(ind.shape[0], c, generator=g)).to(d).to(dt) for _ in range(2))
        torch.cuda.synchronize()
        sys.stderr.write("subtree %d_%d_%d\n" % (level, n, esz))
        sys.stderr.flush()
        _run_subtree(ub, ind, shape, batch, level, x0, gout, "layers")
        sys.stderr.write("result 0 %d\n" % sum(ext.coarse_launches()))
        sys.stderr.flush()


def run_on_gpu():
    """{"probes": [...], "subtrees": [...]}: name, status, launches and trace lines of each"""
    env = dict(os.environ, DODA_TRACE_GATHER="1", DODA_TRACE_BN="1")
    for k in ("DODA_PRE_FWD_ROWS", "DODA_PRE_BWD_ROWS", "DODA_LAY_BN_GRID", "DODA_LAY_TUNED_ROWS", "DODA_BN_TOT_GRID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("the probe run failed with exit status %d" % r.returncode)
    rec, sub, cur, into = [], [], None, None
    for l in r.stderr.splitlines():
        if l.startswith("probe ") or l.startswith("subtree "):
            cur, into = dict(name=l.split(" ", 1)[1], trace=[]), rec if l.startswith("probe ") else sub
        elif l.startswith("result ") and cur is not None:
            cur["status"], cur["launches"] = (int(v) for v in l.split()[1:])
            into.append(cur)
            cur = None
        elif cur is not None and (l.startswith("doda_gather ") or l.startswith("bn route=")):
            cur["trace"].append(l)
    assert [r["name"] for r in rec] == [p[0] for p in probes()] and len(sub) == len(SUBTREES)
    return dict(probes=rec, subtrees=sub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--run", metavar="OUT.json")
    ap.add_argument("--record", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    if a.run or a.record:
        path = RECORD if a.record else a.run
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(run_on_gpu(), f, indent=0)
            f.write("\n")
        return
    for name, esz, _, text in host_lists():
        print("# " + name)
        print("\n".join(text))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()

#!/usr/bin/env python
"""Times the operators of include/doda_pointops.h against the same quantities composed from torch operators on the same GPU.

  fps_batch        4 segments x 20 000 points -> 5 000 samples each (one workgroup per segment; the tail of a segment streams)
  fps_small        one segment of 2 000 points -> 500 samples (register-resident)
  transpose        the index by destination of idx [rows, nsample] (built once per idx; every backward below reuses it)
  <op>_fwd / _bwd  grouping, interpolation, subtraction, aggregation at --rows rows, --nsample neighbours, c in --channels,
                   w_c = c / 8; the backwards are timed with the index already built

The baseline (`torch_*`) does not depend on the code under test: index_select / index_add_ / elementwise torch for the pairs (its
index_add_ is a float atomic scatter, so its backward is not reproducible bit for bit), and a torch loop without host read-backs
for the sampling.  Contenders alternate round by round in one process: --warmup rounds unrecorded, then --reps recorded (the torch
sampling loop: --fps-reps); times are per call between HIP events.  `bytes` is every input and output array counted once (gathered
rows counted at the size of what is gathered), `GB/s` that over the median.  No ratio is a target; a contender that loses to the
torch composition is reported as it is.

    python tools/pointopsbench.py --out profiles/pointops.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    q = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
    return {"median_ms": statistics.median(ms), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def torch_fps(xyz, sizes, wants):
    """The same rule from torch operators, no host read-back inside the loop (argmax returns the first maximum)."""
    out, lo = [], 0
    for size, want in zip(sizes, wants):
        pts = xyz[lo:lo + size]
        run = torch.full((size,), 1e10, device=xyz.device)
        cur = torch.zeros(1, dtype=torch.long, device=xyz.device)
        picked = [cur + lo]
        for _ in range(want - 1):
            diff = pts - pts.index_select(0, cur)
            run = torch.minimum(run, (diff * diff).sum(1))
            cur = torch.argmax(run).reshape(1)
            picked.append(cur + lo)
        out.append(torch.cat(picked))
        lo += size
    return torch.cat(out).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--nsample", type=int, default=16)
    ap.add_argument("--channels", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fps-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from doda_amd import ops, pointops2
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    n, ns = a.rows, a.nsample
    contenders, meta, slow = {}, {}, set()

    def add(name, fn, nbytes=None, **extra):
        contenders[name] = fn
        meta[name] = dict(extra, **({"bytes": int(nbytes)} if nbytes is not None else {}))

    # ---- sampling
    for tag, sizes, wants in (("fps_batch", [20000] * 4, [5000] * 4), ("fps_small", [2000], [500])):
        xyz = torch.rand(sum(sizes), 3, generator=g).to(d)
        off = torch.tensor([0] + sizes, dtype=torch.int32).cumsum(0).to(torch.int32).to(d)
        noff = torch.tensor([0] + wants, dtype=torch.int32).cumsum(0).to(torch.int32).to(d)
        agree = bool(torch.equal(pointops2.furthestsampling(xyz, off, noff), torch_fps(xyz, sizes, wants)))
        add(tag, lambda xyz=xyz, off=off, noff=noff: pointops2.furthestsampling(xyz, off, noff), samples_per_segment=wants[0],
            segments=len(sizes), points_per_segment=sizes[0], agrees_with_torch_loop=agree)
        add("torch_" + tag, lambda xyz=xyz, sizes=sizes, wants=wants: torch_fps(xyz, sizes, wants), samples_per_segment=wants[0],
            segments=len(sizes), points_per_segment=sizes[0])
        slow.add("torch_" + tag)

    # ---- the pairs: a kNN-like idx (each row points near itself), square as in the reference's subtraction / aggregation
    idx = ((torch.arange(n).unsqueeze(1) + torch.randint(-64, 65, (n, ns), generator=g)) % n).to(torch.int32).to(d)
    idxl = idx.view(-1).long()
    start, pos = ops.po_transpose(idx, n)
    add("transpose", lambda: ops.po_transpose(idx, n), 4 * (2 * n * ns + n + 1))
    f4 = 4
    for c in a.channels:
        w_c = max(c // 8, 1)
        x, y = torch.randn(n, c, generator=g).to(d), torch.randn(n, c, generator=g).to(d)
        position, w = torch.randn(n, ns, c, generator=g).to(d), torch.randn(n, ns, w_c, generator=g).to(d)
        w1 = torch.rand(n, ns, generator=g).to(d)
        g_rows, g_full = torch.randn(n, c, generator=g).to(d), torch.randn(n, ns, c, generator=g).to(d)
        full, rows, lists = torch.empty(n, ns, c, device=d), torch.empty(n, c, device=d), 4 * (n * ns + n + 1)
        rows2, full2, d_w = torch.empty(n, c, device=d), torch.empty(n, ns, c, device=d), torch.empty(n, ns, w_c, device=d)
        cols = torch.arange(c, device=d) % w_c
        t = "_c%d" % c
        big, small, ib = f4 * n * ns * c, f4 * n * c, 4 * n * ns

        add("grouping_fwd" + t, lambda x=x, full=full: ops.po_grouping_fwd(x, idx, full), 2 * big + ib)
        add("torch_grouping_fwd" + t, lambda x=x: x.index_select(0, idxl).view(n, ns, -1), 2 * big + ib)
        add("grouping_bwd" + t, lambda g_full=g_full, rows=rows: ops.po_grouping_bwd(g_full.view(n * ns, -1), start, pos, rows),
            big + small + lists)
        add("torch_grouping_bwd" + t, lambda g_full=g_full, c=c: torch.zeros(n, c, device=d).index_add_(0, idxl, g_full.view(n * ns, c)),
            big + small + ib)

        add("interpolation_fwd" + t, lambda x=x, w1=w1, rows=rows: ops.po_interpolation_fwd(x, idx, w1, rows), big + small + 2 * ib)

        def torch_interp(x=x, w1=w1, c=c):
            out = torch.zeros(n, c, device=d)
            for i in range(ns):
                out += x.index_select(0, idxl[i::ns]) * w1[:, i:i + 1]
            return out
        add("torch_interpolation_fwd" + t, torch_interp, big + small + 2 * ib)
        add("interpolation_bwd" + t, lambda g_rows=g_rows, w1=w1, rows=rows: ops.po_interpolation_bwd(g_rows, w1, start, pos, rows),
            big + small + lists + ib)
        add("torch_interpolation_bwd" + t, lambda g_rows=g_rows, w1=w1, c=c: torch.zeros(n, c, device=d).index_add_(
            0, idxl, (g_rows.unsqueeze(1) * w1.unsqueeze(2)).view(n * ns, c)), big + small + 2 * ib)

        add("subtraction_fwd" + t, lambda x=x, y=y, full=full: ops.po_subtraction_fwd(x, y, idx, full), 2 * big + small + ib)
        add("torch_subtraction_fwd" + t, lambda x=x, y=y: x.unsqueeze(1) - y.index_select(0, idxl).view(n, ns, -1), 2 * big + small + ib)
        add("subtraction_bwd" + t, lambda g_full=g_full, rows=rows, rows2=rows2: ops.po_subtraction_bwd(g_full, start, pos, rows, rows2),
            2 * big + 2 * small + lists)
        add("torch_subtraction_bwd" + t, lambda g_full=g_full, c=c: (g_full.sum(1), torch.zeros(n, c, device=d).index_add_(
            0, idxl, -g_full.view(n * ns, c))), 2 * big + 2 * small + ib)

        wb = f4 * n * ns * w_c
        add("aggregation_fwd" + t, lambda x=x, position=position, w=w, rows=rows: ops.po_aggregation_fwd(x, position, w, idx, rows),
            2 * big + wb + small + ib)
        add("torch_aggregation_fwd" + t, lambda x=x, position=position, w=w, cols=cols: (
            (x.index_select(0, idxl).view(n, ns, -1) + position) * w[..., cols]).sum(1), 2 * big + wb + small + ib)
        add("aggregation_bwd" + t, lambda x=x, position=position, w=w, g_rows=g_rows, rows=rows, full2=full2, d_w=d_w:
            ops.po_aggregation_bwd(x, position, w, idx, start, pos, g_rows, rows, full2, d_w), 4 * big + 3 * wb + 2 * small + ib + lists)

        def torch_agg_bwd(x=x, position=position, w=w, g_rows=g_rows, cols=cols, c=c, w_c=w_c):
            d_position = g_rows.unsqueeze(1) * w[..., cols]
            inner = g_rows.unsqueeze(1) * (x.index_select(0, idxl).view(n, ns, c) + position)
            d_weight = inner.view(n, ns, c // w_c, w_c).sum(2)
            return torch.zeros(n, c, device=d).index_add_(0, idxl, d_position.view(n * ns, c)), d_position, d_weight
        add("torch_aggregation_bwd" + t, torch_agg_bwd, 4 * big + 3 * wb + 2 * small + ib)

    times = {k: [] for k in contenders}
    for r in range(a.warmup + a.reps):
        for name, fn in contenders.items():
            if name in slow and r >= a.fps_reps:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup or name in slow:
                times[name].append(e0.elapsed_time(e1))
    result = {}
    for name, ms in times.items():
        s = dict(stats(ms), **meta[name])
        if "bytes" in s:
            s["GB_per_s"] = s["bytes"] / s["median_ms"] / 1e6
        if "samples_per_segment" in s:
            s["us_per_sample"] = 1e3 * s["median_ms"] / s["samples_per_segment"]
        result[name] = s
        print("%-28s median %9.3f ms %s" % (name, s["median_ms"], ("%8.1f GB/s" % s["GB_per_s"]) if "bytes" in s else
                                            ("%8.3f us/sample" % s["us_per_sample"])), flush=True)
    record = {"workload": {"rows": n, "nsample": ns, "channels": a.channels, "w_c": "c / 8"},
              "method": "time per call between HIP events, contenders alternating per round, %d warm-up + %d recorded rounds "
                        "(torch sampling loop: %d rounds, none discarded)" % (a.warmup, a.reps, a.fps_reps),
              "times": result}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"median_ms": {k: round(v["median_ms"], 4) for k, v in result.items()}}))


if __name__ == "__main__":
    main()

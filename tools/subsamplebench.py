#!/usr/bin/env python
"""The training subsample of a batch (DATA_PROCESSOR.downsampling_scale): ops.subsample (doda_subsample_draw, one native call)
against the torch route a loader would write (per scene: randperm, slice, sort, index_select of the points and of the labels).

4 scenes of 1 M points, ds = 4 by default.  Both routes run on a side stream, alternating, each round timed between HIP events;
3 warm-up and 30 recorded rounds; medians and quartiles into profiles/r12_subsample.json (--out).  Under
`rocprofv3 --kernel-trace --stats -- python tools/subsamplebench.py --rounds 5 --out <other file>` the trace lists the time of
each launch (sub_hist x 4, sub_count, sub_emit)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_route(xyz, labels, offsets, ks, gen):
    xs, ls = [], []
    for b, k in enumerate(ks):
        n = offsets[b + 1] - offsets[b]
        idx = torch.sort(torch.randperm(n, device=xyz.device, generator=gen)[:k])[0] + offsets[b]
        xs.append(xyz.index_select(0, idx))
        ls.append(labels.index_select(0, idx))
    return torch.cat(xs), torch.cat(ls)


def quartiles(v):
    q = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"q1_ms": float(q[0]), "median_ms": float(q[1]), "q3_ms": float(q[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--ds", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_subsample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subsamplebench needs an MI355X")
    from doda_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = a.scenes * a.points
    xyz = torch.rand((n, 3), device=dev, generator=g)
    labels = torch.randint(0, 20, (n,), device=dev, generator=g, dtype=torch.int32)
    offsets = [b * a.points for b in range(a.scenes + 1)]
    ks = [int(a.points / a.ds)] * a.scenes
    side = torch.cuda.Stream(dev)
    times = {"native": [], "torch": [], "torch_same_draw": []}
    routes = {"native": lambda r: ops.subsample(xyz, labels, offsets, ks, [r * 64 + b for b in range(a.scenes)]),
              "torch": lambda r: torch_route(xyz, labels, offsets, ks, g),
              "torch_same_draw": lambda r: ops.subsample_torch(xyz, labels, offsets, ks, [r * 64 + b for b in range(a.scenes)])}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for r in range(a.warmup + a.rounds):
            for name, run in routes.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(side)
                run(r)
                t1.record(side)
                t1.synchronize()
                if r >= a.warmup:
                    times[name].append(t0.elapsed_time(t1))
    out = {"scenes": a.scenes, "points_per_scene": a.points, "ds": a.ds, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), **{k: quartiles(v) for k, v in times.items()}}
    out["native_is_default"] = out["native"]["median_ms"] < out["torch"]["q1_ms"]
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times the clustering, segment-pool and proposal-IoU operators of include/doda_pgops.h on synthetic scenes (4 scenes of about
150 k points by default):

  cluster_device   ballquery_batch_p + bfs_cluster on device tensors (union-find components + grouping)
  cluster_host     ballquery_batch_p + the three copies to the CPU + the sequential BFS on the host + the two results copied back:
                   the reference's route, whose BFS is host code
  components       doda_pg_components alone (four launches)
  sec_mean / sec_min / sec_max / roipool_fp / sec_mean_bp / roipool_bp   over the clusters found, C = --channels
  get_iou          --proposals proposals by --instances instances

Contenders alternate round by round on one GPU in one process: --warmup rounds unrecorded, then --reps recorded; the record holds
per contender the median, the quartiles and min / max of the time per call between HIP events (host work between the two events —
the BFS, the read-back of the two sizes — is inside the interval).  No ratio is a target and no default depends on the outcome:
device tensors take the device route, CPU tensors the host route.

    python tools/pgopsbench.py --out profiles/pgops.json
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
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "q1_ms": q[0], "q3_ms": q[2], "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--voxels", type=int, default=115000)      # x 1.3 points per voxel: about 150 k points per scene
    ap.add_argument("--radius", type=float, default=0.04)
    ap.add_argument("--mean-active", type=int, default=50)
    ap.add_argument("--threshold", type=int, default=50)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--proposals", type=int, default=300)
    ap.add_argument("--instances", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from doda_amd import ops, pointgroup_ops as pg
    from doda_amd.scene import make_batch
    d = torch.device("cuda:0")
    b = make_batch(a.scenes, a.voxels, 1000)
    xyz, offsets = b["locs_float"].to(d).contiguous(), b["offsets"].to(d)
    n = xyz.shape[0]
    bidx = torch.repeat_interleave(torch.arange(a.scenes, device=d), (offsets[1:] - offsets[:-1]).long()).to(torch.int32)
    label = b["labels"].to(torch.int32).to(d)

    def query():
        idx, start_len = pg.ballquery_batch_p(xyz, bidx, offsets, a.radius, a.mean_active)
        return idx.contiguous(), start_len

    def cluster_device():
        idx, start_len = query()
        return pg.bfs_cluster(label, idx, start_len, a.threshold)

    def cluster_host():
        idx, start_len = query()
        ci, co = pg.bfs_cluster(label.cpu(), idx.cpu(), start_len.cpu(), a.threshold)
        return ci.to(d), co.to(d)

    idx, start_len = query()
    ci, co = cluster_device()
    hi, ho = cluster_host()
    same = bool(torch.equal(co, ho) and torch.equal(torch.sort(ci[:, 1])[0], torch.sort(hi[:, 1])[0]))
    g = torch.Generator().manual_seed(1)
    n_seg, c = co.numel() - 1, a.channels
    feats = torch.randn(ci.shape[0], c, generator=g).to(d)
    d_out = torch.randn(n_seg, c, generator=g).to(d)
    out, arg = torch.empty(n_seg, c, device=d), torch.empty(n_seg, c, dtype=torch.int32, device=d)
    d_feats = torch.zeros_like(feats)
    ops.roipool_fp(feats, co, out, arg, n_seg, c)
    per = max(n // a.proposals // 4, 1)
    p_idx = torch.randint(0, n, (a.proposals * per,), generator=g).to(torch.int32).to(d)
    p_off = (torch.arange(a.proposals + 1, dtype=torch.int32) * per).to(d)
    inst = torch.randint(0, a.instances, (n,), generator=g).to(d)
    inst[torch.rand(n, generator=g).to(d) < 0.2] = -100
    pointnum = torch.bincount(inst[inst >= 0], minlength=a.instances).to(torch.int32)
    iou = torch.empty(a.proposals, a.instances, device=d)

    contenders = {
        "ballquery": query,
        "cluster_device": cluster_device,
        "cluster_host": cluster_host,
        "components": lambda: ops.pg_components(label, idx, start_len),
        "sec_mean": lambda: ops.sec_mean(feats, co, out, n_seg, c),
        "sec_min": lambda: ops.sec_min(feats, co, out, n_seg, c),
        "sec_max": lambda: ops.sec_max(feats, co, out, n_seg, c),
        "roipool_fp": lambda: ops.roipool_fp(feats, co, out, arg, n_seg, c),
        "sec_mean_bp": lambda: ops.sec_mean_bp(d_feats, co, d_out, n_seg, c),
        "roipool_bp": lambda: ops.roipool_bp(d_feats, co, arg, d_out, n_seg, c),
        "get_iou": lambda: ops.get_iou(p_idx, p_off, inst, pointnum, iou, a.instances, a.proposals),
    }
    times = {k: [] for k in contenders}
    for r in range(a.warmup + a.reps):
        for name, fn in contenders.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    sizes = (co[1:] - co[:-1]).cpu()
    record = {"workload": {"scenes": a.scenes, "points": n, "neighbour_entries": int(idx.numel()), "radius": a.radius,
                           "threshold": a.threshold, "clusters": n_seg, "clustered_points": int(ci.shape[0]),
                           "largest_cluster": int(sizes.max()) if n_seg else 0, "channels": c, "proposals": a.proposals,
                           "instances": a.instances, "proposal_points": int(p_idx.numel())},
              "method": "time per call between HIP events, contenders alternating per round, %d warm-up + %d recorded rounds"
                        % (a.warmup, a.reps),
              "device_and_host_routes_agree_as_sets": same,
              "times": {k: stats(v) for k, v in times.items()}}
    for name, s in record["times"].items():
        print("%-15s median %8.3f ms  [q1 %8.3f, q3 %8.3f]" % (name, s["median_ms"], s["q1_ms"], s["q3_ms"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"workload": record["workload"], "agree": same,
                      "median_ms": {k: round(v["median_ms"], 4) for k, v in record["times"].items()}}))


if __name__ == "__main__":
    main()

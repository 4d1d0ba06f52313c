#!/usr/bin/env python
"""Times the voxel-level Lovasz-softmax head (doda_amd.lovasz._VoxelHeadLovasz: doda_lovasz_fwd / _bwd + the head's weight-gradient
kernel) against the point-level torch restatement (doda_amd.lovasz.lovasz_softmax on _PointLinear's [points, classes] score
matrix) and, as context, against the cross-entropy head (_VoxelHeadCE), forward + backward, on the bench batch (4 scenes x 150 k
voxels) with bf16 features.

All contenders run on the same GPU in the same process, alternating round by round: --warmup rounds unrecorded, then --reps
recorded; the record holds per contender the median, the quartiles and min / max of its device time per call (HIP events around
forward + backward), the ratios of the medians and whether the fused path wins by more than the spread of the repetitions
(its upper quartile below the restatement's lower quartile).  The restatement is timed in its default form (evaluation in fp64) and
with compute_dtype=float32.

    python tools/lovaszbench.py --classes 11 20 --out profiles/r09_lovasz.json
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
    ap.add_argument("--voxels", type=int, default=150000)
    ap.add_argument("--voxel-scale", type=int, default=50)
    ap.add_argument("--classes", type=int, nargs="+", default=[11, 20])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from doda_amd import model
    from doda_amd.lovasz import _VoxelHeadLovasz, lovasz_softmax
    from doda_amd.scene import make_batch
    d = torch.device("cuda:0")
    b = make_batch(a.scenes, a.voxels, 1000, a.voxel_scale)      # (bench.py's batch)
    v2p, p2v = b["v2p_map"].to(d), b["p2v_map"].to(d)
    v2p_t = v2p[:, 1:].t().contiguous()
    m, n = v2p.shape[0], p2v.shape[0]
    record = {"workload": {"scenes": a.scenes, "voxels": m, "points": n, "feature_dtype": "bf16", "v2p_ld": v2p.shape[1]},
              "method": "forward + backward between HIP events, contenders alternating per round, %d warm-up + %d recorded rounds"
                        % (a.warmup, a.reps), "classes": {}}
    g = torch.Generator().manual_seed(1)
    for n_cls in a.classes:
        labels = (b["labels"] % n_cls).to(d)
        labels[torch.randperm(n, generator=g)[: n // 20].to(d)] = 255
        feats = (torch.randn(m, 16, generator=g) * 1.5).to(d).bfloat16().requires_grad_(True)
        W = (torch.randn(n_cls, 16, generator=g) * 0.4).to(d).requires_grad_(True)
        bias = (torch.randn(n_cls, generator=g) * 0.2).to(d).requires_grad_(True)

        def fused():
            return _VoxelHeadLovasz.apply(feats, W, bias, v2p, labels, 255)[0]

        def matrix(dtype):
            def run():
                return lovasz_softmax(model._PointLinear.apply(feats, W, bias, p2v, v2p_t), labels, 255, compute_dtype=dtype)
            return run

        def ce():
            return model._VoxelHeadCE.apply(feats, W, bias, v2p, labels, 255)[0]

        contenders = {"fused_voxel_head": fused, "ce_voxel_head": ce}
        if n_cls % 4 == 0:      # (_PointLinear's gather-GEMM takes class counts that are multiples of four: the model's own condition)
            contenders["torch_restatement_fp64"] = matrix(torch.float64)
            contenders["torch_restatement_fp32"] = matrix(torch.float32)
        else:
            def plain(dtype):
                def run():
                    scores = torch.nn.functional.linear(feats[p2v.long()].float(), W, bias)
                    return lovasz_softmax(scores, labels, 255, compute_dtype=dtype)
                return run
            contenders["torch_restatement_fp64"] = plain(torch.float64)
            contenders["torch_restatement_fp32"] = plain(torch.float32)
        times = {k: [] for k in contenders}
        losses = {}
        for r in range(a.warmup + a.reps):
            for name, fn in contenders.items():
                for t in (feats, W, bias):
                    t.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = fn()
                loss.backward()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
                losses[name] = float(loss.detach())
        res = {k: stats(v) for k, v in times.items()}
        best = min(("torch_restatement_fp64", "torch_restatement_fp32"), key=lambda k: res[k]["median_ms"])
        res["loss"] = losses
        res["restatement_over_fused"] = {k: res[k]["median_ms"] / res["fused_voxel_head"]["median_ms"]
                                         for k in ("torch_restatement_fp64", "torch_restatement_fp32")}
        res["fused_over_ce"] = res["fused_voxel_head"]["median_ms"] / res["ce_voxel_head"]["median_ms"]
        res["fused_faster_beyond_spread"] = res["fused_voxel_head"]["q3_ms"] < res[best]["q1_ms"]
        record["classes"][str(n_cls)] = res
        print("classes %2d: fused %.3f ms [%.3f, %.3f]  restatement fp64 %.3f ms fp32 %.3f ms  CE head %.3f ms  loss fused %.6f / %.6f" % (
            n_cls, res["fused_voxel_head"]["median_ms"], res["fused_voxel_head"]["q1_ms"], res["fused_voxel_head"]["q3_ms"],
            res["torch_restatement_fp64"]["median_ms"], res["torch_restatement_fp32"]["median_ms"], res["ce_voxel_head"]["median_ms"],
            losses["fused_voxel_head"], losses["torch_restatement_fp64"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({k: {c: v[k] for c, v in record["classes"].items()} for k in ("restatement_over_fused", "fused_over_ce",
                                                                                  "fused_faster_beyond_spread")}))


if __name__ == "__main__":
    main()

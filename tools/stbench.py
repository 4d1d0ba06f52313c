"""Pseudo-label generation pass of the self-training stage, timed per target scene (DESIGN.md "Self-training: pseudo labels").

    python tools/stbench.py [--scenes 8] [--voxels 150000] [--dtype f32|bf16] [--json out.json]

Per scene, device time between events: the network trunk (input layer, U-Net, output layer), the new kernels
(doda_st_voxel_confidence + doda_st_point_store), and per pass over all scenes the host radix scan (three doda_st_radix_hist
launches + their read-backs) and doda_st_label.  Against it the same pass done the torch way: the model's existing forward (the
[points, classes] score matrix), softmax + max, and a per-class torch.sort (descending) for the ratio thresholds.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/stbench.py` for the per-kernel split."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--voxels", type=int, default=150000)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from doda_amd import ops
    from doda_amd import pseudo_labels as pl
    from doda_amd.collate import collate_device
    from doda_amd.loader import SyntheticScenes, prepare_cache
    from doda_amd.model import SparseConvNet, default_cfg, sparse_input
    d = torch.device("cuda:0")
    fdt = torch.float32 if a.dtype == "f32" else torch.bfloat16
    cfg = default_cfg()
    torch.manual_seed(0)
    net = SparseConvNet(cfg).to(d).eval()
    n_cls = net.linear.out_features
    cache = os.path.join(tempfile.gettempdir(), "doda_stbench_%d" % os.getuid())
    _, paths = prepare_cache(a.scenes, a.voxels, 50, 501000, cache)
    ds = SyntheticScenes(paths, len(paths), 50, 0, augment=False)
    batches = [collate_device([ds[k]], d) for k in range(len(paths))]
    n_pts = sum(int(b["p2v_map"].numel()) for b in batches)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = {"scenes": a.scenes, "voxels": a.voxels, "points": n_pts, "dtype": a.dtype}
    with torch.no_grad():
        for rep in range(a.reps):
            # ---- this project's pass
            store_cls = torch.empty(n_pts, dtype=torch.uint8, device=d)
            store_conf = torch.empty(n_pts, dtype=torch.float32, device=d)
            hist0 = torch.zeros((n_cls, 256), dtype=torch.int64, device=d)
            t_trunk = t_new = 0.0
            off = 0
            for b in batches:
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                inp, p2v, _ = sparse_input(cfg, net, b, d, fdt)
                feats = net._trunk(inp).features
                e1.record()
                pred, conf = ops.voxel_confidence(feats.contiguous(), net.linear.weight, net.linear.bias)
                ops.st_point_store(pred, conf, p2v, store_cls, store_conf, off, n_cls, hist0)
                e2.record()
                torch.cuda.synchronize()
                t_trunk += e0.elapsed_time(e1)
                t_new += e1.elapsed_time(e2)
                off += p2v.numel()
            t0 = time.perf_counter()
            h0 = hist0.cpu().numpy()
            thres = pl.select_thresholds(h0.sum(1), [0.3], lambda lv, pre: h0 if lv == 0 else ops.st_radix_hist(
                store_cls, store_conf, n_cls, lv, torch.from_numpy(pre).to(d)).cpu().numpy())
            t1 = time.perf_counter()
            e0, e1 = ev(), ev()
            e0.record()
            labels, kept = ops.st_label(store_cls, store_conf, torch.from_numpy(thres).to(d), 255)
            e1.record()
            torch.cuda.synchronize()
            ours = {"trunk_ms": t_trunk / a.scenes, "new_kernels_ms": t_new / a.scenes, "host_scan_ms": 1e3 * (t1 - t0) / a.scenes,
                    "label_ms": e0.elapsed_time(e1) / a.scenes}
            # ---- the torch way: point scores, softmax, per-class sort
            t_fwd = t_sm = 0.0
            confs, preds = [], []
            for b in batches:
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                inp, p2v, v2p = sparse_input(cfg, net, b, d, fdt)
                scores = net(inp, p2v, v2p_map=v2p, v2p_map_t=b.get("v2p_map_t"))
                e1.record()
                c, p = torch.softmax(scores.float(), 1).max(1)
                e2.record()
                torch.cuda.synchronize()
                t_fwd += e0.elapsed_time(e1)
                t_sm += e1.elapsed_time(e2)
                confs.append(c)
                preds.append(p)
            t0 = time.perf_counter()
            c, p = torch.cat(confs), torch.cat(preds)
            tt = []
            for k in range(n_cls):
                v = torch.sort(c[p == k], descending=True).values
                tt.append(float(v[max(1, int(0.3 * v.numel())) - 1]) if v.numel() else 0.0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            torch_way = {"forward_scores_ms": t_fwd / a.scenes, "softmax_max_ms": t_sm / a.scenes, "sort_ms": 1e3 * (t1 - t0) / a.scenes}
            res["threshold_max_abs_diff"] = float(np.abs(np.array(tt, dtype=np.float64) - thres.astype(np.float64)).max())
            res["ours"], res["torch"] = ours, torch_way
    ours, tw = res["ours"], res["torch"]
    res["ours_total_ms"] = sum(ours.values())
    res["torch_total_ms"] = sum(tw.values())
    res["new_kernels_share"] = (ours["new_kernels_ms"] + ours["label_ms"]) / res["ours_total_ms"]
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()

"""Times of the DATA_AUG pipeline (doda_amd.aug) on one GPU.

    python tools/augbench.py [--reps 30] [--out FILE.json]

Two workloads: B4 x 150 k points at voxel_scale 50 and B4 x 500 k points at voxel_scale 100 (room-shaped surface scenes,
the ScanNet DATA_AUG values).  Per workload: device-event time of every native call of one augment_batch (affine, blur and displace
per elastic pass, crop, emit; the Python wrapper's allocations and table uploads around a call are inside its figure, so these are
upper bounds of the kernels' own times), bytes moved and the achieved rate against 8 TB/s, and the loader thread's wall time per
batch for augment_batch against the rigid path of DeviceScenes (_rigid + _finish) on the same scenes, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from doda_amd import aug   # noqa: E402
from doda_amd import _lib   # noqa: E402

HBM = 8.0e12


def scene(seed, n, room):
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 10, n)
    u = rng.random((n, 3)) * np.array(room)
    u[kind < 3, 2] = 0.0
    u[kind == 3, 2] = room[2]
    u[kind == 4, 0] = 0.0
    u[kind == 5, 0] = room[0]
    u[kind == 6, 1] = 0.0
    u[kind == 7, 1] = room[1]
    u += rng.normal(0.0, 0.01, (n, 3))
    u -= u.mean(0)
    return u.astype(np.float32), rng.integers(0, 20, n).astype(np.int32)


class Timed:
    """Wraps the native library: device events around every doda_aug_* call."""

    def __init__(self, lib):
        self.lib, self.spans = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("doda_aug_") or name in ("doda_aug_blocks", "doda_aug_abi_version"):
            return fn

        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = fn(*a)
            e1.record()
            self.spans.append((name, e0, e1))
            return st
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sec = {"aug_list": ["scene_aug", "elastic", "crop", "shuffle"],
           "scene_aug": {"rotation": {"p": 1.0, "value": [0.0, 0.0, 1.0]}, "jitter": True, "flip": {"p": 0.5}},
           "elastic": {"enabled": True, "value": [[6, 40], [20, 160]], "apply_to_feat": False, "p": 1.0}}
    result = {"reps": args.reps, "workloads": []}
    for name, n, scale, room in (("B4x150k_scale50", 150000, 50, (7.0, 6.0, 3.0)), ("B4x500k_scale100", 500000, 100, (4.5, 4.0, 2.6))):
        cfg = aug.AugConfig.from_cfg({"DATA_AUG": sec, "DATA_PROCESSOR": {"voxel_scale": scale, "full_scale": [128, 512],
                                                                          "max_npoint": 250000, "point_range": 200000000}})
        scenes = [scene(100 + b, n, room) for b in range(4)]
        xyz = torch.from_numpy(np.concatenate([s[0] for s in scenes])).to(dev)
        lab = torch.from_numpy(np.concatenate([s[1] for s in scenes])).to(dev)
        offsets = [n * b for b in range(5)]
        bidx = torch.repeat_interleave(torch.arange(4, device=dev), n)
        real = _lib.lib()
        timed = Timed(real)
        per_call, wall_aug, wall_rigid, kept = {}, [], [], 0

        def rigid(rep):        # what DeviceScenes._rigid + _finish do for these scenes
            rng = np.random.default_rng(rep + 3)
            th = rng.uniform(0.0, 2.0 * np.pi, 4)
            flip = np.where(rng.random(4) < 0.5, -1.0, 1.0)
            coef = np.stack((np.cos(th) * flip, np.sin(th) * flip, -np.sin(th), np.cos(th)), 1).astype(np.float32)
            cf = torch.from_numpy(coef).to(dev, non_blocking=True)[bidx]
            m = torch.stack((xyz[:, 0] * cf[:, 0] + xyz[:, 1] * cf[:, 2], xyz[:, 0] * cf[:, 1] + xyz[:, 1] * cf[:, 3], xyz[:, 2]), 1)
            m += (torch.rand(m.shape, device=dev) - 0.5) * 0.01
            q = m * float(scale)
            lo = torch.stack([q[offsets[b]:offsets[b + 1]].amin(0) for b in range(4)])
            q = (q - lo[bidx]).to(torch.int32)
            top = (q.max(0)[0] + 1).cpu().numpy()
            return torch.cat((bidx.to(torch.int32)[:, None], q), 1), top

        for rep in range(-3, args.reps):            # three warm-up rounds
            draws = [aug.SeededDraws(1000 * (rep + 3) + b) for b in range(4)]
            aug.lib = lambda: timed
            timed.spans = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = aug.augment_batch(xyz, lab, offsets, cfg, draws)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            aug.lib = _lib.lib
            rigid(rep)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep < 0:
                continue
            wall_aug.append((t1 - t0) * 1e3)
            wall_rigid.append((t2 - t1) * 1e3)
            kept = int(out["offsets"][-1])
            seen = {}
            for cname, e0, e1 in timed.spans:
                k = "%s#%d" % (cname, seen.setdefault(cname, 0))
                seen[cname] += 1
                per_call.setdefault(k, []).append(e0.elapsed_time(e1) * 1e3)
        N = 4 * n
        bytes_of = {"doda_aug_affine": N * (12 + 24), "doda_aug_displace": N * (24 + 24), "doda_aug_crop": N * (24 + 1),
                    "doda_aug_emit": N * (12 + 24 + 4) + kept * (16 + 12 + 4)}
        calls = {}
        for k, v in per_call.items():
            us = float(np.median(v))
            b = bytes_of.get(k.split("#")[0])
            calls[k] = {"median_us": round(us, 1), "min_us": round(float(np.min(v)), 1), "calls": len(v)}
            if b:
                calls[k].update(bytes=b, tb_per_s=round(b / (us * 1e-6) / 1e12, 3), share_of_8tbs=round(b / (us * 1e-6) / HBM, 3))
        w = {"name": name, "points": N, "kept": kept, "calls": calls,
             "augment_batch_wall_ms": {"median": round(float(np.median(wall_aug)), 3), "min": round(float(np.min(wall_aug)), 3),
                                       "max": round(float(np.max(wall_aug)), 3)},
             "rigid_finish_wall_ms": {"median": round(float(np.median(wall_rigid)), 3), "min": round(float(np.min(wall_rigid)), 3),
                                      "max": round(float(np.max(wall_rigid)), 3)}}
        result["workloads"].append(w)
        print(json.dumps(w))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Time the virtual-scan stage (doda_amd.vss.run) on one large scene and the scipy restatement of the same stage on the host.

    python tools/vss_bench.py [--step 0.0108] [--repeats 5] [--out FILE]

Prints one JSON line: points, views, the stage's wall time on the device (median and minimum over the repeats, the device
synchronised before and after), the host restatement's time (qhull per view), the windowed / undecided split of the vertex decision
and the mean number of constraints in a query's window (first view)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from doda_amd import aug, vss                 # noqa: E402
from tests import vss_cases as vc             # noqa: E402


def window_sizes(points, camera, radius):
    """Constraints per query of the windowed route for one cloud seen from `camera` (numpy restatement of the 3 x 3 x 3 cells)."""
    flipped = vc.flip(points, camera, radius)
    dmax = float(np.linalg.norm(points - np.asarray(camera), axis=1).max())
    g, hinv, _, theta0 = vss.window_of(radius, dmax * (1 + 1e-9))
    if g == 0:
        return None, 0.0
    unit = flipped / np.linalg.norm(flipped, axis=1, keepdims=True)
    cell = np.clip(((unit + 1.0) * hinv).astype(np.int64), 0, g - 1)
    grid = np.zeros((g + 2,) * 3, dtype=np.int64)
    np.add.at(grid, (cell[:, 0] + 1, cell[:, 1] + 1, cell[:, 2] + 1), 1)
    box = sum(grid[1 + a:g + 1 + a, 1 + b:g + 1 + b, 1 + c:g + 1 + c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    return box[cell[:, 0], cell[:, 1], cell[:, 2]], theta0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=float, default=0.0108)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pts, lab = vc.room(args.step, jitter=args.step / 10)
    xyz32 = (pts - pts.mean(0)).astype(np.float32)
    n = lab.size
    cfg = aug.AugConfig.from_cfg(vc.data_cfg()).vss
    x, l = torch.from_numpy(xyz32).to(dev), torch.from_numpy(lab.astype(np.int32)).to(dev)
    times, out = [], None
    for k in range(args.repeats + 2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = vss.run(x, l, [0, n], cfg, [aug.RandomStateDraws(args.seed)], return_debug=True)
        torch.cuda.synchronize()
        if k >= 2:
            times.append(time.perf_counter() - t)
    stats, sample = out["debug"]["stats"], out["debug"]["samples"][0]
    rs = np.random.RandomState(args.seed)
    rs.rand()
    t = time.perf_counter()
    _, ref_sel, log = vc.virtual_scan(vc.VSS, xyz32, lab, vc.CLASS_NAMES, rs)
    host = time.perf_counter() - t
    same = bool(np.array_equal(out["index"].cpu().numpy(), np.nonzero(ref_sel)[0]))
    camera, interest, _ = sample.log[0]
    _xyz, _ = vc.frame(xyz32, lab != vc.IGNORE)
    f = _xyz - interest
    m = vc.view_mask(f, camera - interest, cfg.mode, cfg.camera_view)
    sizes, theta0 = window_sizes(f[m], camera - interest, cfg.radius)
    res = {"points": int(n), "views": len(stats), "kept": int(out["index"].numel()), "equals_host": same,
           "device_stage_ms_median": round(1e3 * float(np.median(times)), 3), "device_stage_ms_min": round(1e3 * min(times), 3),
           "host_scipy_ms": round(1e3 * host, 1), "view_points": [s["points"] for s in stats],
           "windowed": [s["windowed"] for s in stats], "undecided_then_exhaustive": [s["undecided"] for s in stats],
           "theta0": theta0, "mean_window": None if sizes is None else round(float(sizes.mean()), 1),
           "max_window": None if sizes is None else int(sizes.max()), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

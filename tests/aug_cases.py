"""The cases of tests/golden/aug_golden.npz (made by tests/golden/make_aug_golden.py from the reference's own DataAugmentor), shared
by the maker and the tests: the inputs are regenerated from the seeds, the golden holds what the reference computed from them.
The noise is not stored either: the reference draws from numpy's legacy global stream, which is frozen, so a test replays it
from the case's seed (doda_amd.aug.RandomStateDraws)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aug_golden.npz")
STRIDE = 16                   # fp64 positions are stored for every 16th point
FULL = ["scene_aug", "elastic", "crop", "shuffle"]

# the ScanNet values (cfgs/dataset_cfgs/scannet/scannet_cfg.yaml:18-32,60-65)
_BASE = dict(n=16000, room=(7.0, 6.0, 3.0), aug_list=FULL, voxel_scale=50, jitter=True, flip_p=0.5, rot_p=1.0, rot_value=(0.0, 0.0, 1.0),
             elastic_enabled=True, elastic_p=1.0, elastic_value=((6, 40), (20, 160)), apply_to_feat=False, full_scale=(128, 512),
             max_npoint=250000, point_range=200000000)
CASES = [
    dict(_BASE, seed=201, n=24000, flip_p=1.0),                                        # the full list at scale 50, flipped
    dict(_BASE, seed=202, n=20000, voxel_scale=100, room=(4.5, 4.0, 2.6), flip_p=0.0),  # 1 cm voxels, not flipped
    dict(_BASE, seed=203, room=(11.0, 10.0, 2.8), max_npoint=5000),                     # the crop loop                    
    dict(_BASE, seed=204, room=(11.0, 10.0, 2.8), point_range=40000000, flip_p=0.0),    # the volume rule
    dict(_BASE, seed=205, n=12000, elastic_p=0.0, flip_p=1.0),                          # elastic's p does not fire
    dict(_BASE, seed=206, n=12000, apply_to_feat=True),                                 # the distortion applied to xyz_middle
    dict(_BASE, seed=207, aug_list=["elastic", "crop", "shuffle"]),                     # the list the mixed samples go through
    dict(_BASE, seed=208, n=14000, room=(11.0, 10.0, 2.8), point_range=60000000, max_npoint=4000),   # volume rule, then the loop
]


def scene(case):
    """fp32 [n, 3] points of a room-shaped surface scene centred near the origin (as the reference's preprocessed scans are) and
    int64 labels: floor, ceiling, four walls and a few boxes, with 1 cm of noise."""
    rng = np.random.default_rng(case["seed"])
    n, (sx, sy, sz) = case["n"], case["room"]
    kind = rng.integers(0, 10, n)
    u = rng.random((n, 3)) * np.array([sx, sy, sz])
    u[kind < 3, 2] = 0.0                                   # floor
    u[kind == 3, 2] = sz                                   # ceiling
    u[kind == 4, 0] = 0.0
    u[kind == 5, 0] = sx
    u[kind == 6, 1] = 0.0
    u[kind == 7, 1] = sy
    box = kind >= 8                                        # furniture: points in the lower third
    u[box, 2] *= 0.35
    u += rng.normal(0.0, 0.01, (n, 3))
    u -= u.mean(0)
    lab = np.where(kind < 3, 1, np.where(kind < 8, 0, 2 + kind)).astype(np.int64)
    lab[rng.random(n) < 0.05] = 255
    return u.astype(np.float32), lab


def section(case):
    """The DATA_AUG mapping of a case, with the reference's keys."""
    return {"enabled": True, "aug_list": list(case["aug_list"]),
            "scene_aug": {"rotation": {"p": case["rot_p"], "value": list(case["rot_value"])}, "jitter": case["jitter"],
                          "flip": {"p": case["flip_p"]}},
            "elastic": {"enabled": case["elastic_enabled"], "value": [list(v) for v in case["elastic_value"]],
                        "apply_to_feat": case["apply_to_feat"], "p": case["elastic_p"]},
            "shuffle": True}


def data_cfg(case):
    """A dataset config mapping (what AugConfig.from_cfg takes)."""
    return {"DATA_AUG": section(case),
            "DATA_PROCESSOR": {"voxel_scale": case["voxel_scale"], "full_scale": list(case["full_scale"]), "max_npoint": case["max_npoint"],
                               "point_range": case["point_range"], "voxel_mode": 4}}


def load_case(z, i):
    pre = "c%d_" % i
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}

"""Generates tests/golden/aug_golden.npz in the BUILD container (needs /root/reference and scipy).

    python tests/golden/make_aug_golden.py

The reference's own DataAugmentor (dataset/augmentor/data_augmentor.py) and its scene_aug / elastic / crop
(dataset/augmentor/augmentor_utils.py) are imported from where they lie, with the stand-ins make_tacm_golden.py uses for the
imports this image lacks, and run step by step on seeded scenes under numpy.random.seed(seed); nothing of their text is copied —
the file holds numbers only.  The loaded modules see numpy through a facade that records the kind and size of every draw and the
matrix of the [n, 3] @ [3, 3] product; elastic and crop are wrapped to keep their arguments and results.  `shuffle`, the last
entry of the lists, is not run: it permutes the rows after everything else has been drawn.

Per case: the draws' kinds and sizes, the matrix, the bounds of data_dict['xyz'] at every stage and `bb` per elastic pass, the
crop tests (offset, full_scale, valid count after it — replayed from crop's recorded arguments and draws, and asserted equal to
crop's own result), the kept mask (bit-packed), the kept points' truncated coordinates (int16), which coordinates / points sit
within 1e-6 of an integer / of a crop boundary, fp64 positions and xyz_middle of every 16th point, and `E`, the largest
|coordinate| at any stage.  tests/aug_cases.py regenerates the inputs from the seeds (they are not stored); the noise is
replayed from the seed by the tests (numpy's legacy stream is frozen)."""
import importlib.util
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference"

import aug_cases as ac   # noqa: E402


class Recorder:
    def __init__(self):
        self.draws, self.mat = [], None


class NpRandomFacade:
    def __init__(self, rec):
        self.rec = rec

    def rand(self, *shape):
        v = np.random.rand(*shape)
        self.rec.draws.append(("rand", int(np.size(v))))
        return v

    def randn(self, *shape):
        v = np.random.randn(*shape)
        self.rec.draws.append(("randn", int(np.size(v))))
        return v

    def permutation(self, x):
        raise AssertionError("shuffle is not run by the maker")


class NpFacade:
    def __init__(self, rec):
        self.rec = rec
        self.random = NpRandomFacade(rec)

    def __getattr__(self, name):
        return getattr(np, name)

    def matmul(self, a, b):
        if np.ndim(a) == 2 and np.shape(a)[0] != 3 and np.shape(b) == (3, 3):
            self.rec.mat = np.array(b, dtype=np.float64)
        return np.matmul(a, b)


def load_reference(rec):
    for name in ("open3d", "cv2", "lib", "lib.pointgroup_ops", "lib.pointgroup_ops.functions"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["lib.pointgroup_ops.functions"].pointgroup_ops = None
    spec = importlib.util.spec_from_file_location("ref_augmentor_utils", os.path.join(REF, "dataset/augmentor/augmentor_utils.py"))
    au = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(au)
    au.np = NpFacade(rec)
    for name in ("dataset", "dataset.dataset", "dataset.augmentor"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["dataset.augmentor"].augmentor_utils = au
    sys.modules["dataset.augmentor.augmentor_utils"] = au
    spec = importlib.util.spec_from_file_location("dataset.augmentor.data_augmentor", os.path.join(REF, "dataset/augmentor/data_augmentor.py"))
    da = importlib.util.module_from_spec(spec)
    da.__package__ = "dataset.augmentor"
    spec.loader.exec_module(da)
    return au, da


class Param(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def to_param(v):
    if isinstance(v, dict):
        return Param({k: to_param(x) for k, x in v.items()})
    return v


def near_int(x, eps=1e-6):
    return (np.abs(x - np.rint(x)) <= eps) & (x != 0.0)


def run_case(au, da, rec, case):
    xyz32, lab = ac.scene(case)
    rec.draws, rec.mat = [], None
    log = {"elastic": [], "crop": []}
    ref_elastic, ref_crop = au.elastic, au.crop

    def elastic(x, gran, mag):
        out = ref_elastic(x, gran, mag)
        log["elastic"].append((np.array(x, dtype=np.float64), gran, mag, np.array(out, dtype=np.float64)))
        return out

    def crop(xyz, full_scale, point_range, max_npoint):
        at = len(rec.draws)
        out, valid = ref_crop(xyz, full_scale, point_range, max_npoint)
        log["crop"].append((np.array(xyz, dtype=np.float64), np.array(out, dtype=np.float64), np.array(valid), at))
        return out, valid
    au.elastic, au.crop = elastic, crop
    try:
        np.random.seed(case["seed"])
        aug = da.DataAugmentor(to_param(ac.section(case)), "scannet", ["c%d" % k for k in range(20)], 255, case["voxel_scale"], 4,
                               list(case["full_scale"]), case["point_range"], case["max_npoint"])
        # (a list without scene_aug: the mixed sample arrives in fp64 in the reference; the fp32 points widened)
        dd = {"xyz_middle": xyz32 if "scene_aug" in case["aug_list"] else xyz32.astype(np.float64), "label": lab, "valid": True}
        stages = []
        for name in case["aug_list"]:
            if name == "shuffle":
                continue
            if name == "crop":
                mid_before_crop = np.array(dd["xyz_middle"], dtype=np.float64)
            dd = getattr(aug, name)(cfg=aug.cfg[name] if name in aug.cfg else None, data_dict=dd)
    finally:
        au.elastic, au.crop = ref_elastic, ref_crop
    n = xyz32.shape[0]
    fires = case["elastic_enabled"] and case["elastic_p"] >= 1.0
    assert len(log["elastic"]) == (len(case["elastic_value"]) if fires else 0), "elastic fell back to the undistorted points"
    assert len(log["crop"]) == 1
    # the bounds of data_dict['xyz'] at every stage (before the subtraction of the minimum) and E
    first = log["elastic"][0][0] if fires else None
    if first is None:
        base_mid = mid_before_crop
        first = base_mid * case["voxel_scale"]
    stages = [first] + [e[3] for e in log["elastic"]]
    bounds = np.array([[s.min(0), s.max(0)] for s in stages])
    bb = np.array([np.abs(e[0]).max(0).astype(np.int32) // e[1] + 3 for e in log["elastic"]], dtype=np.int64).reshape(-1, 3)
    xyz_in, xyz_off, valid, at = log["crop"][0]
    assert np.array_equal(xyz_in, stages[-1] - stages[-1].min(0))
    E = max(float(np.abs(s).max()) for s in stages + [xyz_in, xyz_off])
    # crop's tests, replayed from its arguments and its draws, checked against its own result
    crop_draws = rec.draws[at:]
    assert all(d == ("rand", 3) for d in crop_draws)
    rs = np.random.RandomState(case["seed"])
    for kind, size in rec.draws[:at]:
        rs.rand(size) if kind == "rand" else rs.randn(size)
    room = xyz_in.max(0) - xyz_in.min(0)
    full = np.array([case["full_scale"][1]] * 3, dtype=np.float64)
    curr = room[0] * room[1] * room[2]
    tests, v, off, near_pt = [], np.ones(n, dtype=bool), np.zeros(3), np.zeros(n, dtype=bool)
    volume = curr > case["point_range"]
    if volume:
        s = math.sqrt(case["point_range"] / curr)
        full = np.minimum(full, np.array([s * room[0], s * room[1], room[2]]))
        v = (xyz_in < full).sum(1) == 3
        near_pt |= (np.abs(xyz_in - full) <= 1e-6).any(1)
        tests.append((np.zeros(3), full.copy(), int(v.sum())))
    while v.sum() > case["max_npoint"]:
        off = np.clip(full - room + 0.001, None, 0) * rs.rand(3)
        q = xyz_in + off
        v = v & (q.min(1) >= 0) & ((q < full).sum(1) == 3)
        near_pt |= (np.abs(q - full) <= 1e-6).any(1) | ((np.abs(q) <= 1e-6) & (q != 0.0)).any(1)     # (an exact 0 is exact on both sides)
        tests.append((off.copy(), full.copy(), int(v.sum())))
        full[:2] -= 32
    assert len(tests) - int(volume) == len(crop_draws)
    assert np.array_equal(v, valid) and np.array_equal(xyz_in + off if len(crop_draws) else xyz_in, xyz_off)
    kept = xyz_off[valid]
    assert kept.min() >= 0 and kept.max() < 32767 and valid.sum() > 0
    assert np.array_equal(dd["xyz"], kept) and np.array_equal(dd["label"], lab[valid])
    out = {
        "seed": np.array(case["seed"]), "n": np.array(n), "E": np.array(E), "volume": np.array(volume),
        "draw_kinds": np.array([d[0] for d in rec.draws]), "draw_sizes": np.array([d[1] for d in rec.draws], dtype=np.int64),
        "has_mat": np.array(rec.mat is not None), "mat": rec.mat if rec.mat is not None else np.eye(3),
        "bounds": bounds, "bb": bb,
        "crop_offset": np.array([t[0] for t in tests]).reshape(-1, 3), "crop_full": np.array([t[1] for t in tests]).reshape(-1, 3),
        "crop_count": np.array([t[2] for t in tests], dtype=np.int64),
        "kept": np.packbits(valid), "coords": kept.astype(np.int64).astype(np.int16),
        "near_coord": np.packbits(near_int(kept).reshape(-1)), "near_point": np.packbits(near_pt),
        "pos16": xyz_off[::ac.STRIDE].copy(), "mid16": mid_before_crop[::ac.STRIDE].copy(),
    }
    return out, dict(n=n, kept=int(valid.sum()), tests=len(tests), loop=len(crop_draws), volume=bool(volume), fires=fires,
                     flip=bool(rec.mat is not None and case["flip_p"] >= 1.0), E=E, bb=bb.tolist(),
                     near=float(near_int(kept).mean()), near_pt=int(near_pt.sum()))


def main():
    rec = Recorder()
    au, da = load_reference(rec)
    out, infos = {}, []
    for i, case in enumerate(ac.CASES):
        assert 12000 <= case["n"] <= 40000
        o, info = run_case(au, da, rec, case)
        out.update({"c%d_%s" % (i, k): v for k, v in o.items()})
        infos.append(info)
        print("case %d:" % i, info)
    # coverage
    cs = ac.CASES
    assert len(cs) >= 7
    assert any(c["aug_list"] == ac.FULL and c["voxel_scale"] == 50 for c in cs) and any(c["voxel_scale"] == 100 for c in cs)
    assert any(f["loop"] >= 3 for f in infos) and any(f["volume"] for f in infos) and any(not f["fires"] for f in infos)
    assert any(c["apply_to_feat"] for c in cs) and any(c["aug_list"][0] == "elastic" for c in cs)
    assert any(c["flip_p"] >= 1.0 for c in cs) and any(c["flip_p"] <= 0.0 for c in cs)
    assert all(f["near"] <= 1e-4 for f in infos)
    out["n_cases"] = np.array(len(cs))
    path = os.path.join(HERE, "aug_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()

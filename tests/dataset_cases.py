"""Tiny datasets in the three file formats doda_amd.datasets reads, and a numpy restatement of how the reference reads them
(dataset/scannet.py:18-58, dataset/s3dis.py:18-57, dataset/front3d.py:25-62, the class mapper of dataset/dataset.py:52-64, the
unaugmented item of dataset/scannet.py:76-78).  The scene content is doda_amd.scene.make_scene at 3000-6000 voxels; the point counts
are unequal.  Every comparison against this module is exact equality."""
import glob
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPPERS = os.path.join(ROOT, "tests", "golden", "class_mapper")
SCANNET_2_S3DIS = os.path.join(MAPPERS, "scannet_2_s3dis.json")
S3DIS_2_SCANNET = os.path.join(MAPPERS, "s3dis_2_scannet.json")
VOXEL_SCALE = 50
SHIFT = np.array([1.5, 2.25, 0.5])      # the files are not centred


def scene(seed, voxels):
    """(xyz float32 [n, 3] around SHIFT, labels int64 [n]) of a procedural scene."""
    from doda_amd.scene import make_scene
    _, mid, lab = make_scene(seed, voxels, VOXEL_SCALE)
    return (mid + SHIFT.astype(np.float32)).astype(np.float32), lab.astype(np.int64)


def _rgb(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ writers
def write_scannet(folder, name, xyz, label=None, suffix=".pth"):
    """<folder>/<name><suffix>: torch.save of (xyz, rgb, label) — (xyz, rgb) without labels — numpy arrays, as the reference's
    preparation writes them."""
    os.makedirs(folder, exist_ok=True)
    rgb = _rgb(xyz.shape[0], 1)
    path = os.path.join(str(folder), name + suffix)
    torch.save((xyz, rgb) if label is None else (xyz, rgb, label), path)
    return path


def write_rows(path, xyz, label, dtype=np.float64, extra_columns=0):
    """An .npy of rows x y z r g b label (+ extra columns) in `dtype` (the S3DIS and 3D-FRONT formats)."""
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    n = xyz.shape[0]
    rows = np.concatenate([xyz.astype(dtype), _rgb(n, 2).astype(dtype), label.astype(dtype)[:, None],
                           np.zeros((n, extra_columns), dtype=dtype)], 1)
    np.save(str(path), rows)
    return str(path)


def scannet_dataset(root, labels_edit=True):
    """DATA_ROOT with train/ (4 scenes, unequal sizes), val/ (2) and test/ (1, no labels).  The first training scene carries labels
    the mapper does not know (2, 3 stay from make_scene; -1 and 255 are written in), the third only such labels."""
    root = str(root)
    files = {"train": [], "val": [], "test": []}
    for k, (name, voxels) in enumerate([("scene0002_00", 3000), ("scene0000_00", 6000), ("scene0001_01", 4000), ("scene0001_00", 5000)]):
        xyz, lab = scene(100 + k, voxels)
        if labels_edit and k == 0:
            lab[::7], lab[3::11] = -1, 255
        if labels_edit and k == 2:
            lab[:] = 3
        files["train"].append(write_scannet(os.path.join(root, "train"), name, xyz, lab))
    for k, (name, voxels) in enumerate([("scene0011_00", 3000), ("scene0010_00", 4000)]):
        files["val"].append(write_scannet(os.path.join(root, "val"), name, *scene(200 + k, voxels)))
    files["test"].append(write_scannet(os.path.join(root, "test"), "scene0707_00", scene(300, 3000)[0]))
    with open(os.path.join(root, "train", "notes.txt"), "w") as f:      # (not a scene: another suffix)
        f.write("x")
    return files


def s3dis_dataset(root, test_area=5, dtype=np.float64):
    """DATA_ROOT with Area_1 / Area_2 / Area_<test_area> rooms (and a file without `Area_` in its name), float64 rows of 8 columns."""
    root = str(root)
    rooms = [("Area_1_office_2", 3000), ("Area_%d_hallway_1" % test_area, 4000), ("Area_2_office_1", 5000), ("Area_1_conferenceRoom_1", 3500),
             ("Area_%d_office_3" % test_area, 3000)]
    out = {}
    for k, (name, voxels) in enumerate(rooms):
        xyz, lab = scene(400 + k, voxels)
        out[name] = write_rows(os.path.join(root, name + ".npy"), xyz, lab, dtype, extra_columns=1)
    np.save(os.path.join(root, "readme.npy"), np.zeros(3))
    return out


def front3d_dataset(top, suffix=".npy", stretch=None):
    """<top>/density1250 = DATA_ROOT with house directories, <top>/train_list.txt and <top>/val_list.txt (the split files, reached
    through `../`).  stretch: {list line: (sx, sy, sz)} factors on a scene's coordinates."""
    top = str(top)
    root = os.path.join(top, "density1250")
    lines = {"training": ["house_b/room_1.npy", "house_a/room_2.npy", "house_a/room_0.npy"], "validation": ["house_c/room_9.npy"]}
    k = 0
    for split, items in lines.items():
        for item in items:
            xyz, lab = scene(500 + k, 3000 + 500 * k)
            if stretch and item in stretch:
                xyz = (xyz * np.asarray(stretch[item], dtype=np.float32)).astype(np.float32)
            write_rows(os.path.join(root, item)[:-4] + ".npy", xyz, lab, np.float64)
            k += 1
        with open(os.path.join(top, {"training": "train_list.txt", "validation": "val_list.txt"}[split]), "w") as f:
            f.write("".join(item + "\n" for item in items))
    return root, lines


# ------------------------------------------------------------------------------------------------ dataset configs
def _config(d):
    from doda_amd.config import Config
    return Config(d)


PROCESSOR = {"voxel_scale": VOXEL_SCALE, "full_scale": [128, 512], "voxel_mode": 4, "max_npoint": 250000, "point_range": 200000000, "cache": True}


def scannet_cfg(root, mapper=None, test="test", **processor):
    d = {"DATA_ROOT": str(root), "DATASET": "scannet",
         "DATA_SPLIT": {"training": "train", "validation": "val", "test": test, "data_suffix": ".pth"},
         "DATA_CLASS": {"n_classes": 20, "ignore_label": 255, "class_names": ["c%d" % c for c in range(20)]},
         "DATA_PROCESSOR": dict(PROCESSOR, **processor)}
    if mapper:
        d["CLASS_MAPPER_FILE"] = mapper
    return d


def s3dis_cfg(root, mapper=None, test_area=5, **processor):
    d = {"DATA_ROOT": str(root), "DATASET": "s3dis",
         "DATA_SPLIT": {"test_area": test_area, "training": "training", "validation": "validation", "test": "validation"},
         "DATA_CLASS": {"n_classes": 13, "ignore_label": 255}, "DATA_PROCESSOR": dict(PROCESSOR, **processor)}
    if mapper:
        d["CLASS_MAPPER_FILE"] = mapper
    return d


def front3d_cfg(root, suffix=".npy", **processor):
    return {"DATA_ROOT": str(root), "DATASET": "front3d",
            "DATA_SPLIT": {"split_files": {"training": "../train_list.txt", "validation": "../val_list.txt", "test": "../val_list.txt"},
                           "training": "train", "validation": "val", "test": "val", "data_suffix": suffix},
            "DATA_CLASS": {"n_classes": 71, "ignore_label": 255}, "DATA_PROCESSOR": dict(PROCESSOR, **processor)}


def experiment(source, target=None, n_classes=20):
    d = {"COMMON_CLASSES": {"n_classes": n_classes}, "DATA_CONFIG": source}
    if target is not None:
        d["DATA_CONFIG_TAR"] = target
    return _config(d)


def arguments(cache, **kw):
    return SimpleNamespace(scene_cache=str(cache), synthetic_scenes=2, synthetic_base=2, synthetic_voxels=3000, **kw)


# ------------------------------------------------------------------------------------------------ the restatement
def ref_mapper(path):
    """dataset/dataset.py:52-64: ones(256) * 255, then the source classes."""
    if path is None:
        return None
    with open(path, "r") as f:
        info = json.load(f)
    table = np.ones(256, dtype=np.int64) * 255
    for key in info["src"]:
        table[int(key)] = info["classes"].index(info["src"][key])
    return table


def ref_scannet_list(root, folder, suffix=".pth"):
    return sorted(glob.glob(os.path.join(str(root), folder) + "/*" + suffix))


def ref_scannet(path, folder, ignore_label=255, mapper=None):
    """-> (xyz, label) of one file: dataset/scannet.py:45-51 (not centred)."""
    if folder.find("test") < 0:
        xyz, _, label, *_ = torch.load(path, weights_only=False)
    else:
        xyz, _ = torch.load(path, weights_only=False)
        label = np.full(xyz.shape[0], ignore_label)
    if mapper is not None:
        label = mapper[label.astype(np.int64)]
    return xyz.astype(np.float32), label.astype(np.int64)


def ref_s3dis_list(root, split_value, test_area):
    names = [item[:-4] for item in sorted(os.listdir(str(root))) if "Area_" in item]
    tag = "Area_{}".format(test_area)
    return [n for n in names if (tag not in n) == (split_value == "training")]


def ref_rows(path, mapper=None):
    """-> (xyz, label) of one S3DIS / 3D-FRONT .npy: columns 0:3 and 6, the mapper, then `xyz -= xyz.mean(0)` over all points in
    the file's dtype (dataset/s3dis.py:43-57, dataset/front3d.py:46-62), then float32 (the collate's cast)."""
    data = np.load(path)
    xyz, label = data[:, 0:3], data[:, 6]
    if mapper is not None:
        label = mapper[label.astype(np.int64)]
    xyz -= xyz.mean(0)
    return xyz.astype(np.float32), label.astype(np.int64)


def ref_front3d_list(root, split_file, suffix=".npy"):
    with open(os.path.normpath(os.path.join(str(root), split_file)), "r") as f:
        items = [line.strip() for line in f.readlines()]
    return [os.path.join(str(root), item)[:-4] + suffix for item in items]


def ref_item(xyz_mid, label, index, voxel_scale=VOXEL_SCALE):
    """The unaugmented item (dataset/scannet.py:76-78) in the types doda_amd.loader.host_collate takes: voxel coordinates
    `xyz_mid * scale - min` truncated, xyz_mid, labels, index."""
    v = xyz_mid * np.float32(voxel_scale)
    v -= v.min(0)
    return torch.from_numpy(v.astype(np.int32)), torch.from_numpy(xyz_mid), torch.from_numpy(label.astype(np.int32)), int(index)


def pool(paths):
    """[(xyz_mid, labels)] of pool files."""
    out = []
    for p in paths:
        with np.load(p) as f:
            assert f["xyz_mid"].dtype == np.float32 and f["labels"].dtype == np.int64
            out.append((f["xyz_mid"], f["labels"]))
    return out

"""The reference's three file datasets as pools of base scenes.

Reference: dataset/scannet.py:18-58, dataset/s3dis.py:18-57, dataset/front3d.py:25-62 and the class mapper of
dataset/dataset.py:52-64.  There a Dataset object reads a scene in __getitem__ (or attaches to a SharedArray copy of it); here a
scene is read ONCE, converted into the pool format every loader of this package already reads — `<stem>.npz` with `xyz_mid`
float32 [n, 3] and `labels` int64 [n] (doda_amd.loader.prepare_cache) — and everything downstream (the HBM-resident loaders, the
worker loader, pseudo labels, full-cloud scoring) runs on the pool, whatever filled it.

  scannet   sorted glob of DATA_ROOT/<DATA_SPLIT[split]>/*<data_suffix>; a file is a torch.load tuple (xyz, rgb, label, *others),
            or (xyz, rgb) where the split's directory name contains `test` (every label is then ignore_label); not centred
  s3dis     sorted listdir of DATA_ROOT, names containing `Area_`, split by DATA_SPLIT.test_area; `<name>.npy` rows of at least 7
            columns, xyz = [:, 0:3], label = [:, 6]; centred on the mean of all points in the array's own dtype, then float32
  front3d   the lines of normpath(DATA_ROOT / DATA_SPLIT.split_files[split]); file join(DATA_ROOT, line)[:-4] + data_suffix;
            `.npy` rows of 7 columns, centred as s3dis; `.ply` needs the plyfile package: an error here

A scene's name is its file stem (doda_amd.pseudo_labels.scene_name): stems must be unique within a split and hold no dot.

No real scan was available when this was written: the formats are the reference's reading expressions, restated."""
import functools
import glob
import hashlib
import json
import os
import shutil
import tempfile
import zipfile

import numpy as np

KINDS = ("synthetic", "scannet", "s3dis", "front3d")
SPLIT_KEYS = {"train": "training", "target": "training", "val": "validation", "test": "test"}     # dataset/__init__.py:125-164, tool/test.py
BASE_SEEDS = {"train": 1000, "target": 501000, "val": 901000, "test": 901000}                    # (as loader.synthetic_dataset's)
MIN_EXTENT_VOXELS = 64      # front3d: a training sample spanning fewer voxels on an axis is drawn again (dataset/front3d.py:80-81)
POOL_VERSION = 1
INLINE_BYTES = 64 << 20     # sources smaller than this in total are converted in this process: starting a pool costs more


# ------------------------------------------------------------------------------------------------ configs
def dataset_config(cfg, split, eval_src=False):
    """The dataset config of a split: DATA_CONFIG for `train`; DATA_CONFIG_TAR for `target`, `val` and `test` where the experiment
    has one (and not eval_src: doda_amd.test --eval_src), else DATA_CONFIG."""
    if split not in SPLIT_KEYS:
        raise ValueError("split %r: one of %s" % (split, sorted(SPLIT_KEYS)))
    if split == "train" or eval_src or "DATA_CONFIG_TAR" not in cfg:
        return cfg.DATA_CONFIG
    return cfg.DATA_CONFIG_TAR


def kind_of(dataset_cfg):
    """DATASET of a dataset config (absent: synthetic); an unknown kind raises."""
    kind = dataset_cfg.get("DATASET", None) or "synthetic"
    if kind not in KINDS:
        raise ValueError("DATASET: %r is not one of %s" % (kind, ", ".join(KINDS)))
    return kind


# ------------------------------------------------------------------------------------------------ class mapper
def load_class_mapper(path):
    """CLASS_MAPPER_FILE -> (int64 [256] table filled with 255, table[int(k)] = classes.index(src[k]); the common class names)."""
    with open(path, "r") as f:
        info = json.load(f)
    classes = list(info["classes"])
    table = np.full(256, 255, dtype=np.int64)
    for k, name in info["src"].items():
        table[int(k)] = classes.index(name)
    return table, classes


def map_labels(label, table, n_classes, ignore_label, fname):
    """table[label] (numpy indexing: a negative label counts from the end, as in the reference) — or the labels as int64 without a
    table —, then the check every later kernel relies on: a label is a class below n_classes or ignore_label."""
    label = np.asarray(label).astype(np.int64)
    if table is not None:
        try:
            label = table[label]
        except IndexError:
            raise ValueError("%s: label %d is outside the class mapper's 256 entries" % (fname, int(label[np.abs(label).argmax()]))) from None
    bad = ((label < 0) | (label >= int(n_classes))) & (label != int(ignore_label))
    if bad.any():
        raise ValueError("%s: label %d is neither a class below %d nor ignore_label %d%s"
                         % (fname, int(label[bad][0]), int(n_classes), int(ignore_label), "" if table is not None else " (no CLASS_MAPPER_FILE)"))
    return label


# ------------------------------------------------------------------------------------------------ readers
def read_scannet(path, labelled=True, ignore_label=255):
    """-> (xyz float32 [n, 3], uncentred: the files are; raw labels).  The files pickle numpy arrays, so torch.load runs with
    weights_only=False, which executes what the pickle says: point DATA_ROOT at your own prepared data only."""
    import torch
    data = torch.load(path, weights_only=False)
    if labelled:
        xyz, label = data[0], data[2]
    else:
        xyz, _ = data
        label = np.full(xyz.shape[0], ignore_label)
    return np.ascontiguousarray(np.asarray(xyz), dtype=np.float32), np.asarray(label)


def read_s3dis(path):
    """-> (xyz float32 [n, 3] centred on the mean of ALL points, the subtraction in the array's own dtype; raw labels)."""
    data = np.load(path)
    xyz, label = data[:, 0:3], data[:, 6]
    xyz -= xyz.mean(0)
    return np.ascontiguousarray(xyz, dtype=np.float32), label


def read_front3d(path):
    """As read_s3dis on [n, 7] rows (the reference takes a contiguous copy of the columns first).  numpy arrays only: the
    reference's allow_pickle=True is not passed on."""
    data = np.load(path)
    xyz, label = np.ascontiguousarray(data[:, :3]), np.ascontiguousarray(data[:, 6], dtype=np.int64)
    xyz -= xyz.mean(0)
    return np.ascontiguousarray(xyz, dtype=np.float32), label


# ------------------------------------------------------------------------------------------------ scene lists
def scannet_scenes(dataset_cfg, split_key):
    """[(source file, reader)] of a scannet dataset config, in the reference's order."""
    sp = dataset_cfg.DATA_SPLIT
    folder = str(sp[split_key])
    files = sorted(glob.glob(os.path.join(str(dataset_cfg.DATA_ROOT), folder) + "/*" + str(sp.data_suffix)))
    labelled = folder.find("test") < 0
    ignore = int(dataset_cfg.DATA_CLASS.ignore_label)
    return [(f, functools.partial(read_scannet, f, labelled, ignore)) for f in files]


def s3dis_scenes(dataset_cfg, split_key):
    sp, root = dataset_cfg.DATA_SPLIT, str(dataset_cfg.DATA_ROOT)
    names = [item[:-4] for item in sorted(os.listdir(root)) if "Area_" in item]
    area = "Area_{}".format(sp.test_area)
    if sp[split_key] == "training":
        names = [n for n in names if area not in n]
    else:
        names = [n for n in names if area in n]
    files = [os.path.join(root, n + ".npy") for n in names]
    return [(f, functools.partial(read_s3dis, f)) for f in files]


def front3d_scenes(dataset_cfg, split_key):
    sp, root = dataset_cfg.DATA_SPLIT, str(dataset_cfg.DATA_ROOT)
    suffix = str(sp.data_suffix)
    if suffix == ".ply":
        raise NotImplementedError("front3d data_suffix .ply: reading it needs the plyfile package, which this package does not use; "
                                  "convert the scenes to .npy rows (x y z r g b label) and set DATA_SPLIT.data_suffix: .npy")
    if suffix != ".npy":
        raise ValueError("front3d data_suffix %r: .npy" % suffix)
    with open(os.path.normpath(os.path.join(root, str(sp.split_files[split_key]))), "r") as f:
        items = [line.strip() for line in f.readlines()]
    files = [os.path.join(root, item)[:-4] + suffix for item in items if item]
    return [(f, functools.partial(read_front3d, f)) for f in files]


SCENES = {"scannet": scannet_scenes, "s3dis": s3dis_scenes, "front3d": front3d_scenes}


def scene_stem(path):
    return os.path.basename(str(path))[:-4]


def check_stems(files):
    """Scene names are file stems (pseudo labels and --save_to_file name their files by them): unique, and without a dot."""
    seen = {}
    for f in files:
        stem = scene_stem(f)
        if "." in stem or not stem:
            raise ValueError("scene file %s: the stem %r holds a dot (a scene's name is its file name up to the first dot)" % (f, stem))
        if stem in seen:
            raise ValueError("scene files %s and %s have the same stem %r" % (seen[stem], f, stem))
        seen[stem] = f


# ------------------------------------------------------------------------------------------------ the pool
def cache_root(scene_cache=None):
    if scene_cache is not None:
        return str(scene_cache)
    root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    return os.path.join(root, "doda_amd_files_%d" % os.getuid())


def file_hash(path):
    if path is None:
        return "none"
    with open(path, "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()


def pool_path(root, kind, src, mapper_hash, extra=()):
    """<root>/<kind>_<key>/<stem>.npz; the key: kind, absolute source path, its size and mtime_ns, the mapper file's hash (and what
    else decides the converted bytes: `extra`).  A changed source or mapper is another directory: nothing stale is ever read."""
    st = os.stat(src)
    key = repr((POOL_VERSION, kind, os.path.abspath(src), st.st_size, st.st_mtime_ns, mapper_hash, tuple(extra)))
    return os.path.join(root, "%s_%s" % (kind, hashlib.sha1(key.encode()).hexdigest()[:20]), scene_stem(src) + ".npz")


def _convert(job):
    """(worker of fill_pool) one source scene -> its pool file, through a temporary name."""
    dst, src, reader, mapper_file, n_classes, ignore_label = job
    if os.path.exists(dst):
        return dst
    table = load_class_mapper(mapper_file)[0] if mapper_file is not None else None
    xyz, label = reader()
    label = map_labels(label, table, n_classes, ignore_label, src)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or label.shape != (xyz.shape[0],):
        raise ValueError("%s: xyz %s and labels %s" % (src, xyz.shape, label.shape))
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    tmp = dst + ".tmp.%d.npz" % os.getpid()
    np.savez(tmp, xyz_mid=np.ascontiguousarray(xyz, dtype=np.float32), labels=label.astype(np.int64))
    os.replace(tmp, dst)
    return dst


def fill_pool(jobs, procs=None):
    """Convert what is missing, in at most 16 processes (small datasets: in this one)."""
    todo = [j for j in jobs if not os.path.exists(j[0])]
    if not todo:
        return 0
    procs = min(len(todo), procs or min(16, os.cpu_count() or 1))
    if procs > 1 and sum(os.path.getsize(j[1]) for j in todo) >= INLINE_BYTES:
        import multiprocessing as mp
        with mp.get_context("forkserver").Pool(procs) as pool:
            pool.map(_convert, todo)
    else:
        for j in todo:
            _convert(j)
    return len(todo)


def pool_points(path):
    """Points of a pool file, from the header of its labels array."""
    with zipfile.ZipFile(path) as z, z.open("labels.npy") as f:
        version = np.lib.format.read_magic(f)
        shape = (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(f)[0]
    return int(shape[0])


def file_dataset(cfg, dataset_cfg, args, split, log=None):
    """The FileScenes of a split of a scannet / s3dis / front3d dataset config: lists the scenes, converts the missing ones into the
    pool (a second run reads no source file) and logs what the pool holds."""
    from .loader import FileScenes
    kind = kind_of(dataset_cfg)
    split_key = SPLIT_KEYS[split]
    scenes = SCENES[kind](dataset_cfg, split_key)
    if not scenes:
        raise FileNotFoundError("DATASET %s, split %s (%s): no scene under DATA_ROOT %s" % (kind, split, split_key, dataset_cfg.DATA_ROOT))
    check_stems([f for f, _ in scenes])
    mapper_file = dataset_cfg.get("CLASS_MAPPER_FILE", None)
    ignore = int(dataset_cfg.DATA_CLASS.ignore_label)
    class_names = list(dataset_cfg.DATA_CLASS.get("class_names", None) or [])
    n_classes = int(dataset_cfg.DATA_CLASS.n_classes)
    if mapper_file is not None:
        class_names = load_class_mapper(mapper_file)[1]
        n_classes = len(class_names)
    common = cfg.get("COMMON_CLASSES", None)
    if common is not None and int(common.n_classes) != n_classes:
        raise ValueError("COMMON_CLASSES.n_classes is %d and the %s labels of split %s have %d classes (%s)"
                         % (int(common.n_classes), kind, split, n_classes, mapper_file or "no CLASS_MAPPER_FILE"))
    root, mhash = cache_root(getattr(args, "scene_cache", None)), file_hash(mapper_file)
    labelled = not (kind == "scannet" and str(dataset_cfg.DATA_SPLIT[split_key]).find("test") >= 0)
    jobs = [(pool_path(root, kind, src, mhash, (labelled, ignore)), src, reader, mapper_file, n_classes, ignore) for src, reader in scenes]
    converted = fill_pool(jobs)
    paths = [j[0] for j in jobs]
    if log is not None:
        points = sum(pool_points(p) for p in paths)
        log("Dataset %s, split %s (%s) under %s: %d scenes, %d points, %d bytes in HBM; pool %s (%d converted now); "
            "one epoch is one pass, the --synthetic_* flags are ignored"
            % (kind, split, split_key, dataset_cfg.DATA_ROOT, len(paths), points, 16 * points, root, converted))
    training = split in ("train", "target")
    ds = FileScenes(paths, len(paths), dataset_cfg.DATA_PROCESSOR.voxel_scale, seed=BASE_SEEDS[split], augment=training)
    ds.kind, ds.class_names, ds.sources = kind, class_names, [src for src, _ in scenes]
    ds.min_extent = MIN_EXTENT_VOXELS if (kind == "front3d" and training) else 0
    return ds


if __name__ == "__main__":   # python -m doda_amd.datasets --clean : empty the default pool of converted scenes of this user on this node
    import sys
    if "--clean" in sys.argv:
        shutil.rmtree(cache_root(), ignore_errors=True)

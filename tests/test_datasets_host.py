"""doda_amd.datasets and loader.dataset_for on the CPU: the scene lists, splits, labels and centring of the three file formats against
the numpy restatement of the reference's readers (tests/dataset_cases.py, exact equality), the error cases, the pool's cache key and
the dispatch on DATASET."""
import os

import numpy as np
import pytest

from tests import dataset_cases as dc


def _stems(paths):
    return [os.path.basename(p).split(".")[0] for p in paths]


@pytest.fixture(scope="module")
def scannet(tmp_path_factory):
    root = tmp_path_factory.mktemp("scannet")
    return root, dc.scannet_dataset(root)


@pytest.fixture(scope="module")
def s3dis(tmp_path_factory):
    root = tmp_path_factory.mktemp("s3dis")
    return root, dc.s3dis_dataset(root)


# ------------------------------------------------------------------------------------------------ scannet
def test_scannet_lists_and_reads_like_the_reference(scannet, tmp_path):
    from doda_amd.loader import dataset_for
    root, files = scannet
    cfg = dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=8)
    args = dc.arguments(tmp_path)
    logs = []
    mapper = dc.ref_mapper(dc.SCANNET_2_S3DIS)
    for split, folder in (("train", "train"), ("val", "val"), ("test", "test")):
        ds = dataset_for(cfg, args, split, log=logs.append)
        want = dc.ref_scannet_list(root, folder)
        assert len(want) == len(files[folder]) and want == sorted(want)
        assert _stems(ds.paths) == _stems(want) and list(ds.sources) == want
        assert ds.length == len(want) and ds.voxel_scale == 50 and ds.augment == (split == "train") and ds.kind == "scannet"
        assert list(ds.class_names) == ["wall", "floor", "chair", "sofa", "table", "door", "window", "bookshelf"]
        for (xyz, lab), src in zip(dc.pool(ds.paths), want):
            rx, rl = dc.ref_scannet(src, folder, 255, mapper)
            assert np.array_equal(xyz.view(np.uint32), rx.view(np.uint32)) and np.array_equal(lab, rl)
            assert abs(float(xyz[:, 0].mean()) - 1.5) < 0.2 and abs(float(xyz[:, 1].mean()) - 2.25) < 0.2      # not centred
            if folder == "test":
                assert (lab == 255).all()
    assert _stems(dataset_for(cfg, args, "train").paths) == ["scene0000_00", "scene0001_00", "scene0001_01", "scene0002_00"]
    assert len(logs) == 3 and "scannet" in logs[0] and "4 scenes" in logs[0] and "synthetic" in logs[0]
    # the labels the mapper does not know: classes 2 and 3, the negative label (numpy counts it from the end: entry 255) and 255
    raw = dc.ref_scannet(files["train"][0], "train")[1]
    got = dc.pool([p for p in dataset_for(cfg, args, "train").paths if "scene0002_00" in p])[0][1]
    assert (raw == -1).any() and (raw == 2).any() and (raw == 255).any()
    assert (got[(raw == -1) | (raw == 2) | (raw == 3) | (raw == 255)] == 255).all() and (got[raw == 4] == 2).all() and (got[raw == 0] == 0).all()
    all_unknown = dc.pool([p for p in dataset_for(cfg, args, "train").paths if "scene0001_01" in p])[0][1]
    assert (all_unknown == 255).all()


def test_a_label_out_of_range_names_the_file(scannet, tmp_path):
    from doda_amd.loader import dataset_for
    root, files = scannet
    # without a mapper the first training scene's -1 is neither a class nor ignore_label
    with pytest.raises(ValueError, match="scene0002_00"):
        dataset_for(dc.experiment(dc.scannet_cfg(root)), dc.arguments(tmp_path / "a"), "train")
    # the validation scenes hold the classes 0..6 of 20: fine without a mapper, out of range for 5 classes
    cfg = dc.experiment(dc.scannet_cfg(root))
    assert dataset_for(cfg, dc.arguments(tmp_path / "b"), "val").length == 2
    five = dc.scannet_cfg(root)
    five["DATA_CLASS"]["n_classes"] = 5
    with pytest.raises(ValueError, match="scene0010_00"):
        dataset_for(dc.experiment(five, n_classes=5), dc.arguments(tmp_path / "c"), "val")
    # a label past the mapper's 256 entries
    bad = tmp_path / "bad"
    xyz, lab = dc.scene(7, 3000)
    lab[5] = 300
    dc.write_scannet(bad / "train", "scene0900_00", xyz, lab)
    with pytest.raises(ValueError, match="scene0900_00"):
        dataset_for(dc.experiment(dc.scannet_cfg(bad, dc.SCANNET_2_S3DIS), n_classes=8), dc.arguments(tmp_path / "d"), "train")
    # the mapper's classes and COMMON_CLASSES must agree
    with pytest.raises(ValueError, match="COMMON_CLASSES"):
        dataset_for(dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=20), dc.arguments(tmp_path / "e"), "train")


def test_duplicate_and_dotted_stems_raise(tmp_path):
    from doda_amd import datasets
    from doda_amd.loader import dataset_for
    with pytest.raises(ValueError, match="same stem"):
        datasets.check_stems(["/a/house_1/room_0.npy", "/a/house_2/room_0.npy"])
    top = tmp_path / "front"
    root, _ = dc.front3d_dataset(top)
    with open(top / "train_list.txt", "a") as f:
        f.write("house_c/room_0.npy\n")      # house_a/room_0 is in the list already
    xyz, lab = dc.scene(1, 3000)
    dc.write_rows(os.path.join(root, "house_c", "room_0.npy"), xyz, lab)
    with pytest.raises(ValueError, match="room_0"):
        dataset_for(dc.experiment(dc.front3d_cfg(root), n_classes=71), dc.arguments(tmp_path / "cache"), "train")
    dotted = tmp_path / "dotted"
    dc.write_scannet(dotted / "train", "scene.v2", xyz, lab)
    with pytest.raises(ValueError, match="dot"):
        dataset_for(dc.experiment(dc.scannet_cfg(dotted)), dc.arguments(tmp_path / "cache"), "train")


# ------------------------------------------------------------------------------------------------ s3dis
@pytest.mark.parametrize("test_area", [5, 1])
def test_s3dis_splits_by_test_area_and_centres_in_float64(s3dis, tmp_path, test_area):
    from doda_amd.loader import dataset_for
    root, files = s3dis
    cfg = dc.experiment(dc.scannet_cfg(tmp_path), dc.s3dis_cfg(root, dc.S3DIS_2_SCANNET, test_area=test_area, downsampling_scale=4), n_classes=8)
    args = dc.arguments(tmp_path / "cache")
    mapper = dc.ref_mapper(dc.S3DIS_2_SCANNET)
    seen = []
    for split, value in (("target", "training"), ("val", "validation"), ("test", "validation")):
        ds = dataset_for(cfg, args, split)
        names = dc.ref_s3dis_list(root, value, test_area)
        assert _stems(ds.paths) == names and len(names) > 0 and ds.kind == "s3dis"
        assert all(("Area_%d" % test_area in n) == (value != "training") for n in names)
        for (xyz, lab), name in zip(dc.pool(ds.paths), names):
            assert np.load(files[name]).dtype == np.float64
            rx, rl = dc.ref_rows(files[name], mapper)
            assert np.array_equal(xyz.view(np.uint32), rx.view(np.uint32)) and np.array_equal(lab, rl)
            assert np.abs(xyz.mean(0)).max() < 1e-5
            # centring after the cast is another array: the order is part of the format
            late = np.load(files[name])[:, 0:3].astype(np.float32)
            late -= late.mean(0)
            assert not np.array_equal(late, xyz)
            assert set(np.unique(lab)) <= set(range(8)) | {255} and (lab == 255).any() and (lab != 255).any()
        seen += names
    assert sorted(set(seen)) == sorted(files)


# ------------------------------------------------------------------------------------------------ front3d
def test_front3d_reads_its_split_file_through_a_parent_directory(tmp_path):
    from doda_amd.loader import dataset_for
    root, lines = dc.front3d_dataset(tmp_path / "front")
    cfg = dc.experiment(dc.front3d_cfg(root), n_classes=71)
    args = dc.arguments(tmp_path / "cache")
    for split, key, name in (("train", "training", "train_list.txt"), ("val", "validation", "val_list.txt")):
        ds = dataset_for(cfg, args, split)
        want = dc.ref_front3d_list(root, "../" + name)
        assert [os.path.relpath(w, root) for w in want] == lines[key]      # the list's order, not the sorted one
        assert _stems(ds.paths) == _stems(want) and list(ds.sources) == want
        assert ds.min_extent == (64 if split == "train" else 0) and ds.kind == "front3d"
        for (xyz, lab), src in zip(dc.pool(ds.paths), want):
            rx, rl = dc.ref_rows(src)
            assert np.array_equal(xyz.view(np.uint32), rx.view(np.uint32)) and np.array_equal(lab, rl)


def test_front3d_ply_is_a_clear_error(tmp_path):
    from doda_amd.loader import dataset_for
    root, _ = dc.front3d_dataset(tmp_path / "front")
    with pytest.raises(NotImplementedError, match="plyfile"):
        dataset_for(dc.experiment(dc.front3d_cfg(root, suffix=".ply"), n_classes=71), dc.arguments(tmp_path / "cache"), "train")


# ------------------------------------------------------------------------------------------------ the pool
def test_the_pool_is_read_again_and_follows_its_sources(scannet, tmp_path, monkeypatch):
    from doda_amd import datasets
    from doda_amd.loader import dataset_for
    root, files = scannet
    args = dc.arguments(tmp_path / "cache")
    cfg = dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=8)
    first = dataset_for(cfg, args, "val")
    calls = []
    real = datasets.read_scannet

    def counted(path, *a):
        calls.append(path)
        return real(path, *a)

    def refuse(*a, **k):
        raise AssertionError("a source file was read")
    # a second run reads no source file
    for name in ("read_scannet", "read_s3dis", "read_front3d"):
        monkeypatch.setattr(datasets, name, refuse)
    again = dataset_for(cfg, args, "val")
    assert again.paths == first.paths and all(os.path.exists(p) for p in again.paths)
    assert not [f for p in again.paths for f in os.listdir(os.path.dirname(p)) if ".tmp." in f]
    # touching a source file converts that file again, and only that one
    monkeypatch.setattr(datasets, "read_scannet", counted)
    st = os.stat(files["val"][0])
    os.utime(files["val"][0], ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    touched = dataset_for(cfg, args, "val")
    assert calls == [files["val"][0]]
    changed = [a != b for a, b in zip(touched.paths, first.paths)]
    assert changed == [_stems([p]) == _stems([files["val"][0]]) for p in first.paths] and sum(changed) == 1
    assert _stems(touched.paths) == _stems(first.paths)
    # another mapper (other bytes, here the same table) converts everything again
    del calls[:]
    other = tmp_path / "mapper.json"
    other.write_text(open(dc.SCANNET_2_S3DIS).read() + "\n")
    swapped = dataset_for(dc.experiment(dc.scannet_cfg(root, str(other)), n_classes=8), args, "val")
    assert sorted(calls) == sorted(files["val"]) and not set(swapped.paths) & set(touched.paths)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(dc.pool(swapped.paths), dc.pool(touched.paths)))
    # and a mapper that maps otherwise gives other labels
    del calls[:]
    plain = dataset_for(dc.experiment(dc.scannet_cfg(root)), args, "val")
    assert len(calls) == 2 and not all(np.array_equal(a[1], b[1]) for a, b in zip(dc.pool(plain.paths), dc.pool(touched.paths)))
    assert datasets.pool_points(plain.paths[0]) == dc.pool(plain.paths)[0][1].shape[0]


def test_conversion_in_worker_processes(scannet, tmp_path, monkeypatch):
    """The process pool of a large dataset (forced here by a byte threshold of zero) writes the same files."""
    from doda_amd import datasets
    from doda_amd.loader import dataset_for
    root, _ = scannet
    cfg = dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=8)
    here = dataset_for(cfg, dc.arguments(tmp_path / "here"), "val")
    monkeypatch.setattr(datasets, "INLINE_BYTES", 0)
    there = dataset_for(cfg, dc.arguments(tmp_path / "there"), "val")
    for a, b in zip(dc.pool(here.paths), dc.pool(there.paths)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_worker_loader_reads_the_same_pool(scannet, tmp_path):
    """--host_loader's DataLoader over a file pool (in-process here): host_collate of the restated items."""
    import torch
    from doda_amd.loader import dataset_for, host_collate, host_loader
    root, _ = scannet
    ds = dataset_for(dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=8), dc.arguments(tmp_path), "val")
    dl, _ = host_loader(ds, 2, 0, 1, 0, shuffle=False, seed=ds.seed)
    batches = list(dl)
    mapper = dc.ref_mapper(dc.SCANNET_2_S3DIS)
    want = host_collate([dc.ref_item(*dc.ref_scannet(f, "val", 255, mapper), k) for k, f in enumerate(dc.ref_scannet_list(root, "val"))])
    assert len(batches) == 1 and set(batches[0]) == set(want) and batches[0]["id"] == [0, 1]
    for key in ("locs32", "locs_float", "labels32", "offsets"):
        assert torch.equal(batches[0][key], want[key]), key
    assert np.array_equal(batches[0]["spatial_shape"], want["spatial_shape"])


# ------------------------------------------------------------------------------------------------ dispatch
def test_synthetic_dispatch_is_synthetic_dataset(tmp_path, monkeypatch):
    from doda_amd import train as tr
    from doda_amd.loader import SyntheticScenes, dataset_for, synthetic_dataset
    monkeypatch.chdir(dc.ROOT)
    _, cfg = tr.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml"])
    assert cfg.DATA_CONFIG.DATASET == "synthetic"
    no_key = dc.experiment({k: v for k, v in cfg.DATA_CONFIG.items() if k != "DATASET"})
    args = dc.arguments(tmp_path)
    for c in (cfg, no_key):
        for split in ("train", "target", "val"):
            got, want = dataset_for(c, args, split), synthetic_dataset(c, args, split)
            assert type(got) is type(want) is SyntheticScenes
            assert (got.paths, got.length, got.seed, got.voxel_scale, got.augment) == (want.paths, want.length, want.seed, want.voxel_scale, want.augment)
    assert dataset_for(cfg, args, "test").paths == synthetic_dataset(cfg, args, "val").paths


def test_unknown_dataset_kind_lists_the_four(tmp_path):
    from doda_amd.loader import dataset_for
    cfg = dc.experiment(dict(dc.scannet_cfg(tmp_path), DATASET="kitti"))
    with pytest.raises(ValueError) as e:
        dataset_for(cfg, dc.arguments(tmp_path), "train")
    assert all(kind in str(e.value) for kind in ("synthetic", "scannet", "s3dis", "front3d", "kitti"))


def test_split_keys_and_dataset_configs(tmp_path):
    from doda_amd import datasets
    both = dc.experiment(dc.scannet_cfg(tmp_path / "s"), dc.s3dis_cfg(tmp_path / "t"))
    one = dc.experiment(dc.scannet_cfg(tmp_path / "s"))
    assert datasets.SPLIT_KEYS == {"train": "training", "target": "training", "val": "validation", "test": "test"}
    assert [datasets.dataset_config(both, s).DATASET for s in ("train", "target", "val", "test")] == ["scannet", "s3dis", "s3dis", "s3dis"]
    assert datasets.dataset_config(both, "test", eval_src=True).DATASET == "scannet"
    assert [datasets.dataset_config(one, s).DATASET for s in ("train", "val", "test")] == ["scannet"] * 3


def test_file_dataset_configs_parse(monkeypatch):
    from doda_amd import st, train as tr
    from doda_amd import test as dt
    monkeypatch.chdir(dc.ROOT)
    for mod, name, src, tar in ((tr, "scannet", "scannet", "scannet"), (tr, "da_scannet_s3dis", "scannet", "s3dis"),
                                (st, "da_scannet_s3dis_st", "scannet", "s3dis"), (dt, "da_scannet_s3dis_eval", "scannet", "s3dis")):
        _, cfg = mod.parse_config(["--cfg_file", "doda_amd/cfgs/files/%s.yaml" % name])
        assert (cfg.DATA_CONFIG.DATASET, cfg.DATA_CONFIG_TAR.DATASET) == (src, tar)
        assert cfg.DATA_CONFIG.DATA_PROCESSOR.cache is False
    assert cfg.DATA_CONFIG_TAR.DATA_PROCESSOR.downsampling_scale == 4 and cfg.DATA_CONFIG_TAR.DATA_PROCESSOR.no_downsample_infer is True
    assert cfg.COMMON_CLASSES.n_classes == 8 and cfg.DATA_CONFIG.CLASS_MAPPER_FILE.endswith("scannet_2_s3dis.json")

"""The file datasets on the MI355X: the HBM-resident loader over a ScanNet-format pool against host_collate of the restated items
(tests/dataset_cases.py, exact equality), `python -m doda_amd.train`, `doda_amd.st` and `doda_amd.test` on tiny ScanNet- and
S3DIS-format datasets with the reference's class mapper files, and the 3D-FRONT rule that a narrow training sample is drawn again."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_cases as dc

pytestmark = pytest.mark.gpu
ROOT = dc.ROOT


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ device collate
def test_device_batch_equals_host_collate_of_the_restated_items(native_lib, tmp_path):
    from doda_amd.loader import DeviceScenes, dataset_for, host_collate
    root = tmp_path / "scannet"
    small, big, ignored = dc.scene(11, 3000), dc.scene(12, 6000), dc.scene(13, 5000)
    ignored[1][:] = 255
    for name, (xyz, lab) in (("scene0003_00", big), ("scene0001_00", small), ("scene0002_00", ignored)):
        dc.write_scannet(root / "train", name, xyz, lab)
    ds = dataset_for(dc.experiment(dc.scannet_cfg(root, dc.SCANNET_2_S3DIS), n_classes=8), dc.arguments(tmp_path / "cache"), "train")
    mapper = dc.ref_mapper(dc.SCANNET_2_S3DIS)
    want_files = dc.ref_scannet_list(root, "train")
    assert [os.path.basename(f) for f in want_files] == ["scene0001_00.pth", "scene0002_00.pth", "scene0003_00.pth"]
    items = [dc.ref_item(*dc.ref_scannet(f, "train", 255, mapper), k) for k, f in enumerate(want_files)]
    assert items[0][0].shape[0] < items[2][0].shape[0] and bool((items[1][2] == 255).all()) and bool((items[0][2] != 255).any())
    want = host_collate(items)
    dsc = DeviceScenes(ds.paths, ds.length, ds.voxel_scale, ds.seed, 3, 0, 1, dev(), augment=False, shuffle=False)
    got = dsc._batch([0, 1, 2])
    assert set(got) == set(want)
    for key in ("locs32", "locs_float", "labels32", "offsets"):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key].cpu(), want[key]), key
    assert np.array_equal(got["spatial_shape"], want["spatial_shape"]) and got["id"] == want["id"] == [0, 1, 2]
    assert [b["id"] for b in dsc] == [[0, 1, 2]]      # an epoch is one pass over the files


# ------------------------------------------------------------------------------------------------ 3D-FRONT: the narrow sample
def test_front3d_narrow_training_scene_is_drawn_again(native_lib, tmp_path):
    from doda_amd import aug
    from doda_amd.loader import DeviceScenes, dataset_for
    wide, narrow = (4.0, 4.0, 6.0), (4.0, 4.0, 1.0)      # z spans about 100 and 17 voxels; the z-rotation leaves it alone
    root, lines = dc.front3d_dataset(tmp_path / "front", stretch={"house_b/room_1.npy": wide, "house_a/room_2.npy": narrow, "house_a/room_0.npy": wide})
    cfg = dc.experiment(dc.front3d_cfg(root), n_classes=71)
    ds = dataset_for(cfg, dc.arguments(tmp_path / "cache"), "train")
    spans = [(xyz.max(0) - xyz.min(0)) * 50 for xyz, _ in dc.pool(ds.paths)]
    assert [bool((s // 64).min() >= 1) for s in spans] == [True, False, True] and ds.min_extent == 64
    dsc = DeviceScenes(ds.paths, ds.length, ds.voxel_scale, ds.seed, 2, 0, 1, dev(), augment=True, min_extent=ds.min_extent)
    seen = []
    for ids in ([1, 0], [2, 1], [4, 3], [1, 1]):
        batch = dsc._batch(ids)
        base = [(i % ds.length) % len(ds.paths) for i in batch["id"]]
        assert 1 not in base and len(base) == 2
        for b in range(2):
            q = batch["locs32"][int(batch["offsets"][b]):int(batch["offsets"][b + 1]), 1:]
            assert int((q.amax(0) // 64).min()) >= 1
        seen += base
    assert set(seen) == {0, 2}
    for epoch in range(3):
        dsc.set_epoch(epoch)
        for batch in dsc:
            assert 1 not in [(i % ds.length) % len(ds.paths) for i in batch["id"]]
    # the rule is the training split's: the same pool unaugmented keeps the narrow scene
    plain = DeviceScenes(ds.paths, ds.length, ds.voxel_scale, ds.seed, 3, 0, 1, dev(), augment=False, shuffle=False, min_extent=ds.min_extent)
    assert plain._batch([0, 1, 2])["id"] == [0, 1, 2]
    # a pool of narrow scenes only: the existing error after MAX_REDRAWS
    only = DeviceScenes([ds.paths[1]], 1, ds.voxel_scale, ds.seed, 1, 0, 1, dev(), augment=True, min_extent=64)
    with pytest.raises(RuntimeError, match="after %d redraws" % aug.MAX_REDRAWS):
        only._batch([0])


# ------------------------------------------------------------------------------------------------ the entry points
def _run(args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """ScanNet-format source (4 training scenes) and S3DIS-format target (3 training rooms, 2 in the test area) -> (tmp, the --set
    list that points the package's configs at them, scannet files, s3dis files)."""
    dev()
    tmp = tmp_path_factory.mktemp("files")
    scannet, s3dis = dc.scannet_dataset(tmp / "scannet"), dc.s3dis_dataset(tmp / "s3dis")
    sets = ["--set", "DATA_CONFIG.DATA_ROOT", str(tmp / "scannet"), "DATA_CONFIG.CLASS_MAPPER_FILE", dc.SCANNET_2_S3DIS,
            "DATA_CONFIG_TAR.DATA_ROOT", str(tmp / "s3dis"), "DATA_CONFIG_TAR.CLASS_MAPPER_FILE", dc.S3DIS_2_SCANNET]
    return tmp, sets, scannet, s3dis


def _common(tmp):
    return ["--output_root", str(tmp), "--scene_cache", str(tmp / "pool"), "--manual_seed", "3", "--batch_size", "2", "--print_freq", "1"]


@pytest.fixture(scope="module")
def stage1(data):
    """`python -m doda_amd.train` for one epoch (two iterations) of da_scannet_s3dis.yaml -> (its output, the checkpoint)."""
    tmp, sets, _, _ = data
    out = _run(["-m", "doda_amd.train", "--cfg_file", "doda_amd/cfgs/files/da_scannet_s3dis.yaml", "--epochs", "1"] + _common(tmp) + sets)
    return out, tmp / "cfgs" / "files" / "da_scannet_s3dis" / "default" / "ckpt" / "train_epoch_1.pth"


def test_train_on_scannet_format_files(native_lib, data, stage1):
    out, ckpt = stage1
    assert ckpt.exists()
    state = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    assert state["linear.weight"].shape[0] == 8 and state["linear.bias"].shape == (8,)
    losses = [float(v) for v in re.findall(r"Epoch: \[1/1\]\[\d/2\] Batch \S+ s Loss (\S+) Accuracy", out)]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), out[-2000:]
    m = re.search(r"Dataset scannet, split train \(training\) under (\S+): 4 scenes, (\d+) points, (\d+) bytes in HBM", out)
    assert m and m.group(1) == str(data[0] / "scannet"), out[-2000:]
    points = sum(dc.ref_scannet(f, "train")[0].shape[0] for f in data[2]["train"])
    assert int(m.group(2)) == points and int(m.group(3)) == 16 * points and "--synthetic_* flags are ignored" in out


def test_st_on_an_s3dis_format_target(native_lib, data, stage1):
    """ScanNet-format source, S3DIS-format target with downsampling_scale 4 and no_downsample_infer: pseudo labels for every point
    of the full clouds under the rooms' names, target batches of int(n / 4) points per room, cuboid mixing on."""
    from doda_amd import pseudo_labels as pl
    from doda_amd import st
    tmp, sets, _, s3dis = data
    argv = (["--cfg_file", "doda_amd/cfgs/files/da_scannet_s3dis_st.yaml", "--weight", str(stage1[1]), "--epochs", "1",
             "--preserve_pseudo_labels"] + _common(tmp) + sets)
    out = _run(["-m", "doda_amd.st"] + argv)
    args, cfg = st.parse_config(argv)
    assert cfg.DATA_CONFIG_TAR.DATA_PROCESSOR.downsampling_scale == 4 and cfg.DATA_CONFIG_TAR.DATA_PROCESSOR.no_downsample_infer is True
    assert cfg.DATA_CONFIG_TAR.DATA_AUG.tacm.enabled is True
    _, _, ckpt_dir, pdir = st.run_dirs(args, cfg)
    assert "pseudo labels: generated" in out and (ckpt_dir / "train_epoch_1.pth").exists()
    rooms = dc.ref_s3dis_list(tmp / "s3dis", "training", 5)
    assert len(rooms) == 3
    assert sorted(os.listdir(pl.txt_dir(pdir))) == sorted(r + ".txt" for r in rooms)
    n_full = [np.load(s3dis[r]).shape[0] for r in rooms]
    for r, n in zip(rooms, n_full):
        with open(os.path.join(pl.txt_dir(pdir), r + ".txt")) as f:
            assert len(f.read().split()) == n
    assert re.search(r"Dataset s3dis, split target \(training\) .*: 3 scenes, %d points" % sum(n_full), out)
    assert "split sampler: tail classes" in out                                  # the mixing is on
    lines = re.findall(r"Subsampled batch: source (\d+) points, target (\d+) points", out)
    assert len(lines) == 2 and all(int(t) > 0 for _, t in lines)                 # 4 source scenes, 2 per batch: two mixed steps
    n_val = [np.load(s3dis[r]).shape[0] for r in dc.ref_s3dis_list(tmp / "s3dis", "validation", 5)]
    m = re.search(r"Val full clouds: (\d+) points scored through (\d+) processed points", out)
    assert m and int(m.group(1)) == sum(n_val) and int(m.group(2)) == sum(int(n / 4) for n in n_val)


def test_evaluation_on_the_s3dis_format_test_area(native_lib, data, stage1):
    from doda_amd import test as dt
    tmp, sets, _, s3dis = data
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        res = dt.main(["--cfg_file", "doda_amd/cfgs/files/da_scannet_s3dis_eval.yaml", "--ckpt", str(stage1[1]), "--output_root", str(tmp),
                       "--scene_cache", str(tmp / "pool"), "--batch_size", "2", "--save_to_file"] + sets)
    finally:
        os.chdir(cwd)
    out = tmp / "cfgs" / "files" / "da_scannet_s3dis_eval" / "default" / "eval" / "epoch_1" / "validation" / "default"
    assert json.loads((out / "result.json").read_text()) == json.loads(json.dumps(res))
    rooms = dc.ref_s3dis_list(tmp / "s3dis", "validation", 5)
    mapper = dc.ref_mapper(dc.S3DIS_2_SCANNET)
    labels = [dc.ref_rows(s3dis[r], mapper)[1] for r in rooms]
    assert len(res["target"]) == 8 and sum(res["target"]) == sum(int((l != 255).sum()) for l in labels) > 0
    assert res["target"] == [int(sum((l == c).sum() for l in labels)) for c in range(8)]
    assert res["class_names"] == ["wall", "floor", "chair", "sofa", "table", "door", "window", "bookshelf"]
    assert sorted(os.listdir(out / "validation_0" / "txt")) == sorted(r + ".txt" for r in rooms)
    for r, l in zip(rooms, labels):
        written = np.loadtxt(out / "validation_0" / "txt" / (r + ".txt"), dtype=np.int64)
        assert written.shape == l.shape and written.min() >= 0 and written.max() < 8
    log = next(out.glob("log_eval_*.txt")).read_text()
    assert "Dataset s3dis, split test (test)" in log and "Val result: mIoU/mAcc/allAcc" in log

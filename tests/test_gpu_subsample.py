"""The training subsample on the MI355X: doda_subsample_draw (include/doda_subsample.h) against the numpy restatement
(tests/subsample_cases.py) — exact equality of the kept indices, of the bit patterns of the kept rows and of the labels —, its
argument checks and memory safety, the resident loaders with a downsampling_scale, and `python -m doda_amd.st` on an S3DIS-shaped
target (spconv_st_ds.yaml) end to end."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import subsample_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
SENTINEL = -77


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _raw_draw(lib, c, pad=64, **override):
    """doda_subsample_draw itself on case c, the outputs `pad` rows too long and filled with SENTINEL.
    -> (status, out_xyz int32 view [K + pad, 3], out_labels, out_idx, K)."""
    xyz, lab, offsets = sc.inputs(c)
    d = dev()
    n_seg, total = len(c["sizes"]), sum(c["ks"])
    tx, tl = torch.from_numpy(xyz).to(d), torch.from_numpy(lab).to(d)
    ox = torch.full((total + pad, 3), SENTINEL, dtype=torch.int32, device=d)
    ol = torch.full((total + pad,), SENTINEL, dtype=torch.int32, device=d)
    oi = torch.full((total + pad,), SENTINEL, dtype=torch.int32, device=d)
    off_h = (C.c_int64 * (n_seg + 1))(*offsets)
    nbytes = max(int(lib.doda_subsample_workspace_bytes(off_h, n_seg)), 1 << 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    a = dict(xyz=tx.data_ptr(), labels=tl.data_ptr(), ei=None, eu=None, off=off_h, n=n_seg, k=(C.c_int32 * n_seg)(*c["ks"]),
             seeds=(C.c_uint64 * n_seg)(*c["seeds"]), mask=c["key_mask"], oxyz=ox.data_ptr(), olab=ol.data_ptr(), oidx=oi.data_ptr(),
             oei=None, oeu=None, ws=ws.data_ptr(), wsb=nbytes, stream=None)
    a.update(override)
    status = lib.doda_subsample_draw(*a.values())
    torch.cuda.synchronize()
    return status, ox.cpu().numpy(), ol.cpu().numpy(), oi.cpu().numpy(), total


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_restatement(native_lib, name):
    from doda_amd import ops
    c = CASES[name]
    xyz, lab, offsets = sc.inputs(c)
    sub, rows, offsets_s = sc.expected(c)
    d = dev()
    x, l, s, o = ops.subsample(torch.from_numpy(xyz).to(d), torch.from_numpy(lab).to(d), offsets, c["ks"], c["seeds"], key_mask=c["key_mask"])
    assert o == offsets_s and x.is_cuda and s.dtype == torch.int32
    assert torch.equal(s.cpu(), torch.from_numpy(sub))
    assert torch.equal(x.cpu().view(torch.int32), torch.from_numpy(xyz[rows].view(np.int32)))
    assert torch.equal(l.cpu(), torch.from_numpy(lab[rows]))
    if name == "ties_mask_0":
        assert torch.equal(s.cpu(), torch.arange(1250, dtype=torch.int32))
    # the torch route on the device: the same bits
    x2, l2, s2, o2 = ops.subsample_torch(torch.from_numpy(xyz).to(d), torch.from_numpy(lab).to(d), offsets, c["ks"], c["seeds"], c["key_mask"])
    assert o2 == o and torch.equal(s2, s) and torch.equal(l2, l) and torch.equal(x2.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("name", ["four_segments", "ties_two_segments", "n1025_ds3", "k_n_minus_1"])
def test_no_row_past_the_kept_count_is_written_and_a_second_call_is_bit_equal(native_lib, name):
    c = CASES[name]
    xyz, lab, _ = sc.inputs(c)
    sub, rows, _ = sc.expected(c)
    st, ox, ol, oi, total = _raw_draw(native_lib, c)
    assert st == 0
    assert np.array_equal(oi[:total], sub) and np.array_equal(ol[:total], lab[rows]) and np.array_equal(ox[:total], xyz[rows].view(np.int32))
    assert (ox[total:] == SENTINEL).all() and (ol[total:] == SENTINEL).all() and (oi[total:] == SENTINEL).all()
    st2, ox2, ol2, oi2, _ = _raw_draw(native_lib, c)
    assert st2 == 0 and np.array_equal(ox, ox2) and np.array_equal(ol, ol2) and np.array_equal(oi, oi2)


def test_argument_errors_leave_the_outputs_untouched(native_lib):
    lib = native_lib
    c = CASES["four_segments"]
    off = lambda *v: (C.c_int64 * len(v))(*v)
    bad = [(dict(off=off(0, 5000, 4999, 5001, 8334)), -1),                                   # decreasing offsets
           (dict(k=(C.c_int32 * 4)(1250, 2, 0, 833)), -1),                                   # k > n
           (dict(off=off(*range(0, 66 * 100, 100)), n=65, k=(C.c_int32 * 65)(*[1] * 65), seeds=(C.c_uint64 * 65)(*range(65))), -4),
           (dict(labels=None), -1), (dict(oidx=None), -1), (dict(ws=None), -1), (dict(wsb=64), -5)]
    for override, want in bad:
        st, ox, ol, oi, _ = _raw_draw(lib, c, **override)
        assert st == want, (override.keys(), st)
        if "oidx" not in override:
            assert (oi == SENTINEL).all()
        assert (ox == SENTINEL).all() and (ol == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the loaders
@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    from doda_amd.loader import prepare_cache
    root = tmp_path_factory.mktemp("sub_scenes")
    _, tar = prepare_cache(2, 4000, 50, 501000, str(root), procs=1)
    _, src = prepare_cache(2, 4000, 50, 1000, str(root), procs=1)
    return tar, src


def test_device_scenes_with_a_downsampling_scale(native_lib, scenes):
    from doda_amd.loader import DeviceScenes
    tar, _ = scenes
    d = dev()
    assert DeviceScenes.SUBSAMPLE_NATIVE in (True, False)
    dsc = DeviceScenes(tar, 2, 50, 7, 2, 0, 1, d, downsampling_scale=4)
    full = [np.load(p) for p in tar]
    n_all = [f["labels"].shape[0] for f in full]
    want = [0, int(n_all[0] / 4), int(n_all[0] / 4) + int(n_all[1] / 4)]
    batch = dsc._batch([0, 1])
    assert batch["offsets"].tolist() == want and batch["locs32"].shape[0] == want[-1] and "offsets_all" not in batch
    x, lab, offsets = dsc._concat([0, 1])
    assert offsets == want
    subs = []
    for b, i in enumerate([0, 1]):
        sub = sc.select((7 * 1000003 + 19 * i + 11) & 0x7fffffffffffffff, n_all[b], int(n_all[b] / 4))
        subs.append(sub)
        assert torch.equal(x[offsets[b]:offsets[b + 1]].cpu(), torch.from_numpy(full[b]["xyz_mid"].astype(np.float32)[sub]))
        assert torch.equal(lab[offsets[b]:offsets[b + 1]].cpu(), torch.from_numpy(full[b]["labels"].astype(np.int32)[sub]))
    new = [torch.from_numpy(np.arange(n, dtype=np.int32) % 13) for n in n_all]
    dsc.set_labels(new)
    lab2 = dsc._concat([0, 1])[1].cpu()
    assert torch.equal(lab2, torch.cat([new[b][torch.from_numpy(subs[b])] for b in range(2)]))
    # a scale of 1: the batches of a loader that never heard of the key, bit for bit
    one, plain = DeviceScenes(tar, 2, 50, 7, 2, 0, 1, d, downsampling_scale=1)._batch([0, 1]), DeviceScenes(tar, 2, 50, 7, 2, 0, 1, d)._batch([0, 1])
    assert set(one) == set(plain) and all(torch.equal(one[k], plain[k]) for k in ("locs32", "locs_float", "labels32", "offsets"))
    assert plain["offsets"].tolist() == [0, n_all[0], sum(n_all)]
    # the validation split: EvalScenes' subsample and the full clouds, on the device
    val = DeviceScenes(tar, 2, 50, 7, 2, 0, 1, d, augment=False, shuffle=False, downsampling_scale=4, subsample_seed=3)._batch([0, 1])
    assert val["offsets"].tolist() == want and val["offsets_all"].tolist() == [0, n_all[0], sum(n_all)] and val["locs_float_all"].is_cuda


def test_mixed_device_scenes_mix_the_subsampled_target(native_lib, scenes):
    from doda_amd import tacm as tacm_mod
    from doda_amd.loader import MixedDeviceScenes
    from tests import tacm_cases as tc
    tar, src = scenes
    tacm = tacm_mod.TacmConfig(enabled=True, split=[2, 2, 1], p=0.5, mix_ratio=0.5, permute_p=0.5, queue_enabled=True, queue_size=16,
                               num_cuboid=2.0, num_class=2, n_classes=20)
    sampler = tacm_mod.SplitSampler(tacm)
    sampler.init_class_ratio(tc.class_ratio_of(np.concatenate([np.load(p)["labels"] for p in tar]).astype(np.int64)))
    sampler.update_cfg(tacm)
    n_tar = [np.load(p)["labels"].shape[0] for p in tar]
    n_src = [np.load(p)["labels"].shape[0] for p in src]
    mixed = MixedDeviceScenes(tar, src, 2, 50, 7, 2, 0, 1, dev(), tacm, sampler, downsampling_scale=4, source_downsampling_scale=1)
    tm, tl, toff, _ = mixed._rigid([0, 1])
    assert toff == [0, int(n_tar[0] / 4), int(n_tar[0] / 4) + int(n_tar[1] / 4)] and tm.shape[0] == toff[-1] == tl.shape[0]
    sm, _, soff, _ = mixed.source._rigid([0, 1])
    assert soff == [0, n_src[0], sum(n_src)]
    batch = mixed._batch([0, 1])
    assert batch["mask1"].numel() == int(batch["offsets"][-1]) == batch["mask2"].numel() == batch["locs32"].shape[0]
    assert int(batch["mask1"].sum()) <= toff[-1]      # (points of the target scenes: at most the subsampled count)
    both = MixedDeviceScenes(tar, src, 2, 50, 7, 2, 0, 1, dev(), tacm, sampler, downsampling_scale=4, source_downsampling_scale=2)
    assert both.source._rigid([0, 1])[2] == [0, int(n_src[0] / 2), int(n_src[0] / 2) + int(n_src[1] / 2)]


# ------------------------------------------------------------------------------------------------ end to end
SYN = ["--synthetic_scenes", "4", "--synthetic_base", "4", "--synthetic_voxels", "5000", "--batch_size", "2", "--print_freq", "1"]


def _run(args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


def test_st_end_to_end_on_a_subsampled_target(native_lib, tmp_path):
    """One epoch of stage 1, then `python -m doda_amd.st` with spconv_st_ds.yaml: pseudo labels for every point of the full clouds,
    target batches of int(n / 4) points per scene, validation through the full clouds."""
    from doda_amd import pseudo_labels as pl
    from doda_amd import st
    from doda_amd.loader import prepare_cache
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    tmp, cache = tmp_path, str(tmp_path / "scenes")
    _run(["-m", "doda_amd.train", "--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml", "--epochs", "1", "--output_root", str(tmp),
          "--scene_cache", cache, "--manual_seed", "3"] + SYN + ["--set", "MODEL.dsnorm", "True"])
    ckpt = tmp / "cfgs" / "synthetic" / "spconv" / "default" / "ckpt" / "train_epoch_1.pth"
    assert ckpt.exists()
    argv = (["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_ds.yaml", "--weight", str(ckpt), "--epochs", "1", "--output_root", str(tmp),
             "--scene_cache", cache, "--st_extra_tag", "ds", "--manual_seed", "3", "--preserve_pseudo_labels"] + SYN)
    out = _run(["-m", "doda_amd.st"] + argv)
    args, cfg = st.parse_config(argv)
    _, _, ckpt_dir, pdir = st.run_dirs(args, cfg)
    assert "pseudo labels: generated" in out and (ckpt_dir / "train_epoch_1.pth").exists()
    _, tar = prepare_cache(4, 5000, 50, 501000, cache)
    _, src = prepare_cache(4, 5000, 50, 1000, cache)
    _, val = prepare_cache(4, 5000, 50, 901000, cache)
    n_tar = [np.load(p)["labels"].shape[0] for p in tar]
    got = pl.read_scene_labels(pdir, tar)
    assert [g.shape[0] for g in got] == n_tar                                   # one line per full-cloud point
    lines = re.findall(r"Subsampled batch: source (\d+) points, target (\d+) points", out)
    assert len(lines) == 2                                                      # 4 scenes per epoch, 2 per batch
    # every base scene once per epoch: the target batches hold int(n / 4) points of each, the source batches every point
    assert sum(int(t) for _, t in lines) == sum(int(n / 4) for n in n_tar)
    assert sum(int(s) for s, _ in lines) == sum(np.load(p)["labels"].shape[0] for p in src)
    n_val = [np.load(p)["labels"].shape[0] for p in val]
    m = re.search(r"Val full clouds: (\d+) points scored through (\d+) processed points", out)
    assert m and int(m.group(1)) == sum(n_val) and int(m.group(2)) == sum(int(n / 4) for n in n_val)
    assert re.search(r"Val result: mIoU/mAcc/allAcc", out)

"""The training subsample under DATA_PROCESSOR.downsampling_scale, host side (no GPU): the companion C ABI include/doda_subsample.h,
the torch fallback of ops.subsample against the numpy restatement (tests/subsample_cases.py), the distribution of the draw, the
configuration per split, the rejections, and the resident loader on the CPU."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import subsample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()


def test_subsample_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses before anything is launched; nothing to keep is nothing to do."""
    lib = native_lib
    off = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    assert lib.doda_subsample_workspace_bytes(off(0, 1024, 1025, 1025), 3) == 4 * (4 * 3 * 256 + 2 * 3 + 2 * 2)
    assert lib.doda_subsample_workspace_bytes(off(1, 5), 1) == 0 and lib.doda_subsample_workspace_bytes(off(0, 5, 4), 2) == 0
    assert lib.doda_subsample_workspace_bytes(off(0, 1 << 31), 1) == 0

    def draw(**kw):
        d = dict(xyz=4, labels=4, ei=None, eu=None, off=off(0, 5), n=1, k=i32(2), seeds=u64(1), mask=0xffffffff, oxyz=4, olab=4, oidx=4,
                 oei=None, oeu=None, ws=4, wsb=1 << 20, stream=None)
        d.update(kw)
        return lib.doda_subsample_draw(*d.values())
    assert draw(off=off(0, 5, 4), n=2, k=i32(1, 1), seeds=u64(1, 2)) == -1                      # decreasing offsets
    assert draw(off=off(1, 5)) == -1 and draw(off=off(0, 1 << 31)) == -1
    assert draw(off=off(*range(66)), n=65, k=i32(*[1] * 65), seeds=u64(*range(65))) == -4       # more segments than a launch carries
    assert draw(k=i32(6)) == -1 and draw(k=i32(-1)) == -1                                       # k outside [0, n]
    assert draw(k=None) == -1 and draw(seeds=None) == -1
    for name in ("xyz", "labels", "oxyz", "olab", "oidx", "ws"):
        assert draw(**{name: None}) == -1, name
    assert draw(ei=4) == -1 and draw(oeu=4) == -1                                               # a column without its output
    assert draw(ws=6) == -1                                                                     # misaligned workspace
    assert draw(wsb=16) == -5
    assert draw(k=i32(0), xyz=None, labels=None, oxyz=None, olab=None, oidx=None, ws=None, wsb=0) == 0
    assert draw(off=off(0, 0), k=i32(0), xyz=None, ws=None) == 0


def test_restatement_is_philox_4x32_10():
    """Random123's known answers for Philox-4x32-10 (kat_vectors), and the key of a point is output word 0 of counter (j, 0, 0, 0)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd))]
    for ctr, key, want in kat:
        got = sc.philox4x32_10([np.array([v], dtype=np.uint64) for v in ctr], key)
        assert tuple(int(g[0]) for g in got) == want
    assert int(sc.keys(0, 1)[0]) == 0x6627e8d5
    seed = 0x299f31d0a4093822
    one = sc.philox4x32_10([np.array([v], dtype=np.uint64) for v in (5, 0, 0, 0)], (seed & 0xffffffff, seed >> 32))[0]
    assert int(sc.keys(seed, 6)[5]) == int(one[0]) and int(sc.keys(seed, 6, 0xF)[5]) == int(one[0]) & 0xF


def test_torch_keys_equal_the_restatement():
    from doda_amd import ops
    for seed in (0, 1, 0xffffffffffffffff, 0x299f31d0a4093822):
        got = ops.subsample_keys(seed, 3000, "cpu").numpy()
        assert np.array_equal(got, sc.keys(seed, 3000).astype(np.int64))
    assert np.array_equal(ops.subsample_keys(7, 100, "cpu", 0x3).numpy(), sc.keys(7, 100, 0x3).astype(np.int64))


@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_fallback_equals_the_restatement(name):
    from doda_amd import ops
    c = CASES[name]
    xyz, lab, offsets = sc.inputs(c)
    sub, rows, offsets_s = sc.expected(c)
    x, l, s, o = ops.subsample(torch.from_numpy(xyz), torch.from_numpy(lab), offsets, c["ks"], c["seeds"], key_mask=c["key_mask"])
    assert o == offsets_s and s.dtype == torch.int32 and l.dtype == torch.int32 and x.dtype == torch.float32
    assert np.array_equal(s.numpy(), sub) and np.array_equal(l.numpy(), lab[rows])
    assert np.array_equal(x.numpy().view(np.uint32), xyz[rows].view(np.uint32))
    if name == "ties_mask_0":
        assert np.array_equal(sub, np.arange(1250))


@pytest.mark.parametrize("ds", [1, 3, 4, 2.5])
def test_count_order_and_seeds(ds):
    from doda_amd import ops
    from doda_amd.loader import subsample_count
    n = 1003
    k = subsample_count(n, ds)
    assert k == int(n / ds) == sc.count(n, ds)
    xyz, lab = sc.scene(n, 3)
    run = lambda seed: ops.subsample(torch.from_numpy(xyz), torch.from_numpy(lab), [0, n], [k], [seed])[2].numpy()
    a = run(11)
    assert a.shape == (k,) and np.all(np.diff(a) > 0) and a.min() >= 0 and a.max() < n
    assert np.array_equal(a, run(11)) and np.array_equal(a, sc.select(11, n, k))
    assert ds == 1 or not np.array_equal(a, run(12))


def test_every_point_is_kept_equally_often():
    """n = 64, k = 16, seeds 0 .. 1999: a point's count is Binomial(2000, 1/4), mean 500, standard deviation 19.4; five of them."""
    hits = np.zeros(64, dtype=np.int64)
    for seed in range(2000):
        hits[sc.select(seed, 64, 16)] += 1
    print("inclusion counts: min %d max %d" % (hits.min(), hits.max()))
    assert hits.sum() == 2000 * 16 and hits.min() >= 403 and hits.max() <= 597


# ------------------------------------------------------------------------------------------------ configuration
def _cfg(name):
    from doda_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", "synthetic", name))


def test_st_ds_config_parses_and_the_scale_is_read_per_split():
    from doda_amd import st, train
    cfg, base = _cfg("spconv_st_ds.yaml"), _cfg("spconv_st.yaml")
    dp = cfg.DATA_CONFIG_TAR.DATA_PROCESSOR
    assert dp.downsampling_scale == 4 and dp.no_downsample_infer is True and dp.voxel_scale == 50
    assert "downsampling_scale" not in cfg.DATA_CONFIG.DATA_PROCESSOR
    assert cfg.MODEL == base.MODEL and cfg.DATA_CONFIG == base.DATA_CONFIG and cfg.SELF_TRAIN == base.SELF_TRAIN
    assert cfg.OPTIMIZATION == base.OPTIMIZATION
    assert [train.downsampling_scale_of(cfg, s) for s in ("train", "target", "val")] == [1, 4, 4]
    assert [train.downsampling_scale_of(base, s) for s in ("train", "target", "val")] == [1, 1, 1]
    cfg.DATA_CONFIG.DATA_PROCESSOR.downsampling_scale = 2.5
    assert train.downsampling_scale_of(cfg, "train") == 2.5 and train.downsampling_scale_of(cfg, "target") == 4
    del cfg["DATA_CONFIG_TAR"]
    assert [train.downsampling_scale_of(cfg, s) for s in ("train", "target", "val")] == [2.5, 2.5, 2.5]
    args, parsed = st.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_ds.yaml"])
    assert args.self_train and parsed.DATA_CONFIG_TAR.DATA_PROCESSOR.downsampling_scale == 4
    st.check_pseudo_label_clouds(parsed)
    train.check_subsample_loader(parsed, args)


def test_the_three_rejections(tmp_path):
    from doda_amd import st, train
    from doda_amd.loader import DeviceScenes, prepare_cache
    cfg = _cfg("spconv_st_ds.yaml")
    # the worker loaders with a training scale above 1
    for flags in ({"host_loader": True, "inline_loader": False}, {"host_loader": False, "inline_loader": True}):
        with pytest.raises(ValueError, match="downsampling_scale"):
            train.check_subsample_loader(cfg, argparse.Namespace(self_train=True, **flags))
        train.check_subsample_loader(_cfg("spconv_st.yaml"), argparse.Namespace(self_train=True, **flags))
    train.check_subsample_loader(cfg, argparse.Namespace(self_train=True, host_loader=False, inline_loader=False))
    # pseudo labels of subsample length
    for value in (False, None):
        bad = _cfg("spconv_st_ds.yaml")
        if value is None:
            del bad.DATA_CONFIG_TAR.DATA_PROCESSOR["no_downsample_infer"]
        else:
            bad.DATA_CONFIG_TAR.DATA_PROCESSOR.no_downsample_infer = value
        with pytest.raises(ValueError, match="no_downsample_infer"):
            st.check_pseudo_label_clouds(bad)
    st.check_pseudo_label_clouds(_cfg("spconv_st.yaml"))
    with pytest.raises(ValueError, match="no_downsample_infer"):      # (before any work: no GPU, no checkpoint, no directory)
        st.main(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_ds.yaml", "--output_root", str(tmp_path / "out"), "--set",
                 "DATA_CONFIG_TAR.DATA_PROCESSOR.no_downsample_infer", "False"])
    assert not (tmp_path / "out").exists()
    # a scene the scale leaves without a point
    _, paths = prepare_cache(1, 300, 50, 901000, str(tmp_path / "scenes"), procs=1)
    n = np.load(paths[0])["labels"].shape[0]
    with pytest.raises(ValueError, match=re.escape(os.path.basename(paths[0]))):
        DeviceScenes(paths, 1, 50, 0, 1, 0, 1, "cpu", downsampling_scale=n + 1)
    DeviceScenes(paths, 1, 50, 0, 1, 0, 1, "cpu", downsampling_scale=n)


# ------------------------------------------------------------------------------------------------ the resident loader on the CPU
@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    from doda_amd.loader import prepare_cache
    _, paths = prepare_cache(2, 2000, 50, 901000, str(tmp_path_factory.mktemp("sub_scenes")), procs=1)
    return paths


def test_validation_split_carries_the_full_clouds_and_evalscenes_subsample(scenes):
    from doda_amd.evaluate import has_full_cloud
    from doda_amd.loader import DeviceScenes, EvalScenes
    dsc = DeviceScenes(scenes, 2, 50, 901000, 2, 0, 1, "cpu", augment=False, shuffle=False, downsampling_scale=4, subsample_seed=5)
    batch = next(iter(dsc))
    src = EvalScenes(scenes, 50, 4, seed=5)
    full = [np.load(p) for p in scenes]
    subs = [src.subsample(k) for k in range(2)]
    n_all = [f["labels"].shape[0] for f in full]
    assert {"locs_float_all", "labels_all", "offsets_all"} <= set(batch) and has_full_cloud(batch)
    assert batch["offsets"].tolist() == [0, int(n_all[0] / 4), int(n_all[0] / 4) + int(n_all[1] / 4)]
    assert batch["offsets_all"].dtype == torch.int32 and batch["offsets_all"].tolist() == [0, n_all[0], sum(n_all)]
    assert batch["labels_all"].dtype == torch.int64 and batch["locs_float_all"].dtype == torch.float32
    assert np.array_equal(batch["locs_float_all"].numpy(), np.concatenate([f["xyz_mid"] for f in full]).astype(np.float32))
    assert np.array_equal(batch["labels_all"].numpy(), np.concatenate([f["labels"] for f in full]))
    assert np.array_equal(batch["locs_float"].numpy(), np.concatenate([f["xyz_mid"][s] for f, s in zip(full, subs)]).astype(np.float32))
    assert np.array_equal(batch["labels32"].numpy(), np.concatenate([f["labels"][s] for f, s in zip(full, subs)]))
    items = [src[0], src[1]]      # the same voxel coordinates as the evaluation entry point's items
    assert torch.equal(batch["locs32"][:, 1:], torch.cat([it[0] for it in items]))
    plain = next(iter(DeviceScenes(scenes, 2, 50, 901000, 2, 0, 1, "cpu", augment=False, shuffle=False)))
    assert "offsets_all" not in plain and torch.equal(plain["locs_float"], batch["locs_float_all"])
    # the concat collate hands the three keys on (what the trainer's feeder runs)
    from doda_amd.collate import collate_device_concat
    out = collate_device_concat(batch, "cpu")
    assert has_full_cloud(out) and out["labels_all"].dtype == torch.int64 and torch.equal(out["locs_float_all"], batch["locs_float_all"])
    assert "offsets_all" not in collate_device_concat(plain, "cpu")


def test_training_split_on_the_cpu_subsamples_before_the_augmentation(scenes):
    from doda_amd.loader import DeviceScenes
    dsc = DeviceScenes(scenes, 2, 50, 7, 2, 0, 1, "cpu", downsampling_scale=4)
    full = [np.load(p) for p in scenes]
    n_all = [f["labels"].shape[0] for f in full]
    ids = [0, 1]
    x, lab, offsets = dsc._concat(ids)
    assert offsets == [0, int(n_all[0] / 4), int(n_all[0] / 4) + int(n_all[1] / 4)] and x.shape[0] == offsets[-1]
    for b, i in enumerate(ids):
        seed = (7 * 1000003 + 19 * i + 11) & 0x7fffffffffffffff
        sub = sc.select(seed, n_all[b], int(n_all[b] / 4))
        assert np.array_equal(x[offsets[b]:offsets[b + 1]].numpy(), full[b]["xyz_mid"].astype(np.float32)[sub])
        assert np.array_equal(lab[offsets[b]:offsets[b + 1]].numpy(), full[b]["labels"][sub])
    x2, _, _ = dsc._concat([2, 3])      # (the same base scenes as other items: another draw)
    assert not torch.equal(x, x2)
    batch = dsc._batch(ids)
    assert batch["offsets"].tolist() == offsets and "offsets_all" not in batch
    new = [torch.full((n,), 7, dtype=torch.int32) for n in n_all]
    dsc.set_labels(new)
    assert torch.equal(dsc._concat(ids)[1], torch.full((offsets[-1],), 7, dtype=torch.int32))
    same = DeviceScenes(scenes, 2, 50, 7, 2, 0, 1, "cpu", downsampling_scale=1)._concat(ids)
    assert same[2] == [0, n_all[0], sum(n_all)] and np.array_equal(same[0].numpy(), np.concatenate([f["xyz_mid"] for f in full]).astype(np.float32))

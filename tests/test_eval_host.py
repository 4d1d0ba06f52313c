"""Full-cloud evaluation, host side (no GPU): the companion C ABI include/doda_eval.h, argument errors as statuses, the seeded
subsample and the collated `*_all` keys (reference dataset/dataset.py:74-77, dataset/s3dis.py:96-130), the sharding of scenes over
ranks and the `python -m doda_amd.test` command line (reference tool/test.py)."""
import numpy as np
import pytest
import torch

from tests import eval_cases as ec


def _scene(n_end, m_end, dims=(1, 1, 1), base=0, side=0.08):
    from doda_amd._lib import EvalScene
    s = EvalScene()
    s.n_end, s.m_end, s.cell_base = n_end, m_end, base
    for k in range(3):
        s.dims[k], s.origin[k] = dims[k], 0.0
    s.side, s.inv_side = side, (1.0 / side if side else 0.0)
    return s


def test_eval_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses before anything is launched: null pointers, negative and over-wide sizes, a scene with
    queries but no processed point, a grid outside the limits."""
    from doda_amd._lib import EvalScene
    lib = native_lib
    one = (EvalScene * 1)(_scene(10, 20))
    nn = lambda scenes, nb, n=10, m=20, p=1: lib.doda_eval_nn(p, p, n, p, scenes, nb, p, None, m, p, p, None)
    assert nn(one, 1, n=-1) == -1 and nn(one, 1, m=-1) == -1
    assert nn(one, 1, n=1 << 31) == -4 and nn(one, 1, m=1 << 31) == -4            # index arithmetic is int32
    assert nn(None, 1) == -1 and nn(one, 0) == -1
    assert nn((EvalScene * 33)(), 33) == -4                                        # more scenes than a launch carries
    assert nn(one, 1, p=None) == -1                                                # null device pointers
    assert nn(one, 1, n=11) == -1 and nn(one, 1, m=21) == -1                       # offsets that do not end at n / m
    empty = (EvalScene * 2)(_scene(0, 5), _scene(10, 20, base=1))
    assert nn(empty, 2) == -1                                                      # full points with nothing to be near to
    assert nn((EvalScene * 1)(_scene(10, 20, dims=(128, 128, 129))), 1) == -1      # above 2^21 cells
    assert nn((EvalScene * 1)(_scene(10, 20, dims=(0, 1, 1))), 1) == -1
    assert nn((EvalScene * 1)(_scene(10, 20, side=0.0)), 1) == -1
    assert nn((EvalScene * 1)(_scene(10, 0)), 1, m=0) == 0                         # no query: nothing to do
    sc = lambda feats=1, m_vox=5, c=16, esz=4, w=1, k=8, n=10, idx=1, m=20, hist=1, out=1, ws=1, nb=1: lib.doda_eval_score(
        feats, m_vox, c, esz, w, None, k, 1, n, idx, 1, m, 255, None, hist, out, ws, nb, None)
    assert sc(out=None) == -1 and sc(hist=None) == -1 and sc(w=None) == -1 and sc(feats=None) == -1 and sc(ws=None) == -1
    assert sc(n=-1) == -1 and sc(m=-1) == -1 and sc(m_vox=-1) == -1 and sc(esz=3) == -1
    assert sc(idx=None) == -1                                                      # identity needs m == n
    assert sc(m=1 << 31) == -4 and sc(c=24) == -4 and sc(k=33) == -4 and sc(k=1) == -4
    assert sc(nb=lib.doda_eval_score_blocks(20) + 1) == -5
    assert lib.doda_eval_score_blocks(20) == 1 and lib.doda_eval_score_blocks(1 << 30) == 2048


def test_brute_force_restatement_takes_the_lowest_index_on_ties():
    """The numpy restatement on case (ii): ties are everywhere and every answer is the lowest index among the nearest points."""
    xyz, ends, new, new_ends, _ = ec.case("ii")
    idx, d2 = ec.brute_force_nn(xyz, ends, new, new_ends)
    d = ((new[:500, None, :].astype(np.float64) - xyz[None].astype(np.float64)) ** 2).sum(2)
    tied = (d == d.min(1, keepdims=True))
    assert tied.sum(1).max() > 1 and np.array_equal(idx[:500], tied.argmax(1))
    assert np.array_equal(d2[:500].astype(np.float64), d.min(1))                  # lattice distances are exact in fp32
    # a scene without processed points keeps the start state; a query past 1e10 away does too
    i2, e2 = ec.brute_force_nn(np.zeros((1, 3), np.float32), [0, 1], np.array([[0, 0, 0], [2e5, 0, 0]], np.float32), [1, 2])
    assert i2.tolist() == [0, 0] and e2.tolist() == [1e10, 1e10]


# ------------------------------------------------------------------------------------------------ subsample, collate
@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    from doda_amd.loader import prepare_cache
    _, paths = prepare_cache(3, 3000, 50, 901000, str(tmp_path_factory.mktemp("eval_scenes")), procs=1)
    return paths


def test_subsample_is_sorted_sized_and_independent_of_batching(scenes):
    from doda_amd.loader import EvalScenes, SyntheticScenes, subsample_indices
    idx = subsample_indices(1003, 4, 7)
    assert idx.shape == (int(1003 / 4),) and np.all(np.diff(idx) > 0) and idx.min() >= 0 and idx.max() < 1003
    assert np.array_equal(idx, subsample_indices(1003, 4, 7)) and not np.array_equal(idx, subsample_indices(1003, 4, 8))
    src, again = EvalScenes(scenes, 50, 4, seed=5), EvalScenes(scenes[::-1], 50, 4, seed=5)
    full = SyntheticScenes(scenes, len(scenes), 50, 0, augment=False)
    for k in range(len(scenes)):
        sub = src.subsample(k)
        n = full[k][1].shape[0]
        assert sub.shape == (int(n / 4),) and np.all(np.diff(sub) > 0)
        assert np.array_equal(sub, again.subsample(len(scenes) - 1 - k))          # the scene decides, not its position
        xyz, mid, lab, ident, extra = src[k]
        assert torch.equal(mid, full[k][1][sub]) and torch.equal(lab, full[k][2][sub]) and ident == k
        assert torch.equal(extra["xyz_mid_all"], full[k][1]) and torch.equal(extra["labels_all"], full[k][2])
        assert xyz.dtype == torch.int32 and int(xyz.min()) == 0
    plain = EvalScenes(scenes, 50, 1)
    assert len(plain[0]) == 4 and all(torch.equal(a, b) for a, b in zip(plain[0][:3], full[0][:3]))


def test_collated_full_cloud_keys(scenes):
    """The reference's three extra keys with its dtypes and shapes; a batch without downsampling has exactly today's keys."""
    from doda_amd.collate import collate_device
    from doda_amd.loader import EvalScenes
    src = EvalScenes(scenes, 50, 4)
    batch = collate_device([src[0], src[2]], "cpu")
    plain = collate_device([EvalScenes(scenes, 50, 1)[0], EvalScenes(scenes, 50, None)[2]], "cpu")
    assert set(batch) - set(plain) == {"locs_float_all", "labels_all", "offsets_all"} and set(plain) <= set(batch)
    n_all = [src[k][4]["labels_all"].shape[0] for k in (0, 2)]
    assert batch["offsets_all"].dtype == torch.int32 and batch["offsets_all"].tolist() == [0, n_all[0], sum(n_all)]
    assert batch["locs_float_all"].dtype == torch.float32 and tuple(batch["locs_float_all"].shape) == (sum(n_all), 3)
    assert batch["labels_all"].dtype == torch.int64 and tuple(batch["labels_all"].shape) == (sum(n_all),)
    assert batch["offsets"].tolist() == [0, int(n_all[0] / 4), int(n_all[0] / 4) + int(n_all[1] / 4)]
    assert torch.equal(batch["labels_all"][:n_all[0]], src[0][4]["labels_all"].long())
    assert torch.equal(plain["locs_float"], batch["locs_float_all"]) and torch.equal(plain["labels"], batch["labels_all"])
    from doda_amd.evaluate import has_full_cloud
    assert has_full_cloud(batch) and not has_full_cloud(plain)
    with pytest.raises(ValueError):
        collate_device([src[0], EvalScenes(scenes, 50, 1)[1]], "cpu")


def test_eval_config_composes_spconv_with_downsampling():
    from doda_amd import test as dt
    args, cfg = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_eval_ds.yaml"])
    _, base = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml"])
    assert cfg.DATA_CONFIG_TAR.DATA_PROCESSOR.downsampling_scale == 4 and "downsampling_scale" not in cfg.DATA_CONFIG.DATA_PROCESSOR
    assert cfg.MODEL == base.MODEL and cfg.DATA_CONFIG == base.DATA_CONFIG and cfg.COMMON_CLASSES == base.COMMON_CLASSES
    assert dt.dataset_config(cfg) is cfg.DATA_CONFIG_TAR and dt.dataset_config(cfg, eval_src=True) is cfg.DATA_CONFIG
    del cfg["DATA_CONFIG_TAR"]
    assert dt.dataset_config(cfg) is cfg.DATA_CONFIG


# ------------------------------------------------------------------------------------------------ entry point
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("batch", [1, 2, 4])
def test_sharding_scores_every_scene_exactly_once(world, batch):
    from doda_amd.test import shard_batches
    seen = []
    for rank in range(world):
        groups = shard_batches(7, world, rank, batch)
        assert all(1 <= len(g) <= batch for g in groups) and all(len(g) == batch for g in groups[:-1])
        seen += [k for g in groups for k in g]
    assert sorted(seen) == list(range(7))


REFERENCE_TEST_FLAGS = [   # tool/test.py:35-64
    ("--cfg_file", "doda_amd/cfgs/synthetic/spconv_eval_ds.yaml"), ("--batch_size", "4"), ("--epochs", "3"), ("--workers", "2"),
    ("--extra_tag", "pre"), ("--start_epoch", "12"), ("--ckpt", "ckpt/train_epoch_12.pth"), ("--weight", "w.pth"), ("--launcher", "none"),
    ("--tcp_port", "18889"), ("--sync_bn", None), ("--manual_seed", "5"), ("--print_freq", "3"), ("--local_rank", "0"),
    ("--max_waiting_mins", "1"), ("--eval_tag", "tag"), ("--save_to_file", None), ("--save_logit", None), ("--save_feat", None),
    ("--pretrain_not_strict", None), ("--eval_src", None),
]


def test_command_line_accepts_every_reference_flag_and_names_the_output_directory(tmp_path):
    from doda_amd import test as dt
    argv = []
    for flag, val in REFERENCE_TEST_FLAGS:
        argv += [flag] + ([val] if val is not None else [])
    argv += ["--output_root", str(tmp_path), "--dtype", "bf16", "--synthetic_scenes", "4", "--synthetic_voxels", "3000", "--set",
             "MODEL.dsnorm", "True"]
    args, cfg = dt.parse_config(argv)
    assert args.batch_size == 4 and args.ckpt == "ckpt/train_epoch_12.pth" and args.eval_tag == "tag" and args.max_waiting_mins == 1
    assert args.save_to_file and args.save_logit and args.save_feat and args.pretrain_not_strict and args.eval_src and args.sync_bn
    assert args.dtype == "bf16" and args.synthetic_scenes == 4 and cfg.MODEL.dsnorm is True
    d = dt.eval_dir(args, cfg, dt.dataset_config(cfg, args.eval_src))
    assert d == tmp_path / "cfgs" / "synthetic" / "spconv_eval_ds" / "pre" / "eval" / "epoch_12" / "val" / "tag"
    dflt, cfg2 = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_eval_ds.yaml", "--ckpt", str(tmp_path / "best_train.pth"),
                                  "--output_root", str(tmp_path)])
    assert (dflt.workers, dflt.tcp_port, dflt.manual_seed, dflt.print_freq, dflt.eval_tag) == (16, 18888, 666, 1, "default")
    assert dt.eval_dir(dflt, cfg2, dt.dataset_config(cfg2)) == \
        tmp_path / "cfgs" / "synthetic" / "spconv_eval_ds" / "default" / "eval" / "epoch_best" / "val" / "default"
    assert dt.epoch_id(None) == "best" and dt.epoch_id("x/3/model_7_final_19.pth") == "19"


@pytest.mark.parametrize("flag", ["--save_logit", "--save_feat"])
def test_save_logit_and_save_feat_raise(flag):
    from doda_amd import test as dt
    with pytest.raises(NotImplementedError):
        dt.main(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_eval_ds.yaml", "--ckpt", "best_train.pth", flag])

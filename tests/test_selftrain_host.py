"""Self-training stage, host side (no GPU): the companion C ABI include/doda_selftrain.h, the exact radix select of the per-class
ratio thresholds against a numpy restatement of util/pseudo_labels_util.py:93-142, the float64 -> float32 conversion of global
thresholds, the pseudo-label file layout and the `python -m doda_amd.st` command line (reference tool/st.py)."""
import numpy as np
import pytest


def test_selftrain_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses (no launch): null pointers, an out-of-range class count or radix level, a store
    range past the end."""
    lib = native_lib
    assert lib.doda_st_voxel_confidence(None, 10, 16, 4, None, None, 8, None, None, None) == -1
    assert lib.doda_st_voxel_confidence(1, 10, 24, 4, 1, None, 8, 1, 1, None) == -4       # 24 channels
    assert lib.doda_st_voxel_confidence(1, 10, 16, 4, 1, None, 33, 1, 1, None) == -4      # 33 classes
    assert lib.doda_st_point_store(1, 1, 4, 1, 10, 8, 1, 1, 15, 6, None, None) == -1      # offset + n > store length
    assert lib.doda_st_radix_hist(1, 1, 10, 8, 4, 1, 1, None) == -1                       # level 4
    assert lib.doda_st_radix_hist(1, 1, 10, 8, 1, None, 1, None) == -1                    # no prefix past level 0
    assert lib.doda_st_label(1, 1, 10, 8, 1, 256, 1, 1, None) == -1                       # ignore label > 255
    assert lib.doda_st_label(1, 1, 0, 8, 1, 255, None, 1, None) == 0                      # empty: nothing to do


# ------------------------------------------------------------------------------------------------ radix select
def np_level_hist(cls, conf, n_cls):
    """The histograms doda_st_radix_hist counts, by numpy."""
    keys = np.ascontiguousarray(conf, dtype=np.float32).view(np.uint32).astype(np.int64)

    def level_hist(level, prefix):
        shift = 24 - 8 * level
        h = np.zeros((n_cls, 256), dtype=np.int64)
        for c in range(n_cls):
            k = keys[cls == c]
            if level > 0:
                k = k[(k >> (shift + 8)) == (int(prefix[c]) & 0xFFFFFFFF)]
            h[c] = np.bincount((k >> shift) & 255, minlength=256)
        return h
    return level_hist


def np_ratio_thresholds(cls, conf, n_cls, thres_ratio):
    """util/pseudo_labels_util.py:93-142 restated: per class the confidences sorted in descending order, sorted[:max(1,
    int(r * n))][-1]; an empty class 0.0."""
    ratios = list(thres_ratio) * n_cls if len(thres_ratio) == 1 else list(thres_ratio)
    out = []
    for c in range(n_cls):
        vals = sorted(conf[cls == c].tolist(), reverse=True)
        try:
            out.append(vals[:int(max(1, int(ratios[c] * len(vals))))][-1])
        except IndexError:
            out.append(0.0)
    return np.array(out, dtype=np.float32)


def _store(seed, n, n_cls, quantised):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_cls, n).astype(np.uint8)
    cls[cls == 3] = 4                                    # class 3: empty
    one = np.flatnonzero(cls == 5)
    cls[one[1:]] = 6                                     # class 5: one point
    if quantised:                                        # heavy ties: a few distinct values
        conf = rng.choice(np.array([1.0, 0.875, 0.5, 0.5000001, 0.25, 1.0 / 3, 0.0625], dtype=np.float32), n)
    else:
        conf = (rng.random(n, dtype=np.float32) * np.float32(0.97) + np.float32(0.03)).astype(np.float32)
        conf[rng.integers(0, n, n // 50)] = np.float32(1.0)
    return cls, conf.astype(np.float32)


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("ratio", [[0.0], [1e-7], [0.3], [1.0], "per_class"])
def test_host_radix_select_equals_numpy_sort(quantised, ratio):
    from doda_amd import pseudo_labels as pl
    n_cls = 11
    cls, conf = _store(7 + quantised, 60000, n_cls, quantised)
    if ratio == "per_class":
        ratio = [0.0, 1e-7, 0.3, 1.0, 0.5, 0.3, 0.99, 0.05, 1e-7, 0.7, 1.0]
    counts = np.bincount(cls, minlength=n_cls)
    assert counts[3] == 0 and counts[5] == 1
    got = pl.select_thresholds(counts, ratio, np_level_hist(cls, conf, n_cls))
    want = np_ratio_thresholds(cls, conf, n_cls, ratio)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_ratio_ranks_follow_the_reference_rule():
    from doda_amd import pseudo_labels as pl
    assert pl.ratio_ranks([0, 1, 10, 10, 10, 3], [0.3]) == [0, 1, 3, 3, 3, 1]
    assert pl.ratio_ranks([10, 10, 10, 7], [0.0, 1e-7, 1.0, 0.99]) == [1, 1, 10, 6]
    with pytest.raises(ValueError):
        pl.ratio_ranks([1, 2, 3], [0.1, 0.2])


# ------------------------------------------------------------------------------------------------ global thresholds
@pytest.mark.parametrize("t64", [0.7, 0.5, 0.9, 1.0])
def test_global_threshold_is_an_exact_fp32_lower_bound(t64):
    from doda_amd import pseudo_labels as pl
    t32 = pl.global_thresholds([t64], 3)
    assert t32.dtype == np.float32 and t32.shape == (3,)
    base = np.array([t64], dtype=np.float32).view(np.int32)[0]
    x = (base + np.arange(-(1 << 16), (1 << 16) + 1, dtype=np.int64)).astype(np.int32).view(np.float32)
    assert np.array_equal(x.astype(np.float64) > t64, x > t32[0])
    assert np.array_equal(pl.global_thresholds([0.7, 0.5, 0.9], 3), np.concatenate([pl.global_thresholds([t], 1) for t in (0.7, 0.5, 0.9)]))


# ------------------------------------------------------------------------------------------------ files
def test_pseudo_label_files_layout_and_no_overwrite(tmp_path):
    from doda_amd import pseudo_labels as pl
    d = tmp_path / "pseudo_labels"
    a = np.array([0, 255, 7, 19, 255], dtype=np.uint8)
    assert pl.write_scene_labels(d, pl.scene_name("/x/scene_s501000_v6000_x50.npz"), a)
    f = d / "txt" / "scene_s501000_v6000_x50.txt"
    assert f.read_text() == "0\n255\n7\n19\n255\n"
    assert not pl.write_scene_labels(d, "scene_s501000_v6000_x50", np.zeros(5, np.uint8))      # kept as it was
    assert f.read_text() == "0\n255\n7\n19\n255\n"
    got = pl.read_scene_labels(d, ["/y/scene_s501000_v6000_x50.npz"])
    assert got[0].dtype == np.int32 and np.array_equal(got[0], a.astype(np.int32))
    kept = np.array([3, 0, 1, 996], dtype=np.int64)
    pl.write_summary(d, kept)
    ratio = np.loadtxt(d / "class_ratio.txt")
    assert ratio.shape == (4,) and abs(ratio.sum() - 1.0) < 1e-12 and ratio[1] == 0.0
    assert np.loadtxt(d / "done.txt") == 1 and pl.is_done(d)


def test_existing_done_flag_skips_generation(tmp_path):
    """set_pseudo_labels: pseudo labels are generated only while done.txt is absent (a resumed run reuses the files)."""
    from doda_amd import pseudo_labels as pl
    (tmp_path / "done.txt").write_text("1\n")
    assert pl.generate(model=None, cfg=None, paths=["/nonexistent.npz"], pseudo_dir=tmp_path, device=None) is None


# ------------------------------------------------------------------------------------------------ command line
REFERENCE_ST_FLAGS = [   # tool/st.py:34-62
    ("--cfg_file", "doda_amd/cfgs/synthetic/spconv_st.yaml"), ("--batch_size", "4"), ("--epochs", "3"), ("--workers", "2"),
    ("--extra_tag", "pre"), ("--st_extra_tag", "st2"), ("--start_epoch", "1"), ("--resume", "r.pth"), ("--weight", "w.pth"),
    ("--weight_ema", None), ("--launcher", "none"), ("--tcp_port", "18888"), ("--sync_bn", None), ("--reserve_old_ckpt", None),
    ("--manual_seed", "5"), ("--ckpt_save_freq", "2"), ("--print_freq", "3"), ("--pseudo_labels_freq", "7"),
    ("--preserve_pseudo_labels", None), ("--local_rank", "0"), ("--max_ckpt_save_num", "9"), ("--pin_memory", None),
]


def test_st_command_line_accepts_every_reference_flag_and_resolves_paths(tmp_path):
    from doda_amd import st
    argv = []
    for flag, val in REFERENCE_ST_FLAGS:
        if flag == "--weight_ema":
            continue
        argv += [flag] + ([val] if val is not None else [])
    argv += ["--output_root", str(tmp_path), "--synthetic_scenes", "4", "--synthetic_voxels", "3000", "--set",
             "SELF_TRAIN.global_thres", "True"]
    args, cfg = st.parse_config(argv)
    assert args.batch_size == 4 and args.epochs == 3 and args.st_extra_tag == "st2" and args.pseudo_labels_freq == 7
    assert args.preserve_pseudo_labels and args.sync_bn and args.pin_memory and args.self_train
    assert cfg.SELF_TRAIN.global_thres is True and cfg.SELF_TRAIN.thres == [0.7] and cfg.SELF_TRAIN.thres_ratio == [0.3]
    pre, out, ckpt, pseudo = st.run_dirs(args, cfg)
    assert pre == tmp_path / "cfgs" / "synthetic" / "spconv_st" / "pre"
    assert out == pre / "st2" and ckpt == out / "ckpt" and pseudo == out / "pseudo_labels"
    d_args, _ = st.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st.yaml"])
    assert d_args.weight == "best_train.pth" and d_args.st_extra_tag == "st" and not d_args.preserve_pseudo_labels
    (pre / "ckpt").mkdir(parents=True)
    (pre / "ckpt" / "best_train.pth").write_bytes(b"")
    assert st.resolve_weight("best_train.pth", pre) == str(pre / "ckpt" / "best_train.pth")
    with pytest.raises(FileNotFoundError):
        st.resolve_weight("absent.pth", pre)
    e_args, _ = st.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st.yaml", "--weight_ema", "t.pth"])
    assert e_args.weight_ema == "t.pth"

"""The DATA_AUG pipeline (scene_aug, elastic, crop), host side (no GPU): the companion C ABI include/doda_aug.h, the host plan of
doda_amd.aug against what the reference's own DataAugmentor computed (tests/golden/aug_golden.npz, made by
tests/golden/make_aug_golden.py), the configuration and the command line."""
import os

import numpy as np
import pytest

from tests import aug_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aug_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses without a launch: offsets that do not start at 0 or decrease, too many segments,
    grids that are too large or degenerate, null pointers, mask pointers that do not pair up; an empty batch is nothing to do."""
    import ctypes as C
    lib = native_lib
    off = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    assert lib.doda_aug_blocks(off(0, 1024, 1025, 1025), 3) == 2
    assert lib.doda_aug_blocks(off(1, 5), 1) == -1 and lib.doda_aug_blocks(off(0, 5, 4), 2) == -1
    assert lib.doda_aug_blocks(off(0, 1 << 31), 1) == -1
    assert lib.doda_aug_affine(1, off(0, 5, 4), 2, 1, 50.0, 1, 1, 1, None) == -1                 # decreasing offsets
    assert lib.doda_aug_affine(1, off(*range(66)), 65, 1, 50.0, 1, 1, 1, None) == -4             # 65 segments
    assert lib.doda_aug_affine(None, off(0, 5), 1, 1, 50.0, 1, 1, 1, None) == -1                 # no points
    assert lib.doda_aug_affine(1, off(0, 5), 1, 1, 0.0, 1, 1, 1, None) == -1                     # scale 0
    assert lib.doda_aug_affine(1, off(0, 5), 1, None, 50.0, 1, 1, 1, None) == -1                 # no matrices
    assert lib.doda_aug_blur(1, 1, i32(4, 1, 4), 1, None) == -1                                  # an axis of one cell
    assert lib.doda_aug_blur(1, 1, i32(4096, 4096, 2), 1, None) == -4                            # 2^25 cells
    assert lib.doda_aug_blur(None, 1, i32(4, 4, 4), 1, None) == -1                               # no grids
    assert lib.doda_aug_blur(None, None, i32(0, 0, 0), 1, None) == 0                             # nothing to blur
    assert lib.doda_aug_displace(1, off(0, 5), 1, 1, i32(4, 4, 4), f64(0.0, 40.0), 1, 1, None) == -1   # granularity 0
    assert lib.doda_aug_displace(None, off(0, 5), 1, 1, i32(4, 4, 4), f64(6.0, 40.0), 1, 1, None) == -1
    assert lib.doda_aug_displace(None, off(0, 5), 1, None, i32(0, 0, 0), f64(0.0, 0.0), None, 1, None) == 0    # no segment fires
    assert lib.doda_aug_crop(1, off(0, 5), 1, 1, None, 1, 1, None) == -1                         # no valid array
    assert lib.doda_aug_crop(None, off(0, 0), 1, None, None, None, None, None) == 0              # empty
    emit = lambda **kw: lib.doda_aug_emit(*[kw.get(k, d) for k, d in (
        ("xyz", 1), ("pos", 1), ("labels", 1), ("mask1", None), ("mask2", None), ("off", off(0, 5)), ("n", 1), ("mat", 1), ("fs", 0.0),
        ("par", 1), ("valid", None), ("blk", None), ("sv", i32(0)), ("ob", off(0)), ("b0", 0), ("ol", 1), ("of", 1), ("olab", 1),
        ("om1", None), ("om2", None), ("top", 1), ("len", 5), ("stream", None))])
    assert emit(mask1=1) == -1                                                                   # one mask of a pair
    assert emit(mask1=1, mask2=1) == -1                                                          # masks without outputs
    assert emit(valid=1) == -1                                                                   # flags without chunk counts
    assert emit(sv=i32(1)) == -1                                                                 # a tested segment, no flags
    assert emit(len=-1) == -1 and emit(ob=off(-1)) == -1 and emit(fs=-1.0) == -1
    assert emit(top=None) == -1 and emit(labels=None) == -1
    assert emit(off=off(0, 0), xyz=None, pos=None, labels=None) == 0                             # empty


# ------------------------------------------------------------------------------------------------ the plan against the reference
@pytest.mark.parametrize("i", range(len(ac.CASES)))
def test_plan_reproduces_the_reference_exactly(i):
    """The host plan on the golden's recorded bounds and counts, with the legacy stream replayed from the seed: the matrix (to
    1e-15), bb per pass, the crop tests (offset and full_scale, fp64 equality) and the number, kind and size of the draws."""
    from doda_amd import aug
    with np.load(ac.GOLDEN) as z:
        assert int(z["n_cases"]) == len(ac.CASES)
        g = ac.load_case(z, i)
    case = ac.CASES[i]
    cfg = aug.AugConfig.from_cfg(ac.data_cfg(case))
    assert cfg.enabled
    draws = aug.RandomStateDraws(case["seed"])
    m = aug.scene_matrix(cfg, draws)
    assert (m is not None) == bool(g["has_mat"]) == ("scene_aug" in case["aug_list"])
    if m is not None:
        assert np.abs(m - g["mat"]).max() <= 1e-15
        if case["flip_p"] in (0.0, 1.0):       # (the flip is the sign of the determinant: the jitter is small, the rotation proper)
            assert (np.linalg.det(m) < 0) == (case["flip_p"] == 1.0)
    fires = aug.elastic_fires(cfg, draws)
    assert fires == (g["bb"].shape[0] > 0)
    bounds = g["bounds"]
    if fires:
        params = aug.elastic_params(cfg)
        assert len(params) == g["bb"].shape[0] == bounds.shape[0] - 1
        for j, (gran, mag) in enumerate(params):
            bb = aug.grid_shape(bounds[j, 0], bounds[j, 1], gran)
            assert np.array_equal(bb, g["bb"][j])
            noise = aug.draw_noise(bb, draws)
            assert noise.dtype == np.float32 and noise.shape == (3, *bb)
    plan = aug.CropPlan(bounds[-1, 0], bounds[-1, 1], int(g["n"]), cfg)
    assert plan.volume == bool(g["volume"])
    tests, at = [], 0
    t = plan.volume_test()
    while True:
        if t is not None:
            tests.append(t)
            plan.count = int(g["crop_count"][at])
            at += 1
        t = plan.next_test(draws)
        if t is None:
            break
    assert len(tests) == g["crop_count"].shape[0]
    for k, (off, full) in enumerate(tests):
        assert np.array_equal(off, g["crop_offset"][k]) and np.array_equal(full, g["crop_full"][k])
    assert [k for k, _ in draws.log] == [str(k) for k in g["draw_kinds"]]
    assert [s for _, s in draws.log] == [int(s) for s in g["draw_sizes"]]


def test_golden_covers_what_the_issue_asks_for():
    with np.load(ac.GOLDEN) as z:
        gs = [ac.load_case(z, i) for i in range(len(ac.CASES))]
    assert len(gs) >= 7 and all(12000 <= int(g["n"]) <= 40000 for g in gs)
    assert any(g["crop_count"].shape[0] - int(g["volume"]) >= 3 for g in gs) and any(bool(g["volume"]) for g in gs)
    assert any(g["bb"].shape[0] == 0 for g in gs) and any(not bool(g["has_mat"]) for g in gs)
    assert any(c["voxel_scale"] == 100 for c in ac.CASES) and any(c["apply_to_feat"] for c in ac.CASES)
    flips = [np.linalg.det(g["mat"]) < 0 for g in gs if bool(g["has_mat"])]
    assert any(flips) and not all(flips)
    for g in gs:
        near = np.unpackbits(g["near_coord"])[:g["coords"].size]
        assert near.mean() <= 1e-4


# ------------------------------------------------------------------------------------------------ configuration
SCANNET_DATA_AUG = {          # cfgs/dataset_cfgs/scannet/scannet_cfg.yaml:18-32,60-65 of the reference
    "enabled": True, "aug_list": ["scene_aug", "elastic", "crop", "shuffle"],
    "scene_aug": {"rotation": {"p": 1.0, "value": [0.0, 0.0, 1.0]}, "jitter": True, "flip": {"p": 0.5}},
    "elastic": {"enabled": True, "value": [[6, 40], [20, 160]], "apply_to_feat": False, "p": 1.0}, "shuffle": True,
    "vss": {"enabled": False, "value": 4}, "tacm": {"enabled": True, "split": [2, 2, 1]}}
SCANNET_PROCESSOR = {"point_range": 200000000, "voxel_scale": 50, "cache": False, "max_npoint": 250000, "full_scale": [128, 512],
                     "voxel_mode": 4}


def _yaml(name):
    from doda_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", "synthetic", name))


def test_aug_config_from_the_new_yaml_and_from_the_reference_values():
    from doda_amd import aug
    ref = aug.AugConfig.from_cfg({"DATA_AUG": SCANNET_DATA_AUG, "DATA_PROCESSOR": SCANNET_PROCESSOR})
    cfg = _yaml("spconv_aug.yaml")
    for data_cfg in (cfg.DATA_CONFIG, cfg.DATA_CONFIG_TAR):
        c = aug.AugConfig.from_cfg(data_cfg)
        assert c.enabled and c.aug_list == ["scene_aug", "elastic", "crop", "shuffle"] == ref.aug_list
        assert c.max_npoint == 250000 == ref.max_npoint and c.point_range == 200000000 == ref.point_range
        assert c.full_scale == [128, 512] == ref.full_scale and c.voxel_scale == 50 == ref.voxel_scale
        assert dict(c.elastic) == ref.elastic and c.scene_aug.to_dict() == ref.scene_aug
        assert aug.elastic_params(c) == [(6, 40.0), (20, 160.0)]
    st = _yaml("spconv_st_tacm_aug.yaml")
    assert aug.AugConfig.from_cfg(st.DATA_CONFIG_TAR).enabled and st.DATA_CONFIG_TAR.DATA_AUG.tacm.enabled
    mixed = aug.AugConfig.from_cfg(st.DATA_CONFIG_TAR).with_list(["elastic", "crop", "shuffle"])
    assert mixed.enabled and aug.scene_matrix(mixed, None) is None


def test_no_aug_list_means_disabled_and_the_existing_configs_have_none():
    from doda_amd import aug
    for name in ("spconv.yaml", "spconv_st.yaml", "spconv_st_tacm.yaml"):
        cfg = _yaml(name)
        assert not aug.AugConfig.from_cfg(cfg.DATA_CONFIG).enabled and not aug.AugConfig.from_cfg(cfg.DATA_CONFIG_TAR).enabled
    assert not aug.AugConfig.from_cfg({"DATA_PROCESSOR": SCANNET_PROCESSOR}).enabled
    assert not aug.AugConfig.from_cfg({"DATA_AUG": dict(SCANNET_DATA_AUG, enabled=False), "DATA_PROCESSOR": SCANNET_PROCESSOR}).enabled
    with pytest.raises(NotImplementedError, match="vss"):
        aug.AugConfig.from_cfg({"DATA_AUG": dict(SCANNET_DATA_AUG, aug_list=["scene_aug", "vss", "crop"]), "DATA_PROCESSOR": SCANNET_PROCESSOR})
    with pytest.raises(ValueError, match="unknown"):
        aug.AugConfig(aug_list=["scene_aug", "mirror"])
    with pytest.raises(ValueError, match="aug_list"):
        aug.augment_batch(None, None, [0, 1], aug.AugConfig(), None)


def test_draw_order_without_probabilities_and_with_disabled_sections():
    """check_p draws only where a section has a `p`; a disabled section draws nothing."""
    from doda_amd import aug
    sec = {"aug_list": ["scene_aug", "elastic", "crop"], "scene_aug": {"jitter": False, "flip": {"enabled": False, "p": 0.5},
                                                                       "rotation": {"value": [0.0, 0.0, 1.0]}},
           "elastic": {"enabled": True, "value": [[6, 40]], "apply_to_feat": False}}
    cfg = aug.AugConfig.from_cfg({"DATA_AUG": sec, "DATA_PROCESSOR": SCANNET_PROCESSOR})
    d = aug.RandomStateDraws(3)
    m = aug.scene_matrix(cfg, d)
    assert d.log == [("rand", 1)] * 3 and abs(np.linalg.det(m) - 1.0) < 1e-12 and m[2, 2] == 1.0
    assert aug.elastic_fires(cfg, d) and len(d.log) == 3
    assert not aug.elastic_fires(cfg.with_list(["scene_aug", "crop"]), d)


def test_train_rejects_the_worker_loaders_with_an_aug_list():
    import argparse
    from doda_amd import train
    src = open(train.__file__).read()
    assert "DATA_AUG.aug_list" in src and "host_loader" in src
    ns = argparse.Namespace(host_loader=True, inline_loader=False)
    cfg = _yaml("spconv_aug.yaml")
    with pytest.raises(ValueError, match="aug_list"):
        train.check_aug_loader(cfg, ns)
    train.check_aug_loader(_yaml("spconv.yaml"), ns)
    train.check_aug_loader(cfg, argparse.Namespace(host_loader=False, inline_loader=False))

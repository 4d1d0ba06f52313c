"""Virtual scan simulation, host side (no GPU): the configuration (vss accepted as the first entry of aug_list only), the draw
order of the plan with and without probabilities, the erosion against scipy's, the window bound of the vertex decision, the
restatement's own hull step against a brute-force linear program, and the argument checks of include/doda_vss.h."""
import os

import numpy as np
import pytest

from tests import vss_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _yaml(*parts):
    from doda_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", *parts))


# ------------------------------------------------------------------------------------------------ configuration
def test_aug_config_accepts_vss_first_and_builds_the_reference_values():
    from doda_amd import aug
    cfg = aug.AugConfig(aug_list=["vss", "scene_aug", "crop"], vss_section=dict(vc.VSS), class_names=vc.CLASS_NAMES)
    assert cfg.enabled and cfg.vss.enabled
    c = aug.AugConfig.from_cfg(vc.data_cfg())
    v = c.vss
    assert c.aug_list == ["vss", "scene_aug", "elastic", "crop", "shuffle"] and v.enabled
    assert (v.p, v.value, v.mode, v.radius, v.camera_view) == (1.0, 4, "fixed", 1000.0, 180.0)
    assert dict(v.random_jitter) == {"enabled": True, "value": 0.01, "p": 1.0}
    assert (v.wall, v.floor, v.ceiling, v.ignore_label) == (0, 1, -1, 255)
    assert aug.AugConfig.from_cfg(vc.data_cfg(class_names=["floor", "x", "ceiling", "wall"])).vss.ceiling == 2
    mixed = c.with_list(["elastic", "crop", "shuffle"])
    assert mixed.enabled and not mixed.vss.enabled and mixed.class_names == vc.CLASS_NAMES
    assert c.with_list(["vss", "crop"]).vss.enabled


def test_vss_anywhere_but_first_still_raises_and_bad_sections_are_named():
    from doda_amd import aug
    with pytest.raises(NotImplementedError, match="vss.*first"):
        aug.AugConfig.from_cfg(vc.data_cfg(aug_list=["scene_aug", "vss", "crop"]))
    with pytest.raises(ValueError, match="mode"):
        aug.AugConfig.from_cfg(vc.data_cfg({"mode": "fisheye"}))
    for names in (["floor", "chair"], ["wall", "chair"], []):
        with pytest.raises(ValueError, match="wall|floor"):
            aug.AugConfig.from_cfg(vc.data_cfg(class_names=names))
    # a list that names vss with a disabled or absent section is the list without it, whatever the class names
    assert not aug.AugConfig.from_cfg(vc.data_cfg({"enabled": False}, class_names=[])).vss.enabled
    sec = vc.data_cfg(class_names=[])
    del sec["DATA_AUG"]["vss"]
    assert not aug.AugConfig.from_cfg(sec).vss.enabled


def test_new_configs_carry_the_reference_values():
    from doda_amd import aug
    from doda_amd.train import aug_config_of
    syn = _yaml("synthetic", "spconv_vss.yaml")
    src, tar = aug_config_of(syn, "train"), aug_config_of(syn, "target")
    assert src.vss.enabled and src.aug_list[0] == "vss" and (src.vss.wall, src.vss.floor) == (0, 1)
    assert tar.enabled and not tar.vss.enabled
    front = _yaml("dataset_cfgs", "files", "front3d_vss_cfg.yaml")
    assert front.DATA_AUG.aug_list == ["vss", "scene_aug", "elastic", "crop", "shuffle"]
    assert front.DATA_AUG.vss.to_dict() == vc.VSS and front.DATA_PROCESSOR.to_dict() == vc.PROCESSOR
    da = _yaml("files", "da_front3d_scannet.yaml")
    v = aug_config_of(da, "train").vss                         # (no mapper read here: COMMON_CLASSES names the labels)
    assert v.enabled and (v.wall, v.floor, v.ceiling) == (0, 1, -1) and v.radius == 1000.0
    assert not aug_config_of(da, "target").vss.enabled
    old = _yaml("dataset_cfgs", "files", "front3d_cfg.yaml")
    assert "vss" not in old.DATA_AUG.aug_list and not aug.AugConfig.from_cfg(old).vss.enabled


# ------------------------------------------------------------------------------------------------ draws
def test_integer_draws_replay_numpy():
    from doda_amd import aug
    from doda_amd.segments import SeededDraws
    d, rs = aug.RandomStateDraws(9), np.random.RandomState(9)
    assert [d.randint(7), d.randint(1000), d.randint(3)] == [rs.randint(7), rs.choice(1000), rs.randint(3)]
    assert d.rand() == rs.rand() and d.log == [("randint", 1)] * 3 + [("rand", 1)]
    s = SeededDraws(4)
    got = [s.randint(5) for _ in range(50)]
    assert all(isinstance(v, int) and 0 <= v < 5 for v in got) and len(set(got)) == 5
    assert [SeededDraws(4).randint(5) for _ in range(3)] == got[:1] * 3


def test_stage_draws_nothing_when_disabled_and_one_number_when_p_does_not_fire():
    """vss.run decides from the draws alone whether it runs: no device call is made for a batch in which it does not."""
    from doda_amd import aug, vss
    off = vss.VssConfig(dict(vc.VSS, enabled=False), vc.CLASS_NAMES)
    d = aug.RandomStateDraws(1)
    assert vss.run(None, None, [0, 5], off, [d]) is None and d.log == []
    never = vss.VssConfig(dict(vc.VSS, p=0.0), vc.CLASS_NAMES)
    assert vss.run(None, None, [0, 5, 9], never, [d, d]) is None and d.log == [("rand", 1)] * 2
    no_p = vss.VssConfig({k: v for k, v in vc.VSS.items() if k != "p"}, vc.CLASS_NAMES)
    assert no_p.p is None and no_p.enabled
    empty = aug.RandomStateDraws(2)
    assert vss.run(None, None, [0, 0], no_p, [empty]) is None and empty.log == []


# ------------------------------------------------------------------------------------------------ erosion
@pytest.mark.parametrize("shape,k", [((43, 33), (4, 3)), ((12, 33), (1, 3)), ((130, 104), (10, 10)), ((9, 9), (0, 0)), ((25, 60), (2, 6))])
def test_erosion_equals_scipy_minimum_filter(shape, k):
    from doda_amd import vss
    rng = np.random.default_rng(shape[0])
    img = np.where(rng.random(shape) < 0.97, 255, 0).astype(np.uint8)
    ours, ref = vss.erode(img, *k), vc.erode(img, *k)
    assert np.array_equal(ours, ref) and 0 < (ours > 0).sum() < (img > 0).sum()


def test_erosion_anchor_of_an_even_kernel_and_the_border():
    from doda_amd import vss
    img = np.full((30, 30), 255, dtype=np.uint8)
    assert (vss.erode(img, 10, 10) == 255).all()              # out-of-image pixels do not erode
    img[15, 15] = 0
    er = vss.erode(img, 10, 10)
    rr, cc = np.where(er == 0)                                # offsets -5 .. +4 around a pixel: the hole spreads +5 .. -4
    assert (rr.min(), rr.max(), cc.min(), cc.max()) == (11, 20, 11, 20)
    cams, image, _ = vss.candidates_of(np.ones((30, 30), dtype=np.uint8), np.zeros((30, 30), dtype=np.uint8), np.array([-14.0, -14.0, 0.0]))
    assert cams.shape == (900, 2) and np.array_equal(cams[0], [-1.5, -1.5]) and np.array_equal(cams[1], [-1.5, -1.4])     # row-major


# ------------------------------------------------------------------------------------------------ the window
def test_window_bound():
    from doda_amd import vss
    t = vss.window_bound(1990.0, 2000.0, 0.15)
    assert 0.04 < t < 0.0425                                  # (0.995 - cos 0.15) / sin 0.15
    assert vss.window_bound(1990.0, 2000.0, 0.05) == 0.0      # cos 0.05 > 0.995: such a window proves nothing
    g, hinv, half, theta0 = vss.window_of(1000.0, 10.0)
    assert 0.15 <= theta0 < 0.1502 and g == 14                # (1.5 acos 0.995, just above the smallest window)
    assert 0 < half < vss.window_bound(1990.0, 2000.0, theta0) / np.sqrt(2) and abs(1 / hinv - 2 * np.sin(theta0 / 2)) < 1e-6
    g, _, half, theta0 = vss.window_of(100.0, 5.0)            # the window widens with the relative depth range
    assert g > 0 and half > 0 and 0.15 < theta0 <= 0.5
    assert vss.window_of(10.0, 5.0)[0] == 0 and vss.window_of(2.0, 5.0)[0] == 0      # a radius comparable to the scene: none
    # the bound does what it promises: no point beyond theta0 binds for |t| <= T
    rng = np.random.default_rng(0)
    T, r_min, r_max = vss.window_bound(1990.0, 2000.0, 0.15), 1990.0, 2000.0
    theta = 0.15 + rng.random(20000) * (np.pi - 0.15)
    rj, ri = r_min + rng.random(20000) * (r_max - r_min), r_min + rng.random(20000) * (r_max - r_min)
    assert (rj * np.sin(theta) * T <= ri - rj * np.cos(theta) + 1e-9).all()


def test_restated_hull_step_equals_a_brute_force_linear_program():
    """qhull's vertices of the flipped points plus the origin are the points whose 2-D program (include/doda_vss.h) is feasible."""
    from scipy.optimize import linprog
    pts = vc.shell(120, 1)
    flipped = vc.flip(pts, (0.1, 0.0, -0.2), 50.0)
    ref = vc.hull_vertices(flipped)
    for i in range(0, 120, 3):
        p = flipped[i]
        ph = p / np.linalg.norm(p)
        e1 = np.cross(ph, [1.0, 0.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(ph, e1)
        d = p - np.delete(flipped, i, 0)
        # maximise the margin s: -(E d) . t + s <= ph . d
        A = np.column_stack((-(d @ e1), -(d @ e2), np.ones(d.shape[0])))
        res = linprog([0, 0, -1], A_ub=A, b_ub=d @ ph, bounds=[(-1e6, 1e6), (-1e6, 1e6), (None, 1.0)])
        assert res.status == 0 and (res.x[2] > 1e-9) == bool(ref[i]), (i, res.x, ref[i])
    assert 0 < ref.sum() < 120


# ------------------------------------------------------------------------------------------------ the C ABI
def test_vss_entry_points_report_bad_arguments(native_lib):
    import ctypes as C
    lib = native_lib
    off = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    assert lib.doda_vss_abi_version() == 1
    assert lib.doda_vss_blocks(off(0, 1024, 1025, 1025), 3) == 2 and lib.doda_vss_blocks(off(1, 5), 1) == -1
    assert lib.doda_vss_bounds(1, 1, off(0, 5, 4), 2, 255, 1, 1, 1, None) == -1                   # decreasing offsets
    assert lib.doda_vss_bounds(1, 1, off(*range(66)), 65, 255, 1, 1, 1, None) == -4               # 65 segments
    assert lib.doda_vss_bounds(None, 1, off(0, 5), 1, 255, 1, 1, 1, None) == -1
    assert lib.doda_vss_image(1, 1, off(0, 5), 1, 255, 1, -1, None, 1, 10, None) == -1            # no frame
    assert lib.doda_vss_image(1, 1, off(0, 5), 1, 255, 1, -1, 1, 1, -1, None) == -1
    assert lib.doda_vss_image(None, None, off(0, 5), 1, 255, 1, -1, None, None, 0, None) == 0     # no image: nothing to do
    assert lib.doda_vss_view(1, 1, off(0, 5), 1, 255, None, 1, 1, None) == -1
    assert lib.doda_vss_view(None, None, off(0, 0), 1, 255, None, None, None, None) == 0          # empty
    assert lib.doda_vss_flip(1, off(0, 5), 1, 1, 1, f64(0.0, 1.0, 4, 0), 1, 1, None) == -1        # radius 0
    assert lib.doda_vss_flip(1, off(0, 5), 1, 1, 1, f64(10.0, 1.0, 65, 0), 1, 1, None) == -4      # 65 cells per axis
    assert lib.doda_vss_flip(1, off(0, 5), 1, 1, 1, f64(10.0, 0.0, 4, 0), 1, 1, None) == -1       # a grid without a cell size
    assert lib.doda_vss_flip(1, off(0, 5), 1, 1, None, f64(10.0, 1.0, 4, 0), 1, 1, None) == -1
    ext = lambda **kw: lib.doda_vss_extreme(*[kw.get(k, d) for k, d in (
        ("pts", 1), ("index", 1), ("begin", i32(0, 5)), ("n", 1), ("cells", 1), ("win", f64(4, 1.0, 0.01, 0)), ("queries", None), ("nq", 5),
        ("flags", 0), ("selected", 1), ("state", 1), ("stream", None))])
    assert ext(begin=i32(1, 5)) == -1 and ext(begin=i32(0, 5, 4), n=2, win=f64(*[0] * 8)) == -1
    assert ext(nq=4) == -1                                                                       # all rows means all rows
    assert ext(flags=2) == -1 and ext(cells=None) == -1 and ext(selected=None) == -1
    assert ext(win=f64(65, 1.0, 0.01, 0)) == -4
    assert ext(begin=i32(0, 0), nq=0, pts=None, index=None) == 0                                 # empty
    assert lib.doda_vss_count(None, off(0, 5), 1, 1, 1, None) == -1 and lib.doda_vss_count(None, off(0, 0), 1, None, None, None) == 0
    emit = lambda **kw: lib.doda_vss_emit(*[kw.get(k, d) for k, d in (
        ("xyz", 1), ("noise", None), ("labels", 1), ("m1", None), ("m2", None), ("off", off(0, 5)), ("n", 1), ("sel", 1), ("blk", 1),
        ("ob", off(0)), ("ox", 1), ("ol", 1), ("oi", 1), ("om1", None), ("om2", None), ("len", 5), ("stream", None))])
    assert emit(m1=1) == -1 and emit(m1=1, m2=1) == -1 and emit(len=-1) == -1 and emit(ob=off(-1)) == -1
    assert emit(sel=None) == -1 and emit(oi=None) == -1
    assert emit(off=off(0, 0), xyz=None, labels=None, sel=None, blk=None) == 0                   # empty

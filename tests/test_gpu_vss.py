"""Virtual scan simulation on the MI355X (doda_amd.vss, include/doda_vss.h) against the numpy / scipy restatement of the reference's
steps (tests/vss_cases.py; the hull step is qhull on the fp64 flipped points plus the origin).

Bounds.  The vertex decision must EQUAL qhull's on every point whose qhull answer does not change when the flipped coordinates are
perturbed by a relative 1e-9; at most 0.1 % of the points may be left out that way.  The windowed route and the exhaustive route
must give bit-equal masks.  The occupancy image, the candidate list, the view masks (the designed inputs have no point within a
relative 1e-12 of a threshold) and the kept indices are exact; downstream voxel coordinates are those of the same pipeline run on
the restatement's output, so they are equal too."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vss_cases as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def reference(step, camera, radius):
    """(points relative to nothing, qhull's vertices, borderline) of the room at `step` seen from CAMERAS[camera]; computed once."""
    key = (step, camera, radius)
    if key not in _CACHE:
        pts, _ = vc.room(step)
        flipped = vc.flip(pts, vc.CAMERAS[camera], radius)
        _CACHE[key] = (pts, vc.hull_vertices(flipped), vc.borderline(flipped))
    return _CACHE[key]


HULL_CASES = [(0.05, 0, 1000), (0.05, 1, 1000), (0.1, 0, 100), (0.1, 1, 10)]


@pytest.mark.parametrize("step,camera,radius", HULL_CASES)
def test_vertex_decision_equals_qhull_and_windowed_equals_exhaustive(native_lib, step, camera, radius):
    from doda_amd import vss
    pts, ref, near = reference(step, camera, radius)
    assert pts.shape[0] == {0.05: 13896, 0.1: 3616}[step]
    stats = []
    ours = vss.hidden_point_removal(_d(pts), vc.CAMERAS[camera], radius, stats=stats).cpu().numpy()
    full = vss.hidden_point_removal(_d(pts), vc.CAMERAS[camera], radius, exhaustive=True).cpu().numpy()
    wrong = (ours != ref) & ~near
    print("step %g camera %d radius %g: qhull keeps %d of %d, ours %d; %d borderline, %d differ; %s"
          % (step, camera, radius, ref.sum(), ref.size, ours.sum(), near.sum(), wrong.sum(), stats))
    assert near.mean() <= 1e-3
    assert wrong.sum() == 0
    assert np.array_equal(ours, full)
    assert 10 < ref.sum() < ref.size
    if radius == 1000:
        assert stats[0]["windowed"] == pts.shape[0]          # (the window exists at the reference's radius)


@pytest.mark.parametrize("n", [10, 63, 64, 65, 1023, 1024, 1025])
def test_sizes_around_the_wave_and_the_chunk(native_lib, n):
    from doda_amd import vss
    pts = vc.shell(n, 100 + n)
    for radius in (1000, 10):
        flipped = vc.flip(pts, (0.0, 0.0, 0.0), radius)
        ref, near = vc.hull_vertices(flipped), vc.borderline(flipped)
        ours = vss.hidden_point_removal(_d(pts), (0.0, 0.0, 0.0), radius).cpu().numpy()
        assert near.mean() <= 1e-3
        assert np.array_equal(ours[~near], ref[~near])


def test_exact_duplicates_keep_the_lowest_index(native_lib):
    from doda_amd import vss
    pts = vc.shell(300, 5)
    ref = vc.hidden_point_removal(pts, (0.0, 0.0, 0.0), 100)       # (radius 100: windowed, and a fair share of hidden points)
    seen, hidden = int(np.nonzero(ref)[0][3]), int(np.nonzero(~ref)[0][3])
    both = np.concatenate((pts, pts[[seen, hidden]]), 0)
    for exhaustive in (False, True):
        ours = vss.hidden_point_removal(_d(both), (0.0, 0.0, 0.0), 100, exhaustive=exhaustive).cpu().numpy()
        assert np.array_equal(ours[:300], ref) and not ours[300] and not ours[301]
    swapped = both[::-1].copy()                               # the copies first: now THEY are the lowest index
    ours = vss.hidden_point_removal(_d(swapped), (0.0, 0.0, 0.0), 100).cpu().numpy()[::-1]
    assert ours[300] and not ours[seen] and not ours[301] and not ours[hidden]


# ------------------------------------------------------------------------------------------------ frame, image, view masks
def _scene32(step=0.1, ignore_share=0.05, seed=3):
    pts, lab = vc.room(step)
    rng = np.random.default_rng(seed)
    lab = lab.copy()
    lab[rng.random(lab.shape[0]) < ignore_share] = vc.IGNORE
    return (pts - pts.mean(0)).astype(np.float32), lab


def _planes(xyz32, lab, class_names):
    """The device's two occupancy planes and the host's frame for one scene."""
    import ctypes as C
    from doda_amd import _lib, vss
    L = _lib.lib()
    n = xyz32.shape[0]
    off = (C.c_int64 * 2)(0, n)
    x, l = _d(xyz32), _d(lab.astype(np.int32))
    part, bounds, cnt = torch.empty((8, 6), device=dev()), torch.empty((1, 2, 3), device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())
    nb = L.doda_vss_blocks(off, 1)
    part = torch.empty((max(1, nb), 6), device=dev())
    _lib.check(L.doda_vss_bounds(x.data_ptr(), l.data_ptr(), off, 1, vc.IGNORE, part.data_ptr(), bounds.data_ptr(), cnt.data_ptr(), None), "bounds")
    b = bounds.cpu().numpy()[0]
    sel = lab != vc.IGNORE
    assert int(cnt.item()) == sel.sum() and np.array_equal(b[0], xyz32[sel].min(0)) and np.array_equal(b[1], xyz32[sel].max(0))
    c, vmin, (H, W), height, lo, hi = vss.frame_of(b[0], b[1])
    frame = _d(np.array([[*c, vmin[0], vmin[1], H, W, 0]], dtype=np.float64))
    img = torch.zeros(2 * H * W, dtype=torch.uint8, device=dev())
    floor = class_names.index("floor")
    ceiling = class_names.index("ceiling") if "ceiling" in class_names else -1
    _lib.check(L.doda_vss_image(x.data_ptr(), l.data_ptr(), off, 1, vc.IGNORE, floor, ceiling, frame.data_ptr(), img.data_ptr(), 2 * H * W, None), "image")
    return img.cpu().numpy().reshape(2, H, W), c, vmin, height


@pytest.mark.parametrize("case", ["room", "narrow", "ceiling"])
def test_occupancy_image_and_candidates_equal_the_restatement(native_lib, case):
    from doda_amd import vss
    xyz32, lab = _scene32()
    names = list(vc.CLASS_NAMES)
    if case == "narrow":                                      # 0.9 m wide: an image of 12 cells, a kernel of one row
        keep = (xyz32[:, 0] > -0.5) & (xyz32[:, 0] < 0.4)
        xyz32, lab = xyz32[keep], lab[keep]
    if case == "ceiling":                                     # a ceiling class: the box top becomes one and no longer blocks its cells
        names[2] = "ceiling"
    planes, c, vmin, height = _planes(xyz32, lab, names)
    sel = lab != vc.IGNORE
    _xyz, c_ref = vc.frame(xyz32, sel)
    cams_ref, img_ref, er_ref, height_ref = vc.camera_candidates(_xyz, lab[sel], names)
    cams, img, er = vss.candidates_of(planes[0], planes[1], vmin)
    assert np.array_equal(c, c_ref) and height == height_ref
    assert img.shape == img_ref.shape and np.array_equal(img, img_ref) and np.array_equal(er, er_ref)
    assert np.array_equal(cams, cams_ref) and cams.shape[0] > 0
    kh, kw = min(10, img.shape[0] // 10), min(10, img.shape[1] // 10)
    print("%s: image %s, kernel %d x %d, %d candidates" % (case, img.shape, kh, kw, cams.shape[0]))
    assert (kh < 10) if case == "narrow" else kh % 2 == 0    # (the even-kernel anchor: 4 rows for the 43-row image)


@pytest.mark.parametrize("mode", ["fixed", "parallel", "perspective"])
def test_view_masks_equal_numpy(native_lib, mode):
    import ctypes as C
    from doda_amd import _lib, vss
    L = _lib.lib()
    xyz32, lab = _scene32()
    n = xyz32.shape[0]
    sel = lab != vc.IGNORE
    _xyz, c = vc.frame(xyz32, sel)
    vcfg = vss.VssConfig(dict(vc.VSS, mode=mode, camera_view=70), vc.CLASS_NAMES, vc.IGNORE)
    off = (C.c_int64 * 2)(0, n)
    x, l = _d(xyz32), _d(lab.astype(np.int32))
    total = 0
    for k, (camera, pick) in enumerate([((0.9, -0.4, 1.9), 17), ((-0.3, 0.2, 1.3), 900), ((0.5, 0.5, 0.4), 2500)]):
        interest = _xyz[pick]
        cam_f, f = np.array(camera) - interest, _xyz - interest
        ref = vc.view_mask(f, cam_f, mode, 70)
        # leave out points within a relative 1e-12 of a threshold (the designed input has none)
        dot = f[:, 0] * cam_f[0] + f[:, 1] * cam_f[1]
        assert np.abs(dot - (cam_f[0] ** 2 + cam_f[1] ** 2)).min() > 1e-12 * (cam_f[0] ** 2 + cam_f[1] ** 2)
        row = vss.view_row(vcfg, c, interest, np.array(camera))
        mask, cnt = torch.empty(n, dtype=torch.uint8, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())
        _lib.check(L.doda_vss_view(x.data_ptr(), l.data_ptr(), off, 1, vc.IGNORE, _d(row[None]).data_ptr(), mask.data_ptr(), cnt.data_ptr(), None), "view")
        got = mask.cpu().numpy().astype(bool)
        assert not got[~sel].any() and np.array_equal(got[sel], ref) and int(cnt.item()) == ref.sum()
        total += ref.sum()
    assert 0 < total < 3 * sel.sum()


# ------------------------------------------------------------------------------------------------ the stage and the pipeline
class Scripted:
    """RandomStateDraws with the scalar rand() and randint() answers taken from a script first."""

    def __new__(cls, seed, rands=(), ints=()):
        from doda_amd import aug

        class _S(aug.RandomStateDraws):
            def rand(self, n=None):
                if n is None and self.rands:
                    self.log.append(("rand", 1))
                    return self.rands.pop(0)
                return super().rand(n)

            def randint(self, n):
                if self.ints:
                    self.log.append(("randint", 1))
                    return self.ints.pop(0) % n
                return super().randint(n)
        s = _S(seed)
        s.rands, s.ints = list(rands), list(ints)
        return s


def _run_stage(scenes, draws, vss_over=None, **kw):
    from doda_amd import aug, vss
    cfg = aug.AugConfig.from_cfg(vc.data_cfg(vss_over))
    offsets = np.concatenate(([0], np.cumsum([s[0].shape[0] for s in scenes]))).tolist()
    out = vss.run(_d(np.concatenate([s[0] for s in scenes])), _d(np.concatenate([s[1] for s in scenes]).astype(np.int32)), offsets, cfg.vss,
                  draws, return_debug=True, **kw)
    torch.cuda.synchronize()
    return out, offsets


def _covered(xyz32, lab):
    """Furniture over every floor cell: no camera candidate."""
    fl = lab == vc.FLOOR
    top = xyz32[fl].copy()
    top[:, 2] += 0.4
    return np.concatenate((xyz32, top)), np.concatenate((lab, np.full(int(fl.sum()), vc.BOX, dtype=lab.dtype)))


def test_stage_equals_the_restatement_on_a_batch_with_an_exit(native_lib):
    """Three scenes: the room, the room with furniture over every floor cell (no candidate: all labelled points, jittered), the
    room in perspective-free `parallel` mode is covered elsewhere; here the kept indices, the jittered xyz and the draw log."""
    from doda_amd import aug
    a, b = _scene32(0.1, 0.05, 3), _covered(*_scene32(0.1, 0.05, 4))
    c = _scene32(0.1, 0.0, 5)
    scenes, seeds = [a, b, c], [31, 32, 33]
    draws = [aug.RandomStateDraws(s) for s in seeds]
    out, offsets = _run_stage(scenes, draws)
    new = out["offsets"]
    for k, ((xyz32, lab), seed) in enumerate(zip(scenes, seeds)):
        rs = np.random.RandomState(seed)
        assert rs.rand() < 1.0                                # the section's p
        ref_xyz, ref_sel, log = vc.virtual_scan(vc.VSS, xyz32, lab, vc.CLASS_NAMES, rs)
        idx = out["index"][new[k]:new[k + 1]].cpu().numpy() - offsets[k]
        print("scene %d: kept %d of %d (restatement %d), %d attempts" % (k, idx.size, lab.size, ref_sel.sum(), len(log)))
        assert np.array_equal(idx, np.nonzero(ref_sel)[0])
        assert np.array_equal(out["xyz"][new[k]:new[k + 1]].cpu().numpy(), ref_xyz[ref_sel])
        assert np.array_equal(out["labels"][new[k]:new[k + 1]].cpu().numpy(), lab[ref_sel].astype(np.int32))
        attempts = out["debug"]["samples"][k].log
        assert [m for _, _, m in attempts] == [m for _, _, m in log]
        n = lab.size
        expect = [("rand", 1), ("rand", 1)] + [("randint", 1)] * (2 * len(log)) + [("rand", 1), ("rand", 3 * n)]
        assert draws[k].log == expect
        if k == 1:
            assert len(log) == 0 and np.array_equal(ref_sel, lab != vc.IGNORE)
        else:
            assert 0 < ref_sel.sum() < (lab != vc.IGNORE).sum()
    # the exhaustive route gives the same batch, bit for bit
    full, _ = _run_stage(scenes, [aug.RandomStateDraws(s) for s in seeds], exhaustive=True)
    assert full["offsets"] == new and torch.equal(full["index"], out["index"]) and torch.equal(full["xyz"], out["xyz"])


def test_a_scene_of_ignored_labels_is_reported_empty(native_lib):
    from doda_amd import aug
    a = _scene32(0.1, 0.05, 3)
    scenes = [a, (a[0], np.full_like(a[1], vc.IGNORE)), a]
    with pytest.raises(aug.EmptySample) as e:
        _run_stage(scenes, [aug.RandomStateDraws(s) for s in (1, 2, 3)])
    assert e.value.index == 1


def _tower():
    """The room with nine wall points in a 1 cm cluster 1.4 m above everything else: a view that looks at one of them from below
    holds exactly those nine points."""
    xyz32, lab = _scene32(0.1, 0.0, 3)
    rng = np.random.default_rng(9)
    top = np.array([xyz32[:, 0].min(), xyz32[:, 1].min(), xyz32[:, 2].max() + 1.4]) + rng.random((9, 3)) * 0.01
    return np.concatenate((xyz32, top.astype(np.float32))), np.concatenate((lab, np.full(9, vc.WALL, dtype=lab.dtype)))


def test_a_view_of_nine_points_consumes_an_attempt(native_lib):
    xyz32, lab = _tower()
    n, n_wall = lab.size, int((lab == vc.WALL).sum())
    # camera height 0.5 * height + 0.25 * height: below the cluster, above the room; first interest point: the last wall point
    out, _ = _run_stage([(xyz32, lab)], [Scripted(5, rands=[0.0, 0.5], ints=[0, n_wall - 1])])
    s = out["debug"]["samples"][0]
    assert s.log[0][2] == 9 and s.tries >= 1 and s.views == 4 and not s.exit_all
    assert all(m >= 10 for _, _, m in s.log[s.tries:]) or s.tries > 1
    # every attempt looks at the cluster: max(5, 4) + 1 failures, then every labelled point, jittered
    out, _ = _run_stage([(xyz32, lab)], [Scripted(6, rands=[0.0, 0.5], ints=[0, n_wall - 1] * 6)])
    s = out["debug"]["samples"][0]
    assert [m for _, _, m in s.log] == [9] * 6 and s.exit_all and s.views == 0
    assert out["index"].cpu().numpy().tolist() == list(range(n))
    assert not torch.equal(out["xyz"], _d(xyz32)) and float((out["xyz"] - _d(xyz32)).abs().max()) <= 0.005 + 1e-6


def test_pipeline_with_vss_first_equals_the_pipeline_on_the_restatement(native_lib):
    """augment_batch under [vss, scene_aug, elastic, crop, shuffle]: the kept indices are the restatement's, and the voxel
    coordinates are those of the rest of the list run on the restatement's output with the same stream of draws."""
    from doda_amd import aug
    xyz32, lab = _scene32(0.1, 0.05, 3)
    cfg = aug.AugConfig.from_cfg(vc.data_cfg())
    assert cfg.vss.enabled and cfg.aug_list[0] == "vss"
    d = aug.RandomStateDraws(77)
    out = aug.augment_batch(_d(xyz32), _d(lab.astype(np.int32)), [0, lab.size], cfg, d, return_debug=True)
    r = aug.RandomStateDraws(77)
    assert r.rs.rand() < 1.0
    ref_xyz, ref_sel, log = vc.virtual_scan(vc.VSS, xyz32, lab, vc.CLASS_NAMES, r.rs)
    rest = aug.AugConfig.from_cfg(vc.data_cfg(aug_list=["scene_aug", "elastic", "crop", "shuffle"]))
    ref = aug.augment_batch(_d(ref_xyz[ref_sel]), _d(lab[ref_sel].astype(np.int32)), [0, int(ref_sel.sum())], rest, r)
    torch.cuda.synchronize()
    assert np.array_equal(out["debug"]["vss"]["index"].cpu().numpy(), np.nonzero(ref_sel)[0])
    for k in ("locs32", "locs_float", "labels32"):
        assert torch.equal(out[k], ref[k]), k
    assert out["offsets"].tolist() == ref["offsets"].tolist() and np.array_equal(out["spatial_shape"], ref["spatial_shape"])
    n = lab.size
    head = [("rand", 1), ("rand", 1)] + [("randint", 1)] * (2 * len(log)) + [("rand", 1), ("rand", 3 * n)]
    assert d.log == head + r.log and len(log) >= 4
    # vss whose p does not fire, or a disabled section: the list without it
    for over in ({"p": 0.0}, {"enabled": False}):
        off = aug.AugConfig.from_cfg(vc.data_cfg(over))
        d0, d1 = aug.RandomStateDraws(5), aug.RandomStateDraws(5)
        a = aug.augment_batch(_d(xyz32), _d(lab.astype(np.int32)), [0, lab.size], off, d0)
        if "p" in over:
            d1.rand()
        b = aug.augment_batch(_d(xyz32), _d(lab.astype(np.int32)), [0, lab.size], rest, d1)
        assert torch.equal(a["locs32"], b["locs32"]) and d0.log[-len(d1.log):] == d1.log[-len(d1.log):]


def test_device_loader_scans_the_synthetic_scenes(native_lib, tmp_path):
    """DeviceScenes under cfgs/synthetic/spconv_vss.yaml: the scans drop points of every batch, and an epoch repeats bit for bit."""
    from doda_amd.config import cfg_from_yaml_file
    from doda_amd.loader import DeviceScenes, prepare_cache
    from doda_amd.train import aug_config_of
    d = dev()
    _, paths = prepare_cache(2, 20000, 50, 1000, str(tmp_path / "scenes"))
    acfg = aug_config_of(cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", "synthetic", "spconv_vss.yaml")), "train")
    assert acfg.vss.enabled
    total = sum(int(np.load(p)["labels"].shape[0]) for p in paths)
    a, b = list(DeviceScenes(paths, 2, 50, 7, 2, 0, 1, d, aug_cfg=acfg)), list(DeviceScenes(paths, 2, 50, 7, 2, 0, 1, d, aug_cfg=acfg))
    assert len(a) == 1 and torch.equal(a[0]["locs32"], b[0]["locs32"]) and torch.equal(a[0]["locs_float"], b[0]["locs_float"])
    kept = np.diff(a[0]["offsets"].tolist())
    print("synthetic scenes: %d points, kept %s" % (total, kept.tolist()))
    assert (kept > 0).all() and kept.sum() < total and a[0]["labels32"].shape[0] == kept.sum()


def test_train_entry_point_runs_two_iterations_with_vss(native_lib, tmp_path):
    cmd = [sys.executable, "-m", "doda_amd.train", "--cfg_file", "doda_amd/cfgs/synthetic/spconv_vss.yaml", "--max_iters", "2",
           "--synthetic_scenes", "8", "--synthetic_base", "4", "--synthetic_voxels", "20000", "--epochs", "1",
           "--scene_cache", str(tmp_path / "scenes"), "--output_root", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

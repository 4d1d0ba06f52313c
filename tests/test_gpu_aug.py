"""The DATA_AUG pipeline on the MI355X: doda_amd.aug.augment_batch (include/doda_aug.h) against the reference's own DataAugmentor
(tests/golden/aug_golden.npz; numpy's legacy stream replayed from each case's seed), the blur against scipy.ndimage, batching and
repeatability, and the two loaders with and without a DATA_AUG.aug_list.

Bounds.  Voxel coordinates and the kept set must EQUAL the reference's wherever the reference's coordinate is farther than 1e-6
from an integer, or exactly 0 (the per-axis minimum), and wherever no crop test had the point within 1e-6 of its boundary; at most
1e-4 of the coordinates / points may be excluded that way.  fp64 positions: 128 * 2^-52 * E (E = the largest |coordinate| at
any stage; about 50 fp64 roundings per pass and coordinate, doubled for contraction differences).  locs_float and the blurred
grids: one fp32 ulp."""
import os

import numpy as np
import pytest
import torch

from tests import aug_cases as ac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def scipy_blur(noise):
    """augmentor_utils.py:62-73 on one fp32 grid, with scipy's own convolve."""
    import scipy.ndimage
    k = [np.ones(s, dtype=np.float32) / 3 for s in ((3, 1, 1), (1, 3, 1), (1, 1, 3))]
    for axis in (0, 1, 2, 0, 1, 2):
        noise = scipy.ndimage.convolve(noise, k[axis], mode="constant", cval=0)
    return noise


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32)))


def capture_draws(seed):
    from doda_amd import aug

    class Capture(aug.RandomStateDraws):
        def __init__(self, s):
            super().__init__(s)
            self.grids = []

        def randn(self, shape):
            v = super().randn(shape)
            if v.ndim == 3 and v.shape != (3, 3):
                self.grids.append(v.astype(np.float32))
            return v
    return Capture(seed)


def run_case(case, **kw):
    from doda_amd import aug
    xyz32, lab = ac.scene(case)
    cfg = aug.AugConfig.from_cfg(ac.data_cfg(case))
    draws = capture_draws(case["seed"])
    out = aug.augment_batch(_d(xyz32), _d(lab.astype(np.int32)), [0, xyz32.shape[0]], cfg, draws, return_debug=True, **kw)
    torch.cuda.synchronize()
    return xyz32, lab, cfg, draws, out


# ------------------------------------------------------------------------------------------------ the reference's own functions
@pytest.mark.parametrize("i", range(len(ac.CASES)))
def test_augment_batch_equals_the_reference_on_every_golden_case(native_lib, i):
    case = ac.CASES[i]
    with np.load(ac.GOLDEN) as z:
        g = ac.load_case(z, i)
    xyz32, lab, cfg, draws, out = run_case(case)
    dbg, n = out["debug"], xyz32.shape[0]
    plan = dbg["plans"][0]
    # the draws, and the host's decisions on the DEVICE's bounds and counts
    assert [k for k, _ in draws.log] == [str(k) for k in g["draw_kinds"]] and [s for _, s in draws.log] == [int(s) for s in g["draw_sizes"]]
    assert np.abs(dbg["mat"][0] - g["mat"]).max() <= 1e-15
    assert len(dbg["bb"]) == g["bb"].shape[0] and all(np.array_equal(dbg["bb"][j][0], g["bb"][j]) for j in range(len(dbg["bb"])))
    E, tol = float(g["E"]), 128 * 2.0 ** -52 * float(g["E"])
    for j, b in enumerate(dbg["bounds"]):
        print("case %d stage %d: bounds deviate by %.3g (tolerance %.3g)" % (i, j, np.abs(b[0] - g["bounds"][j]).max(), tol))
        assert np.abs(b[0] - g["bounds"][j]).max() <= tol
    assert len(plan.tests) == g["crop_count"].shape[0]
    # the blurred grids against scipy's
    for j, grids in enumerate(dbg["grids"]):
        ours = grids.cpu().numpy().reshape(3, *g["bb"][j])
        for k in range(3):
            ref = scipy_blur(draws.grids[3 * j + k])
            err = np.abs(ours[k] - ref) / ulp32(ref)
            print("case %d pass %d grid %d: blur deviates by %.3g fp32 ulp" % (i, j, k, err.max()))
            assert err.max() <= 1.0
    # the kept set
    ref_kept = np.unpackbits(g["kept"])[:n].astype(bool)
    near_pt = np.unpackbits(g["near_point"])[:n].astype(bool)
    kept = dbg["valid"].cpu().numpy().astype(bool) if dbg["valid"] is not None else np.ones(n, dtype=bool)
    assert near_pt.mean() <= 1e-4
    assert np.array_equal(kept[~near_pt], ref_kept[~near_pt])
    print("case %d: kept %d of %d (reference %d), %d points near a crop boundary" % (i, kept.sum(), n, ref_kept.sum(), near_pt.sum()))
    off = out["offsets"].tolist()
    assert off == [0, int(kept.sum())] and out["locs32"].shape == (off[1], 4) and bool((out["locs32"][:, 0] == 0).all())
    # voxel coordinates, on the points both kept
    ours_row, ref_row = np.cumsum(kept) - 1, np.cumsum(ref_kept) - 1
    both = np.nonzero(kept & ref_kept)[0]
    q = out["locs32"][:, 1:].cpu().numpy()[ours_row[both]]
    ref_q = g["coords"].astype(np.int64)[ref_row[both]]
    near = np.unpackbits(g["near_coord"])[:g["coords"].size].astype(bool).reshape(-1, 3)
    assert near.mean() <= 1e-4
    check = ~near[ref_row[both]]
    print("case %d: %d of %d coordinates differ (%d excluded)" % (i, (q != ref_q)[check].sum(), check.sum(), (~check).sum()))
    assert np.array_equal(q[check], ref_q[check])
    assert np.abs(q - ref_q).max() <= 1
    assert np.array_equal(out["labels32"].cpu().numpy()[ours_row[both]], lab[both].astype(np.int32))
    assert np.array_equal(out["spatial_shape"], np.clip(out["locs32"][:, 1:].max(0)[0].cpu().numpy() + 1, case["full_scale"][0], None))
    if dbg["valid"] is not None:
        assert np.array_equal(dbg["top"].cpu().numpy(), out["locs32"][:, 1:].max(0)[0].cpu().numpy() + 1)
    # sampled fp64 positions (before the truncation) of every 16th point
    pos = dbg["pos"].cpu().numpy()[::ac.STRIDE]
    ours_pos = (pos - plan.lo) + plan.offset
    err = np.abs(ours_pos - g["pos16"]).max()
    print("case %d: positions deviate by %.3g voxel (tolerance %.3g, E %.4g)" % (i, err, tol, E))
    assert err <= tol
    # locs_float: fp32 of xyz_middle
    sample = np.arange(0, n, ac.STRIDE)
    sel = kept[sample]
    lf = out["locs_float"].cpu().numpy()[ours_row[sample[sel]]]
    ref_lf = g["mid16"][sel].astype(np.float32)
    err = np.abs(lf.astype(np.float64) - ref_lf.astype(np.float64)) / ulp32(ref_lf)
    print("case %d: locs_float deviates by %.3g fp32 ulp" % (i, err.max()))
    assert err.max() <= 1.0


@pytest.mark.parametrize("shapes", [[(39, 42, 22), (14, 14, 9)], [(2, 2, 2), (0, 0, 0), (3, 50, 2), (83, 80, 34)]])
def test_blur_of_a_batch_of_grids_equals_scipy(native_lib, shapes):
    from doda_amd import aug
    rng = np.random.RandomState(5)
    grids = [rng.randn(3, *s).astype(np.float32) for s in shapes if s[0]]
    noise = aug.blur_grids(_d(np.concatenate([g.reshape(-1) for g in grids])), np.array(shapes)).cpu().numpy()
    at = 0
    for g in grids:
        ours = noise[at:at + g.size].reshape(g.shape)
        at += g.size
        for k in range(3):
            ref = scipy_blur(g[k])
            assert (np.abs(ours[k] - ref) <= ulp32(ref)).all()


def test_batch_of_four_equals_four_single_calls_and_repeats_bit_for_bit(native_lib):
    """Four scenes of different sizes under one configuration whose max_npoint crops two of them and leaves two whole, with
    masks: the batch equals the four single calls (batch index aside) and a repeated call, bit for bit."""
    from doda_amd import aug
    cases = [ac.CASES[k] for k in (0, 2, 5, 7)]
    cfg = aug.AugConfig.from_cfg(ac.data_cfg(dict(ac.CASES[0], max_npoint=15000)))
    scenes = [ac.scene(c) for c in cases]
    rng = np.random.default_rng(3)
    m1 = [(rng.random(s[0].shape[0]) < 0.5).astype(np.uint8) for s in scenes]
    offsets = np.concatenate(([0], np.cumsum([s[0].shape[0] for s in scenes]))).tolist()
    keys = ("locs32", "locs_float", "labels32", "mask1", "mask2")

    def batch():
        out = aug.augment_batch(_d(np.concatenate([s[0] for s in scenes])), _d(np.concatenate([s[1] for s in scenes]).astype(np.int32)),
                                offsets, cfg, [aug.RandomStateDraws(c["seed"]) for c in cases],
                                masks=(_d(np.concatenate(m1)), _d(1 - np.concatenate(m1))), return_debug=True)
        torch.cuda.synchronize()
        return out
    a, b = batch(), batch()
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert a["offsets"].tolist() == b["offsets"].tolist() and np.array_equal(a["spatial_shape"], b["spatial_shape"])
    off = a["offsets"].tolist()
    sizes = np.diff(off)
    tested = [p.tested for p in a["debug"]["plans"]]
    assert tested == [True, True, False, False] and all(s <= 15000 for s in sizes) and sizes[2] == 12000 and sizes[3] == 14000
    assert a["mask1"].dtype == torch.bool and not bool((a["mask1"] & a["mask2"]).any()) and bool((a["mask1"] | a["mask2"]).all())
    top = np.zeros(3, dtype=np.int64)
    for s, (c, (xyz, lab)) in enumerate(zip(cases, scenes)):
        one = aug.augment_batch(_d(xyz), _d(lab.astype(np.int32)), [0, xyz.shape[0]], cfg, aug.RandomStateDraws(c["seed"]),
                                masks=(_d(m1[s]), _d(1 - m1[s])), batch0=s, return_debug=True)
        for k in keys:
            assert torch.equal(one[k], a[k][off[s]:off[s + 1]]), (s, k)
        top = np.maximum(top, one["spatial_shape"])
        valid = one["debug"]["valid"]
        kept = valid.cpu().numpy().astype(bool) if valid is not None else np.ones(xyz.shape[0], dtype=bool)
        assert np.array_equal(one["mask1"].cpu().numpy(), m1[s][kept].astype(bool))
        assert np.array_equal(one["labels32"].cpu().numpy(), lab[kept].astype(np.int32))
    assert np.array_equal(top, a["spatial_shape"])


def test_an_emptied_sample_is_reported(native_lib):
    """A point_range that leaves no room: the volume rule keeps nothing, augment_batch raises EmptySample with the index."""
    from doda_amd import aug
    case = dict(ac.CASES[4], point_range=1e-9)
    xyz32, lab = ac.scene(case)
    cfg = aug.AugConfig.from_cfg(ac.data_cfg(case))
    with pytest.raises(aug.EmptySample) as e:
        aug.augment_batch(_d(xyz32), _d(lab.astype(np.int32)), [0, xyz32.shape[0]], cfg, aug.RandomStateDraws(1))
    assert e.value.index == 0


# ------------------------------------------------------------------------------------------------ the loaders
def _yaml(name):
    from doda_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", "synthetic", name))


def test_device_scenes_with_and_without_an_aug_list(native_lib, tmp_path):
    from doda_amd import aug
    from doda_amd.collate import collate_device_concat
    from doda_amd.loader import DeviceFeeder, DeviceScenes, prepare_cache
    d = dev()
    _, paths = prepare_cache(4, 20000, 50, 1000, str(tmp_path / "scenes"))
    acfg = aug.AugConfig.from_cfg(_yaml("spconv_aug.yaml").DATA_CONFIG)
    small = aug.AugConfig(acfg.aug_list, acfg.scene_aug, acfg.elastic, acfg.voxel_scale, acfg.full_scale, 9000, acfg.point_range)
    for cfg in (acfg, small):
        ds = DeviceScenes(paths, 4, 50, 7, 2, 0, 1, d, aug_cfg=cfg)
        seen = 0
        for hb in ds:
            off = hb["offsets"].tolist()
            q = hb["locs32"]
            n = q.shape[0]
            assert off[0] == 0 and off[-1] == n == hb["locs_float"].shape[0] == hb["labels32"].shape[0] and len(off) == 3
            assert all(0 < b - a <= cfg.max_npoint for a, b in zip(off[:-1], off[1:]))
            assert int(q[:, 1:].min()) >= 0 and int(q[:, 1:].max()) < 512
            assert bool((q[:, 1:].max(0)[0].cpu() < torch.from_numpy(hb["spatial_shape"])).all())
            assert torch.equal(q[:, 0].long(), torch.repeat_interleave(torch.arange(2, device=d), torch.tensor(np.diff(off), device=d)))
            assert len(hb["id"]) == 2 and hb["labels32"].dtype == torch.int32
            batch = collate_device_concat(hb, d)
            assert batch["p2v_map"].shape[0] == n and batch["labels"].dtype == torch.int64
            seen += 1
        assert seen == 2
        if cfg is small:
            sizes = [torch.from_numpy(np.load(p)["labels"]).shape[0] for p in paths]
            assert max(sizes) > 9000             # (the crop loop ran)
    ds = DeviceScenes(paths, 4, 50, 7, 2, 0, 1, d, aug_cfg=acfg)
    a, b = [hb for hb in ds], [hb for hb in ds]
    assert all(torch.equal(x["locs32"], y["locs32"]) and torch.equal(x["locs_float"], y["locs_float"]) for x, y in zip(a, b))
    got = list(DeviceFeeder(iter(ds), d))                                                       # through the feeder thread
    assert len(got) == 2 and all(bt["locs"].shape[0] == bt["locs_float"].shape[0] for bt, _ in got)
    # a validation split is not augmented, and no aug_list is the loader as it was: _rigid + _finish
    ids = [0, 1]
    for kw in (dict(aug_cfg=acfg, augment=False), dict(aug_cfg=aug.AugConfig.from_cfg(_yaml("spconv.yaml").DATA_CONFIG)), dict()):
        new, old = DeviceScenes(paths, 4, 50, 7, 2, 0, 1, d, **kw), DeviceScenes(paths, 4, 50, 7, 2, 0, 1, d, augment=kw.get("augment", True))
        hb, ref = new._batch(ids), old._finish(*old._rigid(ids), ids)
        for k in ("locs32", "locs_float", "labels32", "offsets"):
            assert torch.equal(hb[k], ref[k]), k
        assert np.array_equal(hb["spatial_shape"], ref["spatial_shape"]) and hb["id"] == ref["id"]


def test_mixed_loader_runs_elastic_and_crop_on_the_mixed_points(native_lib, tmp_path):
    from doda_amd import aug, tacm
    from doda_amd.collate import collate_device_concat
    from doda_amd.loader import MixedDeviceScenes, prepare_cache
    from tests import tacm_cases as tc
    d = dev()
    _, tp = prepare_cache(4, 30000, 50, 501000, str(tmp_path / "scenes"))
    _, sp = prepare_cache(4, 30000, 50, 1000, str(tmp_path / "scenes"))
    st = _yaml("spconv_st_tacm_aug.yaml")
    cfg = tacm.TacmConfig.from_cfg(st)
    acfg = aug.AugConfig.from_cfg(st.DATA_CONFIG_TAR)
    sampler = tacm.SplitSampler(cfg)
    labs = np.concatenate([np.load(p)["labels"] for p in tp])
    sampler.init_class_ratio(tc.class_ratio_of(labs.astype(np.int64)))
    sampler.update_cfg(cfg)
    plain = list(MixedDeviceScenes(tp, sp, 4, 50, 7, 2, 0, 1, d, cfg, sampler))
    # a limit that every mixed sample exceeds and that the crop loop's steps of 32 voxels can meet without emptying a sample
    limit = int(0.6 * min(int(v) for hb in plain for v in np.diff(hb["offsets"].tolist())))
    small = aug.AugConfig(acfg.aug_list, acfg.scene_aug, acfg.elastic, acfg.voxel_scale, acfg.full_scale, limit, acfg.point_range)
    for c in (acfg, small):
        ds = MixedDeviceScenes(tp, sp, 4, 50, 7, 2, 0, 1, d, cfg, sampler, aug_cfg=c)
        assert ds.mix_aug_cfg.aug_list == ["elastic", "crop", "shuffle"]
        seen = 0
        for hb, ref in zip(ds, plain):
            off = hb["offsets"].tolist()
            n = hb["locs_float"].shape[0]
            assert off[0] == 0 and off[-1] == n and hb["mask1"].shape == (n,) and hb["mask1"].dtype == torch.bool
            assert int(hb["mask1"].sum() + hb["mask2"].sum()) == n and not bool((hb["mask1"] & hb["mask2"]).any())
            assert all(0 < b - a <= c.max_npoint for a, b in zip(off[:-1], off[1:]))
            q = hb["locs32"]
            assert int(q[:, 1:].min()) >= 0 and bool((q[:, 1:].max(0)[0].cpu() < torch.from_numpy(hb["spatial_shape"])).all())
            assert len(hb["tar_tail_splits"]) == 2 * cfg.num_class and len(hb["tar_splits_class_ratio"]) == cfg.num_class
            if c is acfg:       # nothing cropped: the points of the unaugmented mixed batch, distorted (xyz_middle is not)
                assert n == ref["locs_float"].shape[0] and torch.equal(hb["mask1"], ref["mask1"])
                assert torch.equal(hb["locs_float"], ref["locs_float"]) and torch.equal(hb["labels32"], ref["labels32"])
                assert not torch.equal(hb["locs32"], ref["locs32"])
            else:
                assert n < ref["locs_float"].shape[0]
            batch = collate_device_concat(hb, d)
            assert batch["mask1"] is hb["mask1"] and batch["p2v_map"].shape[0] == n
            seen += 1
        assert seen == 2

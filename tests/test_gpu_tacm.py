"""Tail-aware cuboid mixing on the MI355X: doda_amd.tacm.mix_batch (include/doda_mix.h) against the reference's own tacm()
(tests/golden/tacm_golden.npz, draws replayed), batching and repeatability, a full-size batch against a numpy fp64 restatement, the
mixed loader, `python -m doda_amd.st` with spconv_st_tacm.yaml end to end, and the unmixed configuration left as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tacm_cases as tc
from tests.test_tacm_host import GoldenSampler, golden_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24       # half an fp32 ulp, relative: one rounding to fp32


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def np_cuboid_ids(xyz32, centre32, planes):
    """The reference's membership test in fp64 on the centred fp32 coordinates, the later cuboid winning; 255 = none."""
    x = (xyz32 - centre32[None]).astype(np.float32).astype(np.float64)
    ids = np.full(x.shape[0], 255, dtype=np.int64)
    for q in range(planes.shape[0]):
        ids[np.all(x < planes[q, 0], 1) & np.all(x >= planes[q, 1], 1)] = q
    return ids


# ------------------------------------------------------------------------------------------------ the reference's own function
@pytest.mark.parametrize("i", range(len(tc.CASES)))
def test_mix_batch_equals_the_reference_on_every_golden_case(native_lib, i):
    """Lengths, labels, masks, tar_splits_class_ratio and the tail cuboids' row counts and labels EQUAL; every point's cuboid id
    equal to the fp64 membership test; positions within 4 * 2^-24 * E of the reference's fp64 run (four fp32 roundings on the
    device: centre, move, shrink, recentre; the sums are exact) and within that plus the case's ref_dev of its fp32 run."""
    from doda_amd import tacm
    with np.load(tc.GOLDEN) as z:
        g = tc.load_case(z, i)
    case = tc.CASES[i]
    cfg = golden_cfg(case, g)
    t_xyz, t_lab, s_xyz, s_lab = tc.case_inputs(case)
    sampler = GoldenSampler([it for it in g["items"]])
    for c in sampler.items:
        c.rows = c.rows.to(dev())
    draws = tacm.ReplayDraws(g["draws"])
    out = tacm.mix_batch(_d(t_xyz), _d(t_lab, torch.int32), [0, t_xyz.shape[0]], _d(s_xyz), _d(s_lab, torch.int32), [0, s_xyz.shape[0]],
                         cfg, sampler, draws, return_debug=True)
    assert draws.exhausted()
    n = g["label"].shape[0]
    assert out["xyz_mid"].shape == (n, 3) and out["offsets"] == [0, n]
    assert np.array_equal(out["labels"].cpu().numpy(), g["label"].astype(np.int32))
    m1 = out["mask1"].cpu().numpy()
    assert m1.dtype == bool and np.array_equal(m1, np.arange(n) < int(g["n_pc1"])) and np.array_equal(out["mask2"].cpu().numpy(), ~m1)
    assert np.array_equal(np.asarray(out["tar_splits_class_ratio"], dtype=np.float64), g["ratio"])
    tail = out["tar_tail_splits"]
    assert len(tail) == tc.NUM_CLASS
    for lst, rows, hists in zip(tail, g["tail_rows"], g["tail_label_hist"]):
        assert [c.n for c in lst] == [int(r) for r in rows[rows >= 0]]
        for c, h in zip(lst, hists):
            r = c.rows.cpu().numpy()
            assert np.array_equal(np.bincount(r[:, 3].astype(np.int64), minlength=256), h)
    dbg = out["debug"]
    cub = dbg["cub"].cpu().numpy().astype(np.int64)
    nt = t_xyz.shape[0]
    assert np.array_equal(cub[:nt], np_cuboid_ids(t_xyz, dbg["centre"][0], dbg["planes"][0]))
    assert np.array_equal(cub[nt:], np_cuboid_ids(s_xyz, dbg["centre"][1], dbg["planes"][1]))
    assert np.array_equal(dbg["stats"][0], g["stats"][0]) and np.array_equal(dbg["stats"][1], g["stats"][1])     # counts, histograms, sums
    assert np.array_equal(dbg["bounds"], g["bounds"])
    got = out["xyz_mid"].cpu().numpy().astype(np.float64)
    ref32 = g["xyz"].astype(np.float64)
    ref64 = ref32 - g["dev"].astype(np.float64)
    E, ref_dev = float(g["E"]), float(g["ref_dev"])
    tol = 4 * U * E
    e64 = float(np.abs(got - ref64).max()) if n else 0.0
    e32 = float(np.abs(got - ref32).max()) if n else 0.0
    print("case %d: |device - fp64 run| %.3g (bound %.3g), |device - fp32 run| %.3g (bound %.3g), ref_dev %.3g" % (
        i, e64, tol, e32, tol + ref_dev, ref_dev))
    assert e64 <= tol, (e64, tol)
    assert e32 <= tol + ref_dev, (e32, tol + ref_dev)


# ------------------------------------------------------------------------------------------------ batching, repeatability
def _filled_sampler(cfg, seed):
    """A real SplitSampler whose queues hold the tail cuboids of a few scenes (one unmixed pass)."""
    from doda_amd import tacm
    rng = np.random.default_rng(seed)
    t_xyz, t_lab = tc.scene(rng, 7000, True)
    s_xyz, s_lab = tc.scene(rng, 5000, True)
    sampler = tacm.SplitSampler(cfg)
    sampler.init_class_ratio(tc.class_ratio_of(t_lab))
    sampler.update_cfg(cfg)
    for k in range(3):
        out = tacm.mix_batch(_d(t_xyz), _d(t_lab, torch.int32), [0, 7000], _d(s_xyz), _d(s_lab, torch.int32), [0, 5000], cfg, sampler,
                             tacm.SeededDraws(100 + k))
        sampler.update(out["tar_tail_splits"])
    assert sum(q.cur_size for q in sampler.queues) > 0
    return sampler


def test_batch_of_four_equals_four_single_calls_and_repeats_bit_for_bit(native_lib):
    from doda_amd import tacm
    cfg = tacm.TacmConfig(enabled=True, split=[2, 2, 1], p=0.7, mix_ratio=0.5, permute_p=0.7, queue_enabled=True, queue_size=64,
                          num_cuboid=2.0, num_class=2, n_classes=tc.N_CLASSES)
    sampler = _filled_sampler(cfg, 5)
    rng = np.random.default_rng(77)
    ts = [tc.scene(rng, n, True) for n in (6100, 1024, 5000, 7777)]          # (one scene of exactly one chunk)
    ss = [tc.scene(rng, n, True) for n in (5000, 4097, 6000, 3000)]
    cat = lambda parts, k, dt: _d(np.concatenate([p[k] for p in parts]), dt)
    off = lambda parts: [0] + list(np.cumsum([p[0].shape[0] for p in parts]))
    call = lambda: tacm.mix_batch(cat(ts, 0, None), cat(ts, 1, torch.int32), off(ts), cat(ss, 0, None), cat(ss, 1, torch.int32), off(ss),
                                  cfg, sampler, [tacm.SeededDraws(900 + b) for b in range(4)])
    a, b = call(), call()
    for k in ("xyz_mid", "labels", "mask1", "mask2"):
        assert torch.equal(a[k], b[k]), k
    assert a["offsets"] == b["offsets"] and np.array_equal(a["tar_splits_class_ratio"], b["tar_splits_class_ratio"])
    used_queue = 0
    for s in range(4):
        one = tacm.mix_batch(_d(ts[s][0]), _d(ts[s][1], torch.int32), [0, ts[s][0].shape[0]], _d(ss[s][0]), _d(ss[s][1], torch.int32),
                             [0, ss[s][0].shape[0]], cfg, sampler, tacm.SeededDraws(900 + s))
        lo, hi = a["offsets"][s], a["offsets"][s + 1]
        assert one["offsets"] == [0, hi - lo]
        for k in ("xyz_mid", "labels", "mask1", "mask2"):
            assert torch.equal(a[k][lo:hi], one[k]), (s, k)
        mine = a["tar_tail_splits"][s * cfg.num_class:(s + 1) * cfg.num_class]
        assert [[c.n for c in lst] for lst in mine] == [[c.n for c in lst] for lst in one["tar_tail_splits"]]
        for la, lb in zip(mine, one["tar_tail_splits"]):
            for ca, cb in zip(la, lb):
                assert torch.equal(ca.rows, cb.rows) and np.array_equal(ca.sum, cb.sum) and np.array_equal(ca.max, cb.max)
        used_queue += int(np.sum(one["tar_splits_class_ratio"]) > 0)
    assert used_queue > 0          # (the comparison covers cuboids from the queue)


# ------------------------------------------------------------------------------------------------ full size, fp64 restatement
def np_mix_sample(t, s, plan, centre_t, centre_s, planes_t, planes_s, total):
    """One sample in numpy fp64 from the plan's DECISIONS only (which cuboids are kept, where they move, which queue cuboids
    join): membership, compaction order, and every mean recomputed from the points themselves.
    -> (xyz fp64, labels, n target points kept, E = largest |coordinate| at any stage, per-scene cuboid ids)."""
    parts, labs, E, ids_out = [], [], 0.0, []
    for (xyz, lab), centre, planes, tab in ((t, centre_t, planes_t, plan.tab_t), (s, centre_s, planes_s, plan.tab_s)):
        ids = np_cuboid_ids(xyz, centre, planes)
        ids_out.append(ids)
        grp = np.where(ids == 255, total - 1, ids)
        x = (xyz - centre[None]).astype(np.float32).astype(np.float64)
        E = max(E, float(np.abs(x).max()))
        keep = tab[grp, 0] != 0
        y = x.copy()
        for c in np.unique(grp[keep]):
            m = grp == c
            y[m] += tab[c, 1:4]
            E = max(E, float(np.abs(y[m]).max()))
            y[m] -= 0.1 * y[m].mean(0)
        parts.append(y[keep])
        labs.append(lab[keep])
    n_t = parts[0].shape[0]
    for q, it in enumerate(plan.items):
        r = it.rows.cpu().numpy().astype(np.float64)
        y = r[:, :3] + plan.item_tab[q, 1:4]
        E = max(E, float(np.abs(y).max()))
        y -= 0.1 * y.mean(0)
        parts.append(y)
        labs.append(r[:, 3].astype(np.int64))
    xyz = np.concatenate(parts)
    E = max(E, float(np.abs(xyz).max()))
    xyz -= xyz.mean(0)
    return xyz, np.concatenate(labs), n_t, max(E, float(np.abs(xyz).max())), ids_out


@pytest.mark.parametrize("split", [[2, 2, 1], [3, 3, 2]])
def test_full_size_batch_against_fp64_restatement(native_lib, split):
    """4 x (150 k + 150 k) points of doda_amd.scene: cuboid ids, counts, histograms, labels and masks equal to the numpy
    restatement; positions within 4 * 2^-24 * E of it."""
    from doda_amd import tacm
    from doda_amd.scene import make_scene
    B, K = 4, tc.N_CLASSES
    scenes = []
    for k in range(2 * B):
        _, mid, lab = make_scene(4000 + k, 150000, 50)
        lab = np.asarray(lab).astype(np.int64)
        lab[k::97] = 255
        scenes.append((np.ascontiguousarray(mid, dtype=np.float32), lab))
    ts, ss = scenes[:B], scenes[B:]
    cfg = tacm.TacmConfig(enabled=True, split=split, p=0.8, mix_ratio=0.5, permute_p=0.6, queue_enabled=True, queue_size=32,
                          num_cuboid=2.0, num_class=2, n_classes=K)
    sampler = tacm.SplitSampler(cfg)
    sampler.init_class_ratio(tc.class_ratio_of(np.concatenate([t[1] for t in ts])))
    sampler.update_cfg(cfg)
    cat = lambda parts, k, dt: _d(np.concatenate([p[k] for p in parts]), dt)
    off = lambda parts: [0] + [int(v) for v in np.cumsum([p[0].shape[0] for p in parts])]
    args = (cat(ts, 0, None), cat(ts, 1, torch.int32), off(ts), cat(ss, 0, None), cat(ss, 1, torch.int32), off(ss))
    warm = tacm.mix_batch(*args, cfg, sampler, [tacm.SeededDraws(10 + b) for b in range(B)])
    sampler.update([[c for lst in warm["tar_tail_splits"][i::cfg.num_class] for c in lst] for i in range(cfg.num_class)])
    out = tacm.mix_batch(*args, cfg, sampler, [tacm.SeededDraws(20 + b) for b in range(B)], return_debug=True)
    dbg = out["debug"]
    cub = dbg["cub"].cpu().numpy().astype(np.int64)
    total = cfg.total_splits
    toff, soff = off(ts), off(ss)
    got = out["xyz_mid"].cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(B):
        p = dbg["plans"][b]
        xyz, lab, n_t, E, ids = np_mix_sample(ts[b], ss[b], p, dbg["centre"][b], dbg["centre"][B + b], dbg["planes"][b], dbg["planes"][B + b], total)
        assert np.array_equal(cub[toff[b]:toff[b + 1]], ids[0]) and np.array_equal(cub[toff[-1] + soff[b]:toff[-1] + soff[b + 1]], ids[1])
        for seg, (sc, idv) in ((b, (ts[b], ids[0])), (B + b, (ss[b], ids[1]))):
            row = np.where(idv == 255, total, idv)
            bins = np.where((sc[1] >= 0) & (sc[1] < K), sc[1], K)
            x = (sc[0] - dbg["centre"][seg][None]).astype(np.float32).astype(np.float64)
            fx = np.rint(x * tc.FIX).astype(np.int64)
            for r in range(total + 1):
                assert np.array_equal(dbg["stats"][seg, r, 3:], np.bincount(bins[row == r], minlength=K + 1)), (seg, r)
                assert np.array_equal(dbg["stats"][seg, r, :3], fx[row == r].sum(0)), (seg, r)
        lo, hi = out["offsets"][b], out["offsets"][b + 1]
        assert hi - lo == xyz.shape[0]
        assert np.array_equal(out["labels"][lo:hi].cpu().numpy(), lab.astype(np.int32))
        m1 = out["mask1"][lo:hi].cpu().numpy()
        assert np.array_equal(m1, np.arange(hi - lo) < n_t) and np.array_equal(out["mask2"][lo:hi].cpu().numpy(), ~m1)
        err = float(np.abs(got[lo:hi] - xyz).max())
        print("split %s sample %d: %d points, %d queue cuboids, |device - fp64| %.3g, bound %.3g (E %.3g)" % (
            split, b, hi - lo, len(p.items), err, 4 * U * E, E))
        assert err <= 4 * U * E, (err, 4 * U * E)
        worst = max(worst, err)
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------ loader
def _tiny_args(tmp, cfg_file, extra=()):
    from doda_amd import st
    argv = ["--cfg_file", cfg_file, "--output_root", str(tmp), "--scene_cache", str(tmp / "scenes"), "--manual_seed", "3",
            "--synthetic_scenes", "4", "--synthetic_base", "4", "--synthetic_voxels", "5000", "--batch_size", "2"] + list(extra)
    return st.parse_config(argv)


def test_mixed_loader_yields_a_batch_the_collate_accepts(native_lib, tmp_path):
    from doda_amd import tacm
    from doda_amd.collate import collate_device_concat
    from doda_amd.loader import DeviceFeeder, MixedDeviceScenes, prepare_cache
    d = dev()
    _, tp = prepare_cache(4, 5000, 50, 501000, str(tmp_path / "scenes"))
    _, sp = prepare_cache(4, 5000, 50, 1000, str(tmp_path / "scenes"))
    cfg = tacm.TacmConfig(enabled=True, split=[2, 2, 1], p=0.5, mix_ratio=0.5, permute_p=0.5, queue_enabled=True, queue_size=16,
                          num_cuboid=2.0, num_class=2, n_classes=20)
    sampler = tacm.SplitSampler(cfg)
    labs = np.concatenate([np.load(p)["labels"] for p in tp])
    sampler.init_class_ratio(tc.class_ratio_of(labs.astype(np.int64)))
    sampler.update_cfg(cfg)
    ds = MixedDeviceScenes(tp, sp, 4, 50, 7, 2, 0, 1, d, cfg, sampler)
    ds.set_labels([torch.from_numpy(np.load(p)["labels"].astype(np.int32)) for p in tp])        # (still works: the target side)
    seen = 0
    for hb in ds:
        off = hb["offsets"].tolist()
        n = hb["locs_float"].shape[0]
        assert off[0] == 0 and off[-1] == n and hb["mask1"].shape == (n,) and hb["mask1"].dtype == torch.bool
        assert int(hb["mask1"].sum() + hb["mask2"].sum()) == n and not bool((hb["mask1"] & hb["mask2"]).any())
        assert len(hb["tar_tail_splits"]) == 2 * cfg.num_class and len(hb["tar_splits_class_ratio"]) == cfg.num_class
        q = hb["locs32"]
        assert int(q[:, 1:].min()) >= 0 and bool((q[:, 1:].max(0)[0].cpu() < torch.from_numpy(hb["spatial_shape"])).all())
        assert torch.equal(q[:, 0].long(), torch.repeat_interleave(torch.arange(2, device=d), torch.tensor(np.diff(off), device=d)))
        batch = collate_device_concat(hb, d)
        assert batch["mask1"] is hb["mask1"] and batch["tar_tail_splits"] is hb["tar_tail_splits"]
        assert batch["p2v_map"].shape[0] == n and batch["labels"].dtype == torch.int64
        sampler.update([[c for lst in hb["tar_tail_splits"][i::2] for c in lst] for i in range(2)])
        seen += 1
    assert seen == 2
    ds.set_epoch(1)
    got = list(DeviceFeeder(iter(ds), d))                                                       # through the feeder thread
    assert len(got) == 2 and all(b["mask1"].shape[0] == b["locs"].shape[0] for b, _ in got)


def test_unmixed_configuration_is_untouched(native_lib, tmp_path):
    """spconv_st.yaml has no tacm section: the trainer's target loader is a plain DeviceScenes whose first batch is bit-equal,
    key by key, to that of a DeviceScenes built directly with the same arguments and seed."""
    from doda_amd.loader import DeviceScenes, MixedDeviceScenes
    from doda_amd.spconv import functional as Fsp
    from doda_amd.train import Trainer
    args, cfg = _tiny_args(tmp_path, "doda_amd/cfgs/synthetic/spconv_st.yaml")
    tr = Trainer(args, cfg, dev(), 0, 1, log=lambda *_: None)
    try:
        assert not tr.tacm.enabled and tr.split_sampler is None
        dl, sampler = tr._loader("target")
        assert type(dl) is DeviceScenes and not isinstance(dl, MixedDeviceScenes)
        ds = tr._datasets["target"]
        direct = DeviceScenes(ds.paths, ds.length, ds.voxel_scale, ds.seed + 3, 2, 0, 1, dev(), augment=ds.augment, shuffle=True,
                              full_scale0=cfg.DATA_CONFIG.DATA_PROCESSOR.full_scale[0])
        dl.set_epoch(0)
        direct.set_epoch(0)
        a, b = next(iter(dl)), next(iter(direct))
        assert set(a) == set(b) == {"locs32", "locs_float", "labels32", "offsets", "spatial_shape", "id"}
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
            else:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        # and with the tacm config the same trainer class builds the mixed loader
        a2, c2 = _tiny_args(tmp_path, "doda_amd/cfgs/synthetic/spconv_st_tacm.yaml")
        tr2 = Trainer(a2, c2, dev(), 0, 1, log=lambda *_: None)
        try:
            assert tr2.tacm.enabled and isinstance(tr2._loader("target")[0], MixedDeviceScenes)
        finally:
            if tr2.prefetch is not None:
                tr2.prefetch.shutdown()
    finally:
        if tr.prefetch is not None:
            tr.prefetch.shutdown()
        Fsp.set_deferred_wgrad(False)


# ------------------------------------------------------------------------------------------------ end to end
def _run(args, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


def test_st_with_tacm_end_to_end(native_lib, tmp_path):
    """A tiny stage-1 checkpoint, then `python -m doda_amd.st` with spconv_st_tacm.yaml in a child process: exit status 0,
    ckpt/split_sampler.pth with non-empty queues, and a tail_class_ratio that moved (tar_splits_class_ratio was consumed).

    The pseudo-label files are put in place by the test, as a resumed run finds them (generation is skipped while done.txt
    exists): a checkpoint this small labels every target point with class 0 (measured: class_ratio.txt = [1, 0, ..., 0] after 1,
    10 and 15 epochs on 8-16 scenes — its target-domain BatchNorm statistics are untrained), and one class has no tail class
    to queue.  The files hold the target scenes' own labels with 30 % of the points ignored."""
    from doda_amd import pseudo_labels as pl
    from doda_amd import st, tacm
    from doda_amd.loader import prepare_cache
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    tmp, cache = tmp_path, str(tmp_path / "scenes")
    syn = ["--synthetic_scenes", "8", "--synthetic_base", "4", "--synthetic_voxels", "5000", "--batch_size", "2", "--print_freq", "1",
           "--output_root", str(tmp), "--scene_cache", cache, "--manual_seed", "3"]
    _run(["-m", "doda_amd.train", "--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml", "--epochs", "1"] + syn + ["--set", "MODEL.dsnorm", "True"])
    ckpt = tmp / "cfgs" / "synthetic" / "spconv" / "default" / "ckpt" / "train_epoch_1.pth"
    assert ckpt.exists()
    argv = ["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_tacm.yaml", "--weight", str(ckpt), "--epochs", "3", "--preserve_pseudo_labels"] + syn
    args, cfg = st.parse_config(argv)
    _, _, ckpt_dir, pdir = st.run_dirs(args, cfg)
    _, paths = prepare_cache(4, 5000, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_scale, 501000, cache)
    rng = np.random.default_rng(0)
    kept = np.zeros(cfg.COMMON_CLASSES.n_classes, dtype=np.int64)
    for p in paths:
        lab = np.load(p)["labels"].astype(np.int64)
        lab[rng.random(lab.shape[0]) < 0.3] = 255
        assert pl.write_scene_labels(pdir, pl.scene_name(p), lab)
        kept += np.bincount(lab[lab != 255], minlength=kept.shape[0])
    pl.write_summary(pdir, kept)
    assert int((kept > 0).sum()) >= 3
    out = _run(["-m", "doda_amd.st"] + argv)
    assert "pseudo labels: reused" in out and "split sampler: tail classes" in out, out[-3000:]
    args, cfg = st.parse_config(argv)
    _, _, ckpt_dir, pdir = st.run_dirs(args, cfg)
    saved = ckpt_dir / st.SAMPLER_FILE
    assert saved.exists() and (ckpt_dir / "train_epoch_3.pth").exists()
    buf = torch.load(saved, weights_only=False)
    print([l for l in out.splitlines() if "split sampler" in l], np.loadtxt(pdir / "class_ratio.txt"))
    assert sum(q["cur_size"] for q in buf["queues"]) > 0, (np.loadtxt(pdir / "class_ratio.txt"), buf["tail_class_idx"])
    assert all(r is None or (r.dim() == 2 and r.shape[1] == 4 and not r.is_cuda) for q in buf["queues"] for r in q["queue"])
    t = tacm.TacmConfig.from_cfg(cfg)
    fresh = tacm.SplitSampler(t)
    fresh.init_class_ratio(np.loadtxt(pdir / "class_ratio.txt"))
    assert np.array_equal(fresh.tail_class_idx, buf["tail_class_idx"])
    print("tail_class_ratio initial %s after %s" % (fresh.tail_class_ratio, buf["tail_class_ratio"]))
    assert not np.array_equal(fresh.tail_class_ratio, buf["tail_class_ratio"])

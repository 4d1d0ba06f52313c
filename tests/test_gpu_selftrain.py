"""Self-training stage on the MI355X: the pseudo-label kernels of include/doda_selftrain.h against torch / numpy restatements of the
reference (model/unet.py:115-132, util/pseudo_labels_util.py:93-158), the odd-class-count backward of the voxel-level head, and
`python -m doda_amd.st` end to end (tool/st.py) with one and two ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ voxel confidence
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("n_cls", [8, 11, 13, 20, 32])
def test_voxel_confidence_matches_head_pred_and_fp64_softmax(native_lib, n_cls, c, dtype):
    from doda_amd import ops
    d = dev()
    m = 70001                                            # (not a multiple of the 256-thread block)
    g = torch.Generator().manual_seed(n_cls * 100 + c)
    feats = (torch.randn(m, c, generator=g) * 1.2).to(d).to(dtype)
    feats[:64] = feats[64:128]                           # a few duplicated rows
    W = (torch.randn(n_cls, c, generator=g) * 0.35).to(d)
    W[n_cls - 1] = W[0]                                  # two identical classes: exact ties -> the lower index
    b = (torch.randn(n_cls, generator=g) * 0.2).to(d)
    b[n_cls - 1] = b[0]
    pred, conf = ops.voxel_confidence(feats, W, b)
    assert pred.dtype == torch.int32 and conf.dtype == torch.float32 and pred.shape == (m,)
    if c == 16:      # the fused training head's argmax on the same operands: bit for bit
        v2p = torch.stack((torch.ones(m, dtype=torch.int32), torch.arange(m, dtype=torch.int32)), 1).to(d)
        _, hp = ops.head_ce_fwd(feats, W, b, v2p, torch.zeros(m, dtype=torch.int64, device=d), 255)
        assert torch.equal(pred, hp)
    Wr = W.to(dtype).double() if dtype == torch.bfloat16 else W.double()
    z = feats.double() @ Wr.t() + b.double()
    p = torch.softmax(z, 1)
    top2 = z.topk(2, 1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5
    assert torch.equal(pred.long()[clear], z.argmax(1)[clear])
    assert int((pred == n_cls - 1).sum()) == 0           # (class n_cls - 1 always ties with class 0)
    rel = ((conf.double() - p.max(1).values).abs() / p.max(1).values).max()
    assert float(rel) < 2e-6, float(rel)
    assert float(conf.min()) >= 1.0 / n_cls * (1 - 1e-6) and float(conf.max()) <= 1.0


# ------------------------------------------------------------------------------------------------ selection and labels
def _np_ratio_thresholds(cls, conf, n_cls, ratios):
    out = []
    for k in range(n_cls):
        vals = np.sort(conf[cls == k])[::-1]
        n = vals.shape[0]
        out.append(vals[:max(1, int(ratios[k] * n))][-1] if n else 0.0)
    return np.array(out, dtype=np.float32)


def _store(n, n_cls, seed):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_cls, n).astype(np.int32)
    cls[cls == 2] = 3                                    # empty class
    one = np.flatnonzero(cls == 4)
    cls[one[1:]] = 5                                     # a class with one point
    conf = rng.random(n, dtype=np.float32) * np.float32(0.9) + np.float32(0.1)
    q = rng.random(n) < 0.5                              # half of them on a few values: heavy ties
    conf[q] = rng.choice(np.array([1.0, 0.75, 0.5, 0.3, 0.30000001], dtype=np.float32), int(q.sum()))
    return cls, conf.astype(np.float32)


@pytest.mark.parametrize("ratio", [[0.0], [1e-7], [0.3], [1.0], "per_class"])
def test_radix_select_on_device_equals_numpy_sort(native_lib, ratio):
    """>= 2 M points through doda_st_point_store (identity p2v; level 0 counted in the same launch) and doda_st_radix_hist: the
    thresholds are bit-equal to sorted(conf of class c, descending)[max(1, int(r n)) - 1]."""
    from doda_amd import ops
    from doda_amd import pseudo_labels as pl
    d = dev()
    n_cls, n = 13, 2_100_003
    cls, conf = _store(n, n_cls, 3)
    ratios = pl.per_class([0.0, 1e-7, 0.3, 1.0, 0.5, 0.99, 0.3, 0.05, 0.7, 1.0, 0.2, 1e-7, 0.6] if ratio == "per_class" else ratio, n_cls)
    store_cls = torch.full((n + 10,), 200, dtype=torch.uint8, device=d)
    store_conf = torch.full((n + 10,), -1.0, dtype=torch.float32, device=d)
    hist0 = torch.zeros((n_cls, 256), dtype=torch.int64, device=d)
    half = n // 2
    ident = torch.arange(n, dtype=torch.int32, device=d)
    pred_d, conf_d = torch.from_numpy(cls).to(d), torch.from_numpy(conf).to(d)
    ops.st_point_store(pred_d, conf_d, ident[:half].contiguous(), store_cls, store_conf, 0, n_cls, hist0)      # two calls at offsets
    ops.st_point_store(pred_d, conf_d, ident[half:].contiguous(), store_cls, store_conf, half, n_cls, hist0)
    assert int(store_cls[n:].eq(200).sum()) == 10                                                       # nothing past the range
    store_cls, store_conf = store_cls[:n], store_conf[:n]
    assert torch.equal(store_cls.long().cpu(), torch.from_numpy(cls).long()) and torch.equal(store_conf.cpu(), torch.from_numpy(conf))
    keys = conf.view(np.uint32).astype(np.int64)
    want0 = np.stack([np.bincount(keys[cls == k] >> 24, minlength=256) for k in range(n_cls)])
    assert np.array_equal(hist0.cpu().numpy(), want0)

    def level_hist(level, prefix):
        if level == 0:
            return hist0.cpu().numpy()
        return ops.st_radix_hist(store_cls, store_conf, n_cls, level, torch.from_numpy(prefix).to(d)).cpu().numpy()
    got = pl.select_thresholds(want0.sum(1), ratios, level_hist)
    want = _np_ratio_thresholds(cls, conf, n_cls, ratios)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert np.array_equal(ops.st_radix_hist(store_cls, store_conf, n_cls, 0).cpu().numpy(), want0)


@pytest.mark.parametrize("mode", ["global", "ratio"])
def test_labels_and_kept_counts_bit_exact(native_lib, mode):
    """doda_st_label against model/unet.py:127-132 restated in numpy (fp32 confidence > fp64 threshold of its class)."""
    from doda_amd import ops
    from doda_amd import pseudo_labels as pl
    d = dev()
    n_cls, n = 11, 1_000_003
    cls, conf = _store(n, n_cls, 5)
    if mode == "global":
        t64 = np.array(pl.per_class([0.3, 0.5, 0.7, 0.75, 0.9, 0.3, 1.0, 0.0, 0.30000001, 0.6, 0.5], n_cls))
        t32 = pl.global_thresholds(list(t64), n_cls)
    else:
        t32 = _np_ratio_thresholds(cls, conf, n_cls, pl.per_class([0.3], n_cls))
        t64 = t32.astype(np.float64)
    labels, kept = ops.st_label(torch.from_numpy(cls.astype(np.uint8)).to(d), torch.from_numpy(conf).to(d),
                                torch.from_numpy(t32).to(d), 255)
    keep = conf.astype(np.float64) > t64[cls]
    want = np.where(keep, cls, 255).astype(np.uint8)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(kept.cpu().numpy(), np.bincount(cls[keep], minlength=n_cls))


# ------------------------------------------------------------------------------------------------ odd class counts in the head backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_cls,m", [pytest.param(8, None, id="8"), pytest.param(11, None, id="11"), pytest.param(13, None, id="13"),
                                     pytest.param(11, 257, id="11-m257"), pytest.param(13, 100, id="13-m100")])
def test_voxel_head_backward_with_odd_class_counts(native_lib, n_cls, m, dtype):
    """_VoxelHeadCE (doda_head_ce_fwd / _bwd, the dz rows of odd class counts stored element by element) against the fp64 score
    matrix definition, at the tolerances tests/test_gpu_round6.py holds the 20-class head to.  m: the first m voxels of the scene
    and their points only — one voxel past a workgroup of the backward sweep (its column sums then cover a workgroup with a single
    voxel) and less than one workgroup; None: the whole scene."""
    import torch.nn.functional as F
    from doda_amd.model import _VoxelHeadCE
    from doda_amd.scene import make_batch
    d = dev()
    b = make_batch(2, 60000, 51)
    v2p, p2v = b["v2p_map"].to(d), b["p2v_map"].to(d)
    g = torch.Generator().manual_seed(9 + n_cls)
    labels = torch.randint(0, n_cls, b["labels"].shape, generator=g).to(d)
    labels[torch.randperm(labels.numel(), generator=g)[:5000].to(d)] = 255
    if m is not None:      # (the point lists keep their point numbers: labels of points outside the first m voxels are not read)
        v2p = v2p[:m].contiguous()
        labels = torch.where(p2v < m, labels, torch.full_like(labels, 255))
        p2v = p2v.clamp(max=m - 1)
    m = v2p.shape[0]
    feats = (torch.randn(m, 16, generator=g) * 1.5).to(d).to(dtype).requires_grad_(True)
    W = (torch.randn(n_cls, 16, generator=g) * 0.4).to(d).requires_grad_(True)
    bias = (torch.randn(n_cls, generator=g) * 0.2).to(d).requires_grad_(True)
    loss, _ = _VoxelHeadCE.apply(feats, W, bias, v2p, labels, 255)
    loss.backward()
    fd = feats.detach().double().requires_grad_(True)
    Wd = (W.detach().to(dtype).double() if dtype == torch.bfloat16 else W.detach().double()).requires_grad_(True)
    bd_ = bias.detach().double().requires_grad_(True)
    ref = F.cross_entropy(fd[p2v.long()] @ Wd.t() + bd_, labels, ignore_index=255)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref)) < 1e-5 * abs(float(ref))
    rel = lambda a, c: float((a.double() - c).abs().max() / c.abs().max())
    assert rel(feats.grad, fd.grad) < (1e-4 if dtype == torch.float32 else 2.0 ** -7), rel(feats.grad, fd.grad)
    assert rel(bias.grad, bd_.grad) < 1e-4
    assert rel(W.grad, Wd.grad) < (1e-4 if dtype == torch.float32 else 3e-3), rel(W.grad, Wd.grad)


# ------------------------------------------------------------------------------------------------ end to end
SYN = ["--synthetic_scenes", "4", "--synthetic_base", "4", "--synthetic_voxels", "5000", "--batch_size", "2", "--print_freq", "1"]


def _run(args, tmp, timeout=600, env_extra=None):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def stage1(tmp_path_factory):
    """One epoch of `python -m doda_amd.train` (DSNorm on) on tiny synthetic scenes -> (tmp dir, scene cache, checkpoint)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    tmp = tmp_path_factory.mktemp("st")
    cache = str(tmp / "scenes")
    _run(["-m", "doda_amd.train", "--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml", "--epochs", "1", "--output_root", str(tmp),
          "--scene_cache", cache, "--manual_seed", "3"] + SYN + ["--set", "MODEL.dsnorm", "True"], tmp)
    ckpt = tmp / "cfgs" / "synthetic" / "spconv" / "default" / "ckpt" / "train_epoch_1.pth"
    assert ckpt.exists()
    return tmp, cache, str(ckpt)


def _st_argv(tmp, cache, ckpt, mode, tag, extra=(), thres=None):
    sets = ["SELF_TRAIN.global_thres", "True" if mode == "global" else "False"]
    if thres is not None:
        sets += ["SELF_TRAIN.thres", "[%r]" % thres]
    return (["-m", "doda_amd.st", "--cfg_file", "doda_amd/cfgs/synthetic/spconv_st.yaml", "--weight", ckpt, "--epochs", "1",
             "--max_iters", "2", "--output_root", str(tmp), "--scene_cache", cache, "--st_extra_tag", tag, "--manual_seed", "3"]
            + SYN + list(extra) + ["--set"] + sets)


def _torch_scores(cfg, ckpt, paths):
    """Per scene (confidence, argmax, top-2 logit margin) per point the torch way: the model's existing forward (point scores),
    softmax, max."""
    from doda_amd.collate import collate_device
    from doda_amd.dsnorm import DSNorm, set_ds_target
    from doda_amd.loader import SyntheticScenes
    from doda_amd.model import SparseConvNet, voxelize_and_run
    from doda_amd.train import get_ckpt
    d = dev()
    net = DSNorm.convert_dsnorm(SparseConvNet(cfg)).to(d)
    net.load_state_dict(get_ckpt(ckpt)["state_dict"])
    net.eval()
    net.apply(set_ds_target)
    dp = cfg.DATA_CONFIG_TAR.DATA_PROCESSOR
    ds = SyntheticScenes(paths, len(paths), dp.voxel_scale, 0, augment=False)
    confs, preds, margins = [], [], []
    with torch.no_grad():
        for k in range(len(paths)):
            batch = collate_device([ds[k]], d, voxel_mode=dp.voxel_mode, full_scale=dp.full_scale)
            scores = voxelize_and_run(cfg, net, batch, d).float()
            c, a = torch.softmax(scores, 1).max(1)
            top2 = scores.topk(2, 1).values
            confs.append(c.cpu().numpy())
            preds.append(a.cpu().numpy())
            margins.append((top2[:, 0] - top2[:, 1]).cpu().numpy())
    return np.concatenate(confs), np.concatenate(preds), np.concatenate(margins)


@pytest.mark.parametrize("mode", ["ratio", "global"])
def test_st_end_to_end(native_lib, stage1, mode):
    from doda_amd import pseudo_labels as pl
    from doda_amd import st
    from doda_amd.loader import prepare_cache
    tmp, cache, ckpt = stage1
    tag = "st_" + mode
    args, cfg = st.parse_config(_st_argv(tmp, cache, ckpt, mode, tag)[2:])
    n_cls = cfg.COMMON_CLASSES.n_classes
    _, paths = prepare_cache(4, 5000, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_scale, 501000, cache)
    c, a, mg = _torch_scores(cfg, ckpt, paths)
    thres = None
    if mode == "global":      # (a threshold inside this checkpoint's confidence range: some points kept, some not)
        thres = float(np.quantile(c.astype(np.float64), 0.6))
        t = np.array([thres] * n_cls)
    else:
        t = _np_ratio_thresholds(a, c, n_cls, pl.per_class(cfg.SELF_TRAIN.thres_ratio, n_cls)).astype(np.float64)
    w = np.where(c.astype(np.float64) > t[a], a, 255)
    out = _run(_st_argv(tmp, cache, ckpt, mode, tag, ["--preserve_pseudo_labels"], thres), tmp)
    assert "pseudo labels: generated" in out, out[-3000:]
    _, _, ckpt_dir, pdir = st.run_dirs(args, cfg)
    assert (ckpt_dir / "train_epoch_1.pth").exists()
    files = sorted(os.listdir(pdir / "txt"))
    assert files == sorted(pl.scene_name(p) + ".txt" for p in paths)
    assert (pdir / "done.txt").exists() and abs(np.loadtxt(pdir / "class_ratio.txt").sum() - 1.0) < 1e-12
    got = pl.read_scene_labels(pdir, paths)
    gt = [np.load(p)["labels"] for p in paths]
    assert [x.shape for x in got] == [y.shape for y in gt]                      # one line per point
    allg = np.concatenate(got)
    assert (allg == 255).any() and (allg != 255).any()
    ratio = np.bincount(allg[allg != 255], minlength=n_cls) / float((allg != 255).sum())
    assert np.allclose(np.loadtxt(pdir / "class_ratio.txt"), ratio, rtol=0, atol=1e-15)
    # against the torch way, from the same checkpoint
    diff = np.flatnonzero(w != allg)
    assert diff.size <= 1e-3 * allg.size, (diff.size, allg.size)
    near = (np.abs(c[diff] - t[a[diff]]) <= 1e-5) | (mg[diff] <= 1e-5)
    assert near.all(), (diff[~near][:10], c[diff][~near][:10], t)
    # target batches carry the pseudo labels of their base scenes (resident loader and worker loader), not the ground truth
    from doda_amd.spconv import functional as Fsp
    from doda_amd.train import Trainer
    for host in (False, True):
        a2, _ = st.parse_config(_st_argv(tmp, cache, ckpt, mode, tag, ["--host_loader", "--workers", "0"] if host else [])[2:])
        tr = Trainer(a2, cfg, dev(), 0, 1, log=lambda *_: None)
        try:
            assert [pl.scene_name(p) for p in tr.split_paths("target")] == [pl.scene_name(p) for p in paths]
            tr.set_split_labels("target", [torch.from_numpy(x) for x in got])
            dl, sampler = tr._loader("target")
            sampler.set_epoch(0)
            hb = next(iter(dl))
            base = [(i % a2.synthetic_scenes) % len(paths) for i in hb["id"]]
            lab = hb["labels32"].cpu().numpy()
            assert np.array_equal(lab, np.concatenate([got[k] for k in base]))
            assert not np.array_equal(lab, np.concatenate([gt[k] for k in base]))
        finally:      # (Trainer switches the process-wide deferred weight gradients on: later tests expect them off)
            if tr.prefetch is not None:
                tr.prefetch.shutdown()
            Fsp.set_deferred_wgrad(False)
    # a second run (resumed for one more epoch) reuses the files; without --preserve_pseudo_labels the directory goes at the end
    out2 = _run(_st_argv(tmp, cache, ckpt, mode, tag, ["--epochs", "2"], thres), tmp)
    assert "pseudo labels: reused" in out2, out2[-3000:]
    assert not pdir.exists()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_st_two_ranks_on_one_gpu_writes_the_same_labels(native_lib, stage1):
    """Two ranks (gloo, sharing the MI355X; the scenes sharded, the histograms summed over ranks) and one rank: identical label
    files and class_ratio.txt."""
    from doda_amd import st
    tmp, cache, ckpt = stage1
    outs = {}
    for world in (1, 2):
        tag = "st_w%d" % world
        argv = _st_argv(tmp, cache, ckpt, "ratio", tag, ["--preserve_pseudo_labels", "--batch_size", "4"])   # (2 scenes per rank)
        if world == 2:
            argv = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(_free_port()), "-m", "doda_amd.st", "--launcher", "pytorch"] + argv[2:]
        _run(argv, tmp, timeout=900, env_extra={"DODA_DIST_BACKEND": "gloo"})
        args, cfg = st.parse_config(_st_argv(tmp, cache, ckpt, "ratio", tag)[2:])
        outs[world] = st.run_dirs(args, cfg)[3]
    a, b = outs[1], outs[2]
    names = sorted(os.listdir(a / "txt"))
    assert names == sorted(os.listdir(b / "txt")) and len(names) == 4
    for f in names:
        assert (a / "txt" / f).read_bytes() == (b / "txt" / f).read_bytes(), f
    assert (a / "class_ratio.txt").read_bytes() == (b / "class_ratio.txt").read_bytes()

"""Full-cloud evaluation on the GPU: ops.eval_nn (doda_eval_nn) bit for bit against the brute-force ops.knnquery on the cases of
tests/eval_cases.py, ops.eval_score (doda_eval_score) against the voxel-level head, the torch meters and an fp64 cross-entropy,
and `python -m doda_amd.test` end to end against the slow route (brute-force neighbours, torch gather, argmax, torch histograms)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import eval_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _case(name):
    d = dev()
    xyz, ends, new, new_ends, side = ec.case(name)
    return tuple(torch.from_numpy(a).to(d) for a in (xyz, ends, new, new_ends)) + (side,)


def _knn1(xyz, ends, new, new_ends):
    from doda_amd import ops
    m = new.shape[0]
    idx = torch.empty((m, 1), dtype=torch.int32, device=xyz.device)
    d2 = torch.empty((m, 1), dtype=torch.float32, device=xyz.device)
    ops.knnquery(m, 1, xyz, new, ends, new_ends, idx, d2)
    return idx.view(-1), d2.view(-1)


# ------------------------------------------------------------------------------------------------ nearest processed point
@pytest.mark.parametrize("name", ec.CASES)
def test_eval_nn_equals_brute_force_bit_for_bit(native_lib, name):
    from doda_amd import ops
    xyz, ends, new, new_ends, side = _case(name)
    want_i, want_d = _knn1(xyz, ends, new, new_ends)
    for sort_queries in (True, False):
        idx, d2 = ops.eval_nn(xyz, new, ends, new_ends, cell_side=side, sort_queries=sort_queries)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32
        assert torch.equal(idx, want_i), (name, int((idx != want_i).sum()))
        assert torch.equal(d2, want_d), name
    if name in ("ii", "v", "vii"):      # and the numpy restatement of the rule (small cases: it is a [queries, points] matrix)
        np_i, np_d = ec.brute_force_nn(*ec.case(name)[:4])
        assert np.array_equal(idx.cpu().numpy(), np_i) and np.array_equal(d2.cpu().numpy(), np_d)


def test_eval_table_grid_limits(native_lib):
    """Case (vi): a 1 mm cell side is doubled until the grid has at most 2^21 cells; 100 m gives a single cell per scene."""
    from doda_amd import ops
    xyz, ends, _, _, _ = _case("i")
    small, large = ops.eval_table(xyz, ends, 1e-3), ops.eval_table(xyz, ends, 100.0)
    for s in small.scenes:
        cells = s.dims[0] * s.dims[1] * s.dims[2]
        assert (1 << 18) < cells <= (1 << 21) and s.side > 1e-3 and abs(np.log2(s.side / np.float32(1e-3)) % 1.0) < 1e-6
    assert [tuple(s.dims) for s in large.scenes] == [(1, 1, 1)] * 2 and large.cell_start.tolist() == [0, 3001, 6000]
    assert int(small.cell_start[-1]) == 6000 and torch.equal(small.order.long().sort()[0], torch.arange(6000, device=xyz.device))


def test_eval_nn_rejects_a_scene_without_processed_points(native_lib):
    from doda_amd import ops
    from doda_amd._lib import DodaNativeError
    xyz, _, new, _, side = _case("v")
    d = xyz.device
    with pytest.raises(DodaNativeError):
        ops.eval_nn(xyz, new, torch.tensor([0, 1], dtype=torch.int32, device=d), torch.tensor([100, 500], dtype=torch.int32, device=d), cell_side=side)


# ------------------------------------------------------------------------------------------------ scoring
@pytest.fixture(scope="module")
def scored():
    """Case (i) with about 1500 voxels under its 6000 processed points and its nearest-neighbour indices (shared, read only)."""
    from doda_amd import ops
    xyz, ends, new, new_ends, side = _case("i")
    g = torch.Generator().manual_seed(11)
    p2v = torch.randint(0, 1500, (xyz.shape[0],), generator=g).to(torch.int32).to(xyz.device)
    idx, _ = ops.eval_nn(xyz, new, ends, new_ends, cell_side=side)
    return p2v, idx, g


def _labels(m, k, g, device):
    lab = torch.randint(0, k, (m,), generator=g)
    lab[torch.rand(m, generator=g) < 0.05] = 255
    lab[:7] = torch.tensor([k, k + 3, -1, 254, -7, 1 << 40, k])      # out of range: dropped, as ops.seg_meters drops them
    return lab.to(device)


def _torch_hist(preds, labels, k):
    from doda_amd.train import DeviceMeters
    meters = DeviceMeters(k, 255, "cpu")       # (CPU tensors take DeviceMeters' torch fallback)
    meters.update(torch.zeros(()), preds.cpu().long(), labels.cpu())
    return meters.cnt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [20, 11, 8])
def test_eval_score_matches_head_meters_and_fp64_loss(native_lib, scored, k, dtype):
    from doda_amd import ops
    p2v, idx, g = scored
    d = p2v.device
    gg = torch.Generator().manual_seed(100 + k)
    feats = torch.randn(1500, 16, generator=gg).to(d).to(dtype).contiguous()
    W = (torch.randn(k, 16, generator=gg) * 0.5).to(d)
    b = torch.randn(k, generator=gg).to(d)
    labels = _labels(idx.shape[0], k, gg, d)
    hist = torch.zeros(3, k, dtype=torch.int64, device=d)
    out, pred = ops.eval_score(feats, W, b, p2v, idx, labels, 255, hist)
    # the prediction: head_ce_fwd's voxel argmax gathered through p2v[idx]
    v2p = torch.zeros((1500, 2), dtype=torch.int32, device=d)
    _, vox_pred = ops.head_ce_fwd(feats, W, b, v2p, labels, 255)
    vox = p2v.long()[idx.long()]
    assert pred.dtype == torch.uint8 and torch.equal(pred.long(), vox_pred.long()[vox])
    # the histograms: DeviceMeters' torch fallback fed those predictions
    assert torch.equal(hist.cpu(), _torch_hist(pred, labels, k))
    # the loss: fp64 cross-entropy on the gathered rows, the weights rounded as the kernels round them
    Wr = W.to(dtype).double() if dtype == torch.bfloat16 else W.double()
    rows = (feats.double() @ Wr.t() + b.double())[vox]
    valid = (labels != 255) & (labels >= 0) & (labels < k)
    want = F.cross_entropy(rows, torch.where(valid, labels, 255), ignore_index=255, reduction="sum")
    print("eval_score k=%d %s: loss sum %.9g against fp64 %.9g, valid %d" % (k, dtype, float(out[0]), float(want), int(out[1])))
    assert int(out[1]) == int(valid.sum()) and out.dtype == torch.float64
    assert abs(float(out[0]) - float(want)) <= 1e-5 * abs(float(want))
    # the same bits on a second run
    hist2 = torch.zeros_like(hist)
    out2, pred2 = ops.eval_score(feats, W, b, p2v, idx, labels, 255, hist2)
    assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(hist, hist2) and torch.equal(pred, pred2)
    # everything ignored: loss 0, counts 0, no NaN; the histograms are ADDED to
    out3, _ = ops.eval_score(feats, W, b, p2v, idx, torch.full_like(labels, 255), 255, hist2, want_pred=False)
    assert out3.tolist() == [0.0, 0.0] and torch.equal(hist, hist2)
    ops.eval_score(feats, W, b, p2v, idx, labels, 255, hist2)
    assert torch.equal(hist2, 2 * hist)
    # idx = NULL on a plain batch: ops.seg_meters over the voxel predictions and p2v
    plain = labels[:p2v.shape[0]].contiguous()
    h_id = torch.zeros_like(hist)
    _, pred_id = ops.eval_score(feats, W, b, p2v, None, plain, 255, h_id)
    h_sm = ops.seg_meters(torch.zeros_like(hist), vox_pred, plain, k, 255, p2v=p2v)
    assert torch.equal(h_id, h_sm) and torch.equal(pred_id.long(), vox_pred.long()[p2v.long()])


def test_eval_score_32_channels(native_lib, scored):
    """The 32-channel head (`mid_channel: 16 # or 32`): the prediction is voxel_confidence's."""
    from doda_amd import ops
    p2v, idx, _ = scored
    d = p2v.device
    gg = torch.Generator().manual_seed(5)
    feats = torch.randn(1500, 32, generator=gg).to(d).to(torch.bfloat16).contiguous()
    W, b = torch.randn(13, 32, generator=gg).to(d), torch.randn(13, generator=gg).to(d)
    labels = _labels(idx.shape[0], 13, gg, d)
    hist = torch.zeros(3, 13, dtype=torch.int64, device=d)
    _, pred = ops.eval_score(feats, W, b, p2v, idx, labels, 255, hist)
    vox_pred, _ = ops.voxel_confidence(feats, W, b)
    assert torch.equal(pred.long(), vox_pred.long()[p2v.long()[idx.long()]]) and torch.equal(hist.cpu(), _torch_hist(pred, labels, 13))


# ------------------------------------------------------------------------------------------------ end to end
SYN = ["--synthetic_scenes", "4", "--synthetic_voxels", "6000"]


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A seeded random-init network of spconv.yaml saved with save_params -> (tmp dir, scene cache, checkpoint path)."""
    from doda_amd import test as dt
    from doda_amd.model import SparseConvNet
    from doda_amd.train import save_params
    dev()
    tmp = tmp_path_factory.mktemp("eval")
    _, cfg = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml"])
    torch.manual_seed(7)
    net = SparseConvNet(cfg)
    with torch.no_grad():
        net.linear.weight.mul_(4.0)      # (spread the logits: a head at its init scale predicts nearly one class)
    save_params(str(tmp / "model_epoch_3.pth"), net, torch.optim.SGD(net.parameters(), lr=0.1), 3)
    return tmp, str(tmp / "scenes"), str(tmp / "model_epoch_3.pth")


def _main(checkpoint, cfg_name, tag, batch_size, extra=()):
    from doda_amd import test as dt
    tmp, cache, ckpt = checkpoint
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        res = dt.main(["--cfg_file", "doda_amd/cfgs/synthetic/%s.yaml" % cfg_name, "--ckpt", ckpt, "--output_root", str(tmp), "--scene_cache",
                       cache, "--eval_tag", tag, "--batch_size", str(batch_size)] + SYN + list(extra))
    finally:
        os.chdir(cwd)
    out = tmp / "cfgs" / "synthetic" / cfg_name / "default" / "eval" / "epoch_3" / "val" / tag
    on_disk = json.loads((out / "result.json").read_text())
    assert on_disk == json.loads(json.dumps(res))
    return on_disk, out


def _network(cfg, ckpt):
    from doda_amd.model import SparseConvNet
    from doda_amd.train import get_ckpt
    net = SparseConvNet(cfg).to(dev())
    net.load_state_dict(get_ckpt(ckpt)["state_dict"])
    return net.eval()


def test_entry_point_scores_full_clouds_like_the_slow_route(native_lib, checkpoint):
    from doda_amd import test as dt
    from doda_amd.collate import collate_device
    from doda_amd.loader import EvalScenes, prepare_cache
    from doda_amd.model import sparse_input
    from doda_amd.train import DeviceMeters
    tmp, cache, ckpt = checkpoint
    res, out = _main(checkpoint, "spconv_eval_ds", "ds_b2", 2, ["--save_to_file"])
    # the slow route: trunk on the subsample, brute-force neighbours, torch gather of fp64 voxel logits, argmax, torch histograms
    args, cfg = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_eval_ds.yaml"] + SYN)
    d = dev()
    net = _network(cfg, ckpt)
    dp = cfg.DATA_CONFIG_TAR.DATA_PROCESSOR
    _, paths = prepare_cache(4, 6000, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_scale, 901000, cache)
    src = EvalScenes(paths, dp.voxel_scale, dp.downsampling_scale, seed=args.manual_seed)
    meters = DeviceMeters(20, 255, "cpu")
    n_valid = 0
    with torch.no_grad():
        for k in range(4):
            batch = collate_device([src[k]], d, voxel_mode=dp.voxel_mode, full_scale=dp.full_scale)
            assert batch["offsets_all"][-1] > 3 * batch["offsets"][-1]
            inp, p2v, _ = sparse_input(cfg, net, batch, d, torch.float32, inputs_ready=True)
            feats = net._trunk(inp).features
            z = feats.double() @ net.linear.weight.double().t() + net.linear.bias.double()
            top2 = z.topk(2, 1).values
            # an fp32 chain of 16 fused multiply-adds is within 17 * 2^-24 * sum |w f| of these fp64 logits: with a wider margin
            # the fp32 argmax is this one
            bound = 17 * 2.0 ** -24 * (feats.double().abs() @ net.linear.weight.double().abs().t() + net.linear.bias.double().abs()).max(1).values
            assert bool(((top2[:, 0] - top2[:, 1]) > 2 * bound).all())
            idx, _ = _knn1(batch["locs_float"], batch["offsets"][1:].to(d), batch["locs_float_all"], batch["offsets_all"][1:].to(d))
            preds = z.argmax(1)[p2v.long()][idx.long()]
            labels = batch["labels_all"]
            meters.update(torch.zeros(()), preds.cpu(), labels.cpu())
            n_valid += int(((labels != 255) & (labels >= 0) & (labels < 20)).sum())
            txt = out / "val_0" / "txt" / (os.path.basename(paths[k]).split(".")[0] + ".txt")
            written = np.loadtxt(txt, dtype=np.int64)
            assert written.shape[0] == labels.shape[0] and np.array_equal(written, preds.cpu().numpy())
    cnt = meters.cnt.numpy()
    assert res["intersection"] == cnt[0].tolist() and res["target"] == cnt[2].tolist()
    assert res["union"] == (cnt[1] + cnt[2] - cnt[0]).tolist()
    assert sum(res["target"]) == n_valid and len(set(np.nonzero(cnt[1])[0])) > 1
    assert np.isfinite(res["loss"]) and res["loss"] > 0 and 0.0 <= res["mIoU"] <= 1.0
    assert len(list(out.glob("log_eval_*.txt"))) == 1 and "Val result: mIoU/mAcc/allAcc" in next(out.glob("log_eval_*.txt")).read_text()
    # batching does not change a count
    for bs in (1, 4):
        other, _ = _main(checkpoint, "spconv_eval_ds", "ds_b%d" % bs, bs)
        assert all(other[key] == res[key] for key in ("intersection", "union", "target"))


def test_entry_point_without_downsampling_equals_the_validation_computation(native_lib, checkpoint):
    from doda_amd import test as dt
    from doda_amd.collate import collate_device
    from doda_amd.loader import SyntheticScenes, prepare_cache
    from doda_amd.model import voxelize_and_run
    from doda_amd.train import DeviceMeters
    tmp, cache, ckpt = checkpoint
    res, _ = _main(checkpoint, "spconv", "plain_b2", 2)
    _, cfg = dt.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv.yaml"])
    d = dev()
    net = _network(cfg, ckpt)
    dp = cfg.DATA_CONFIG.DATA_PROCESSOR
    _, paths = prepare_cache(4, 6000, dp.voxel_scale, 901000, cache)
    ds = SyntheticScenes(paths, 4, dp.voxel_scale, 0, augment=False)
    meters = DeviceMeters(20, 255, "cpu")
    with torch.no_grad():
        for b0 in (0, 2):      # Trainer.validate_epoch's computation: the point scores' argmax
            batch = collate_device([ds[b0], ds[b0 + 1]], d, voxel_mode=dp.voxel_mode, full_scale=dp.full_scale)
            scores = voxelize_and_run(cfg, net, batch, d, feature_dtype=torch.float32, inputs_ready=True)
            meters.update(torch.zeros(()), scores.argmax(1).cpu(), batch["labels"].cpu())
    cnt = meters.cnt.numpy()
    assert res["intersection"] == cnt[0].tolist() and res["target"] == cnt[2].tolist() and res["union"] == (cnt[1] + cnt[2] - cnt[0]).tolist()

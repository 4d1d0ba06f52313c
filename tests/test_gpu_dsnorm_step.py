"""Domain adaptation against fp64: the DSNorm-converted U-Net over the HIP path must reproduce what the REFERENCE's model/unet.py
and model/dsnorm.py produced over the CPU oracle in fp64 (tests/golden/dsnorm_step_golden.npz, made by
tests/golden/make_dsnorm_golden.py; scenario and seeds in tests/dsnorm_cases.py): one two-pass self-training step whose
gradients sum into one optimizer step, and the eval forward on either domain's running statistics."""
import os

import numpy as np
import pytest
import torch

from tests import dsnorm_cases as C
from tests.test_gpu_unet import BF16_NORM_MEDIAN, BF16_NORM_WORST

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
RUNNING_FP32 = 1e-4                # relative L2 per running vector: 10x below what a 1 % error in a layer's batch statistics leaves
#                                    after momentum 0.1 (1e-3), 250x above the oracle's own fp32 distance (3.9e-7)
BF16_RUNNING_DISTANCE = 2.82e-3    # printed by make_dsnorm_golden.py --bf16-distance (unet.u.u.u.u.u.deconv.0)
RUNNING_BF16 = 4 * BF16_RUNNING_DISTANCE   # the margin the fp32 gradient bound has over its oracle distance: the GPU also stores
#                                            gradients in bf16 and sums in another order


@pytest.fixture(scope="module")
def scenario(native_lib):
    """(golden, the three batches on the device): made once, left unchanged."""
    dev = torch.device("cuda:0")
    step = np.load(os.path.join(GOLDEN, "dsnorm_step_golden.npz"))
    batches = C.batches()
    for k, b in enumerate(batches):
        assert b["locs"].shape[0] == int(step["n_points"][k]) and b["voxel_locs"].shape[0] == int(step["n_voxels"][k])
        assert int(b["voxel_locs"].numpy().astype(np.int64).sum()) == int(step["voxel_checksum"][k])
    on_dev = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    on_dev[1]["labels"] = C.pseudo_labels(batches[1]["labels"]).to(dev)
    return step, on_dev


def _model(step):
    """-> (cfg, the project's DSNorm U-Net on the device with seeded weights and domain statistics)."""
    from doda_amd.dsnorm import DSNorm
    from doda_amd.model import SparseConvNet, default_cfg
    from tests.util import deterministic_init
    cfg = default_cfg()
    net = DSNorm.convert_dsnorm(deterministic_init(SparseConvNet(cfg), seed=0)).to(torch.device("cuda:0"))
    assert C.seed_domains(net) == [str(n) for n in step["layer_names"]]
    return cfg, net


def _equal(a, b):
    return all(torch.equal(a[n], b[n]) for n in a)


@pytest.mark.parametrize("dtype,route", [(torch.float32, "immediate"), (torch.float32, "deferred"), (torch.float32, "trainer"),
                                         (torch.bfloat16, "trainer")], ids=["fp32-immediate", "fp32-deferred", "fp32-trainer", "bf16-trainer"])
def test_two_pass_step(scenario, dtype, route):
    """Source pass on source statistics, target pass on target statistics and pseudo labels, W_SRC / W_TAR, no zero_grad in
    between, through cross_entropy(scores) with the weight gradients immediate / deferred and through Trainer._pass's route
    (the loss from the fused head, deferred).  Bit for bit in every route: the source pass leaves every target vector at its
    seed, the target pass every source vector at its snapshot, every counter is 2.  Against the fp64 golden, fp32: losses
    1e-4, summed-gradient norms 5e-3 for every parameter, the 2048-element sample 8e-3 relative and 2e-2 of the tensor's
    maximum (the bounds of test_gpu_unet.py on this batch size), running vectors RUNNING_FP32 relative L2 per vector; bf16:
    losses 2e-2, BF16_NORM_MEDIAN / BF16_NORM_WORST, running vectors RUNNING_BF16.
    Measured on MI355X, the same in all three fp32 routes: losses 1.3e-8 / 3.7e-8; running vectors 2.8e-7 worst
    (unet.u.u.u.u.u.deconv.0.running_mean_target); summed-gradient norms 5.4e-5 median / 1.06e-3 worst (a level-3 BatchNorm
    bias); sample 3.5e-3 relative (unet.u.u.conv.0.bias) / 8.5e-3 of the tensor's maximum.  bf16: losses 1.3e-4 / 1.6e-4; running
    vectors 3.4e-3 worst (the same vector; bound 1.13e-2); summed-gradient norms 1.9e-2 median / 0.217 worst."""
    from doda_amd.dsnorm import set_ds_source, set_ds_target
    from doda_amd.model import cross_entropy, voxelize_and_run
    from doda_amd.spconv import functional as Fsp
    from tests.golden.make_unet_golden import grad_sample_index
    step, (src, tar, _) = scenario
    dev = torch.device("cuda:0")
    cfg, net = _model(step)
    net.train()
    seed = C.running_vectors(net)
    losses, snap = [], None
    try:
        assert Fsp.set_deferred_wgrad(route != "immediate") == (route != "immediate")
        for batch, setter, weight in ((src, set_ds_source, C.W_SRC), (tar, set_ds_target, C.W_TAR)):
            net.apply(setter)
            if route == "trainer":
                loss = voxelize_and_run(cfg, net, batch, dev, feature_dtype=dtype, labels=batch["labels"], ignore_index=C.IGNORE)
                assert loss.dim() == 0 and net.voxel_pred is not None      # the fused head made the loss: no score matrix
            else:
                loss = cross_entropy(voxelize_and_run(cfg, net, batch, dev, feature_dtype=dtype), batch["labels"], C.IGNORE)
            (loss * weight if weight != 1.0 else loss).backward()
            torch.cuda.synchronize()
            losses.append(float(loss.detach()))
            if snap is None:
                snap = C.running_vectors(net)
    finally:
        Fsp.set_deferred_wgrad(False)
    post = C.running_vectors(net)
    layers = C.dsnorm_layers(net)
    # structure, bit for bit
    assert all(torch.equal(snap[n][2:], seed[n][2:]) for n, _ in layers), "the source pass moved target statistics"
    assert all(torch.equal(post[n][:2], snap[n][:2]) for n, _ in layers), "the target pass moved source statistics"
    assert all(not torch.equal(snap[n][:2], seed[n][:2]) and not torch.equal(post[n][2:], snap[n][2:]) for n, _ in layers)
    assert [int(m.num_batches_tracked) for _, m in layers] == [2] * len(layers) == list(step["num_batches_tracked"])

    fp32 = dtype == torch.float32
    for got, key in zip(losses, ("loss_source", "loss_target")):
        err = abs(got - float(step[key])) / float(step[key])
        print("%s: %.2e relative" % (key, err))
        assert err < (1e-4 if fp32 else 2e-2), (key, got, float(step[key]))
    # running vectors
    off, want = step["running_offsets"], step["running"].astype(np.float64)
    worst = (0.0, "")
    for k, (n, _) in enumerate(layers):
        got, ref = post[n].double().cpu().numpy(), want[:, off[k]:off[k + 1]]
        for row, vec in enumerate(C.VECTORS):
            worst = max(worst, (float(np.linalg.norm(got[row] - ref[row]) / np.linalg.norm(ref[row])), n + "." + vec))
    print("running vectors: worst relative L2 %.2e (%s)" % worst)
    assert worst[0] <= (RUNNING_FP32 if fp32 else RUNNING_BF16), worst
    # summed gradients
    params = dict(net.named_parameters())
    names = [str(n) for n in step["grad_names"]]
    assert sorted(params) == names and all(p.grad is not None for p in params.values())
    errs = sorted((abs(float(params[n].grad.double().norm()) - r) / (r + 1e-30), n) for n, r in zip(names, step["grad_norms"]))
    print("summed gradient norms: median %.2e  worst %.2e (%s)" % (errs[len(errs) // 2][0], *errs[-1]))
    if not fp32:
        assert errs[len(errs) // 2][0] < BF16_NORM_MEDIAN and errs[-1][0] < BF16_NORM_WORST, errs[-3:]
        return
    assert errs[-1][0] < 5e-3, errs[-1]
    goff, vals, amax, count = step["grad_sample_offsets"], step["grad_sample_values"], step["grad_absmax"], int(step["grad_sample_count"])
    worst_el, worst_rel = (0.0, ""), (0.0, "")
    for k, n in enumerate(names):
        p = params[n]
        idx = torch.from_numpy(grad_sample_index(n, p.numel(), count)).to(dev)
        got, ref = p.grad.reshape(-1)[idx].double().cpu().numpy(), vals[goff[k]:goff[k + 1]].astype(np.float64)
        assert got.shape == ref.shape
        worst_el = max(worst_el, (float(np.abs(got - ref).max() / (amax[k] + 1e-30)), n))
        worst_rel = max(worst_rel, (float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30)), n))
    print("gradient sample: worst relative %.2e (%s), worst of the tensor's maximum %.2e (%s)" % (*worst_rel, *worst_el))
    assert worst_rel[0] < 8e-3, worst_rel
    assert worst_el[0] < 2e-2, worst_el


@pytest.mark.parametrize("domain", ["source", "target"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_eval_logits_per_domain(scenario, dtype, domain):
    """eval() under no_grad on the golden's post-step statistics (copied in: no dependence on the step test), one domain set:
    head rows and column sums within 1e-3 (fp32) / 6e-2 (bf16) of the golden's range, and at least 0.1 of the range away from
    the OTHER domain's golden in the median row (the goldens are 0.239 apart).  fp32: the arg-max of every point whose golden
    top-2 margin is at least 2e-3 of the range equals the golden's (the generator asserts that at most 10 % fall below; 3.8 %
    do), and so does the fused head's per-voxel arg-max gathered through p2v_map.
    Measured on MI355X: fp32 head rows 3.5e-7 / 2.0e-7 (source / target), column sums 5.5e-8 / 5.4e-8; bf16 head rows 8.2e-3 /
    4.9e-3, column sums 1.9e-3 / 1.6e-3; the other domain's golden 0.220 / 0.235 away in the median row."""
    from doda_amd.dsnorm import set_ds_source, set_ds_target
    from doda_amd.model import point_predictions, voxelize_and_run
    step, (_, _, batch) = scenario
    dev = torch.device("cuda:0")
    cfg, net = _model(step)
    off, want = step["running_offsets"], torch.from_numpy(step["running"])
    with torch.no_grad():
        for k, (_, m) in enumerate(C.dsnorm_layers(net)):
            for row, vec in enumerate(C.VECTORS):
                getattr(m, vec).copy_(want[row, off[k]:off[k + 1]])
    net.eval()
    net.apply(set_ds_source if domain == "source" else set_ds_target)
    before = C.running_vectors(net)
    with torch.no_grad():
        scores = voxelize_and_run(cfg, net, batch, dev, feature_dtype=dtype).float()
        voxelize_and_run(cfg, net, batch, dev, feature_dtype=dtype, labels=batch["labels"], ignore_index=C.IGNORE)
        assert net.voxel_pred is not None
        voxel_route = point_predictions(net, batch["p2v_map"]).cpu().numpy()
    assert _equal(before, C.running_vectors(net))            # eval moves no statistics
    scores = scores.double().cpu().numpy()
    other = "target" if domain == "source" else "source"
    head, colsum = step["eval_head_" + domain].astype(np.float64), step["eval_colsum_" + domain]
    tol = 1e-3 if dtype == torch.float32 else 6e-2
    e_head = float(np.abs(scores[:C.HEAD_ROWS] - head).max() / np.abs(head).max())
    e_col = float(np.abs(scores.sum(0) - colsum).max() / np.abs(colsum).max())
    away = C.row_distance(scores[:C.HEAD_ROWS], step["eval_head_" + other], float(step["eval_range_" + other]))[0]
    print("head rows %.2e, column sums %.2e of the range; median row %.3f away from the %s golden" % (e_head, e_col, away, other))
    assert e_head < tol and e_col < tol, (e_head, e_col)
    assert away >= 0.1, away
    if dtype == torch.float32:
        sure = step["eval_margin_" + domain] >= C.MARGIN_MIN
        assert sure.mean() >= 0.9
        assert np.array_equal(scores.argmax(1)[sure], step["eval_argmax_" + domain][sure])
        assert np.array_equal(voxel_route[sure], step["eval_argmax_" + domain][sure])


def test_conversion_shares_then_separates(native_lib):
    from doda_amd.dsnorm import DSNorm
    from doda_amd.model import SparseConvNet, default_cfg
    dev = torch.device("cuda:0")
    pairs = (("running_mean_source", "running_mean_target"), ("running_var_source", "running_var_target"))
    net = DSNorm.convert_dsnorm(SparseConvNet(default_cfg()))
    layers = C.dsnorm_layers(net)
    assert len(layers) == 65
    # as in the reference: after the conversion both domains ARE the BatchNorm layer's tensors, with its one counter
    assert all(getattr(m, a) is getattr(m, b) for _, m in layers for a, b in pairs)
    assert all(m.num_batches_tracked.dim() == 0 and "num_batches_tracked_target" not in m._buffers for _, m in layers)
    # the host -> device move copies buffer by buffer: distinct storage, equal values
    net = net.to(dev)
    for _, m in C.dsnorm_layers(net):
        for a, b in pairs:
            assert not C.shares_storage(getattr(m, a), getattr(m, b)) and torch.equal(getattr(m, a), getattr(m, b))
    # A model that is ALREADY on the device keeps sharing: no later .to(dev) copies anything, so a target pass would also move
    # the source statistics.  This is why every entry point (Trainer, whose model validate_epoch and pseudo_labels.generate
    # run, and doda_amd.test) converts on the host and moves afterwards, and why seed_domains replaces a target pair that still
    # shares its storage by clones.
    late = DSNorm.convert_dsnorm(SparseConvNet(default_cfg()).to(dev)).to(dev)
    assert all(C.shares_storage(getattr(m, a), getattr(m, b)) for _, m in C.dsnorm_layers(late) for a, b in pairs)

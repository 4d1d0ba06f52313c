"""The second supported backbone width (`mid_channel: 32`, reference cfgs: `mid_channel: 16 # or 32`) and the reference's
domain-adaptation class counts (8 / 11 / 13) on the HIP path.

End to end: SparseConvNet(default_cfg(mid_channel=32, n_classes=11)) against the reference model's fp64 golden
(tests/golden/unet_golden_m32c11_120k.npz, made by tests/golden/make_unet_golden.py), on the trainer's route (deferred weight
gradients: the coarse plan where it applies) and module by module; the bench-sized step with and without tilebooks; the
width-16 head at 8 / 11 / 13 classes against OracleUNet in fp64; point_predictions() on every head route.

Kernels at the shapes width 32 reaches (levels carry 32 .. 224 channels, concatenations 64 .. 448), each against a direct
fp64 evaluation: BatchNorm at 256 channels (op list) and 320 / 384 / 448 (module path), the weight gradients of levels 1-2,
the gathers of levels 1-7 and the 1x1 skips, a folded BatchNorm prologue at kc 224, and the point-level head at 32 channels.

Tolerances: the fp32 end-to-end bars are those of tests/test_gpu_unet.py where the CPU oracle's own fp32-vs-fp64 distance at
width 32 (make_unet_golden.py docstring: logits 2.1e-6, loss 1.4e-7, gradient norms 1.4e-3 worst) stays below a third of
them; the elementwise gradient sample, where that distance is 1.1e-2 / 4.4e-2 worst, gets 3x those.  Kernel bars: one bf16 rounding of the output (2^-7 of
the largest entry) for bf16 stores, the bars of tests/test_gpu_wgrad_wide.py for weight gradients.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_layers import _pack, _scale_err
from tests.test_gpu_layers import test_batchnorm_ops_vs_torch as _batchnorm_ops_vs_torch
from tests.test_gpu_unet import BF16_NORM_MEDIAN, BF16_NORM_WORST
from tests.test_gpu_wgrad_wide import check as _check_dw
from tests.test_gpu_wgrad_wide import ref_dw as _ref_dw

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
GOLD = os.path.join(G, "unet_golden_m32c11.npz")
GOLD_120K = os.path.join(G, "unet_golden_m32c11_120k.npz")
WIDE = dict(mid_channel=32, n_classes=11)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


class _Route:
    """"default": the trainer's configuration (deferred weight gradients + direct gradients: the coarse plan runs where it
    applies); "off": set_coarse_mode("off"), immediate weight gradients."""

    def __init__(self, route):
        self.route = route

    def __enter__(self):
        from doda_amd import model as M
        from doda_amd.spconv import functional as Fsp
        self.old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
        if self.route == "off":
            M.set_coarse_mode("off")
        else:
            M.set_coarse_mode("layers", 1)
            assert Fsp.set_deferred_wgrad(True)
        return self

    def __exit__(self, *exc):
        from doda_amd import model as M
        from doda_amd.spconv import functional as Fsp
        Fsp.set_deferred_wgrad(False)
        M.set_coarse_mode(*self.old)
        return False


def _run(dtype, route, gold=GOLD_120K, voxels=60000):
    from doda_amd.model import SparseConvNet, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from tests.util import deterministic_init
    g = np.load(gold)
    assert int(g["mid_channel"]) == 32 and int(g["n_classes"]) == 11
    batch = make_batch(2, voxels, 4242)
    assert batch["locs"].shape[0] == int(g["n_points"]) and batch["voxel_locs"].shape[0] == int(g["n_voxels"])
    assert int(batch["voxel_locs"].numpy().astype(np.int64).sum()) == int(g["voxel_checksum"])
    d = dev()
    cfg = default_cfg(**WIDE)
    net = deterministic_init(SparseConvNet(cfg), seed=0).to(d).train()
    with _Route(route):
        net.zero_grad(set_to_none=True)
        scores = voxelize_and_run(cfg, net, batch, d, feature_dtype=dtype).float()
        loss = torch.nn.functional.cross_entropy(scores, batch["labels"].to(d), ignore_index=255)
        loss.backward()
        torch.cuda.synchronize()
    grads = {k: float(p.grad.double().norm()) for k, p in net.named_parameters()}
    return g, scores.detach().cpu().double().numpy(), float(loss.detach()), grads, net


@pytest.mark.parametrize("route", ["default", "off"])
def test_wide_unet_fp32_matches_reference_golden_120k(native_lib, route):
    """fp32 logits, loss, every gradient norm and an elementwise sample of every gradient against the reference model's
    fp64 golden at width 32 / 11 classes (2 x 60k voxels), with the bars of the width-16 test
    (tests/test_gpu_unet.py::test_unet_fp32_gradients_match_reference_model_golden_120k).  Measured on MI355X, both routes:
    gradient norms 4.0e-5 median / 5.3e-4 worst, the sample's relative distance 4.0e-3 worst, its largest deviation 1.3e-2.
    Before the coarse plan had a channel bound, the default route raised here (doda_layers_run: a 320-channel BatchNorm)."""
    g, scores, loss, grads, net = _run(torch.float32, route)
    scale = np.abs(g["scores_head"]).max()
    assert np.abs(scores[:4096] - g["scores_head"]).max() / scale < 1e-3
    assert np.abs(scores.sum(0) - g["scores_colsum"]).max() / np.abs(g["scores_colsum"]).max() < 1e-3
    assert abs(loss - float(g["loss"])) / float(g["loss"]) < 1e-4
    assert set(grads) == {str(n) for n in g["grad_names"]}
    errs = sorted((abs(grads[str(n)] - r) / (r + 1e-30), str(n)) for n, r in zip(g["grad_names"], g["grad_norms"]))
    print("fp32 %s: gradient norms vs golden median %.2e worst %.2e (%s)" % (route, errs[len(errs) // 2][0], *errs[-1]))
    assert errs[-1][0] < 5e-3, errs[-3:]
    from tests.golden.make_unet_golden import grad_sample_index
    count = int(g["grad_sample_count"])
    params = dict(net.named_parameters())
    off, vals, amax = g["grad_sample_offsets"], g["grad_sample_values"], g["grad_absmax"]
    worst_el, worst_rel = (0.0, ""), (0.0, "")
    for k, name in enumerate(g["grad_names"]):
        p = params[str(name)]
        idx = torch.from_numpy(grad_sample_index(str(name), p.numel(), count)).to(p.device)
        got = p.grad.reshape(-1)[idx].double().cpu().numpy()
        want = vals[off[k]:off[k + 1]].astype(np.float64)
        assert got.shape == want.shape
        worst_el = max(worst_el, (float(np.abs(got - want).max() / (amax[k] + 1e-30)), str(name)))
        worst_rel = max(worst_rel, (float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30)), str(name)))
    print("fp32 %s: elementwise sample worst relative distance %.2e (%s), worst deviation %.2e (%s)" % (
        route, *worst_rel, *worst_el))
    # (the width-16 bars 8e-3 / 2e-2 are below the CPU oracle's own fp32-vs-fp64 distance at width 32 — 1.1e-2 / 4.4e-2
    # worst, make_unet_golden.py —: 3x those)
    assert worst_rel[0] < 3.3e-2, worst_rel
    assert worst_el[0] < 0.13, worst_el


def test_wide_unet_bf16_gradient_norms_against_the_120k_golden(native_lib):
    """bf16 feature storage on the trainer's route against the same fp64 golden: loss within 2 %, gradient-norm median and
    worst within the width-16 bounds (tests/test_gpu_unet.py BF16_NORM_*).  Measured on MI355X: median 0.026, p90 0.071,
    worst 0.147 (unet.u.u.u.u.blocks.block1.conv_branch.0.weight)."""
    g, scores, loss, grads, net = _run(torch.bfloat16, "default")
    assert abs(loss - float(g["loss"])) / float(g["loss"]) < 2e-2
    errs = sorted((abs(grads[str(n)] - r) / (r + 1e-30), str(n)) for n, r in zip(g["grad_names"], g["grad_norms"]))
    print("bf16 width 32: gradient norms vs golden median %.3f  p90 %.3f  worst %.3f (%s)" % (
        errs[len(errs) // 2][0], errs[int(0.9 * len(errs))][0], errs[-1][0], errs[-1][1]))
    assert errs[len(errs) // 2][0] < BF16_NORM_MEDIAN and errs[-1][0] < BF16_NORM_WORST, errs[-3:]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_unet_eval_forward_routes_agree_with_golden_logits(native_lib, dtype):
    """Evaluation (no gradient): the coarse plan is tried without deferral there.  The default route and the module path
    give the same logits, and the training-mode logits of the 2 x 10k golden come out of the default route."""
    from doda_amd.model import SparseConvNet, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from tests.util import deterministic_init
    g = np.load(GOLD)
    batch = make_batch(2, 10000, 4242)
    assert batch["voxel_locs"].shape[0] == int(g["n_voxels"])
    d = dev()
    cfg = default_cfg(**WIDE)
    net = deterministic_init(SparseConvNet(cfg), seed=0).to(d)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    out = {}
    for route in ("default", "off"):
        net.load_state_dict(state)
        with _Route(route), torch.no_grad():
            net.eval()
            out[route, "eval"] = voxelize_and_run(cfg, net, batch, d, feature_dtype=dtype).float().cpu().double()
            net.train()
            out[route, "train"] = voxelize_and_run(cfg, net, batch, d, feature_dtype=dtype).float().cpu().double()
    tol = 1e-4 if dtype == torch.float32 else 6e-2
    for mode in ("eval", "train"):
        a, b = out["default", mode], out["off", mode]
        assert float((a - b).abs().max() / b.abs().max()) < tol, mode
    scale = np.abs(g["scores_head"]).max()
    err = np.abs(out["default", "train"].numpy()[:4096] - g["scores_head"]).max() / scale
    assert err < (1e-3 if dtype == torch.float32 else 6e-2), err


def _step(cfg, dtype, tiled, bd):
    from doda_amd import spconv
    from doda_amd.model import SparseConvNet, cross_entropy, voxelize_and_run
    from doda_amd.spconv import functional as Fsp
    from tests.util import deterministic_init
    d = dev()
    old = spconv.ops.TILE_KERNEL
    assert Fsp.set_deferred_wgrad(True)
    try:
        spconv.ops.TILE_KERNEL = tiled
        net = deterministic_init(SparseConvNet(cfg), seed=3).to(d).train()
        net.zero_grad(set_to_none=True)
        loss = cross_entropy(voxelize_and_run(cfg, net, bd, d, feature_dtype=dtype), bd["labels"], ignore_index=255)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
        return float(loss.detach()), grads
    finally:
        spconv.ops.TILE_KERNEL = old
        Fsp.set_deferred_wgrad(False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_wide_bench_size_step_tile_path_vs_dense_table_path(native_lib, dtype, monkeypatch):
    """4 x 150k voxels at width 32: the step with tilebooks against the step on dense tables, with the tolerances of
    tests/test_gpu_round4.py::test_config2_size_step_tile_path_vs_dense_table_path."""
    from doda_amd.model import default_cfg
    from doda_amd.scene import make_batch
    import doda_amd.model as dmodel
    d = dev()
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in make_batch(4, 150000, 1000).items()}
    assert bd["voxel_locs"].shape[0] >= 4 * 140000
    if dtype == torch.float32 and dmodel.tile_levels_for(dtype) == 0:
        monkeypatch.setattr(dmodel, "tile_levels_for", lambda dt: 1)
    cfg = default_cfg(**WIDE)
    l0, g0 = _step(cfg, dtype, False, bd)
    l1, g1 = _step(cfg, dtype, True, bd)
    assert np.isfinite(l0) and np.isfinite(l1)
    tol = (2e-2, 0.1) if dtype == torch.bfloat16 else (1e-4, 2e-2)
    assert abs(l0 - l1) < tol[0] * abs(l0), (l0, l1)
    for k, a in g0.items():
        b = g1[k]
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), k
        assert (a.float() - b.float()).norm().item() <= tol[1] * a.float().norm().item() + 1e-6, k


def _oracle_head(k, batch):
    """OracleUNet(mid=16, n_classes=k) in fp64: the trunk forward, then output layer + Linear + CrossEntropyLoss with
    autograd — loss and the output_layer.* / linear.* gradients (they depend on the trunk's output only)."""
    from oracle import oracle as orc
    from oracle import spconv_cpu as sp
    from oracle.unet_cpu import OracleUNet
    from tests.util import deterministic_init
    net = deterministic_init(OracleUNet(mid=16, n_classes=k), seed=0).double().train()
    vf = torch.from_numpy(orc.voxelize_fp(batch["feats"].numpy(), batch["v2p_map"].numpy(), True)).double()
    inp = sp.SparseConvTensor(vf, batch["voxel_locs"].int(), batch["spatial_shape"], batch["offsets"].numel() - 1)
    with torch.no_grad():
        trunk = net.unet(net.input_conv(inp))
    out = net.output_layer(trunk)
    scores = net.linear(out.features[batch["p2v_map"].long()])
    loss = torch.nn.functional.cross_entropy(scores, batch["labels"], ignore_index=255)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()
             if n.startswith(("linear.", "output_layer.")) and p.grad is not None}
    return float(loss), grads


@pytest.mark.parametrize("k", [8, 11, 13])
def test_fused_voxel_head_odd_class_counts_vs_oracle_fp64(native_lib, oracle, k):
    """Width 16 with the reference's domain-adaptation class counts: the fused voxel head (head_ce_fwd / head_ce_bwd, odd
    class counts store dz element by element) — loss and the linear.* / output_layer.* gradients against OracleUNet in fp64
    on the 2 x 10k batch.  Measured on MI355X: 3e-5 relative distance at most (output_layer.0.bias, 11 classes)."""
    from doda_amd.model import SparseConvNet, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from tests.util import deterministic_init
    batch = make_batch(2, 10000, 4242)
    ref_loss, ref_grads = _oracle_head(k, batch)
    d = dev()
    cfg = default_cfg(n_classes=k)
    net = deterministic_init(SparseConvNet(cfg), seed=0).to(d).train()
    loss = voxelize_and_run(cfg, net, batch, d, feature_dtype=torch.float32, labels=batch["labels"].to(d))
    assert getattr(net, "voxel_pred", None) is not None          # the fused voxel head ran
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) / ref_loss < 1e-4, (float(loss), ref_loss)
    params = dict(net.named_parameters())
    assert set(ref_grads) == {"linear.weight", "linear.bias", "output_layer.0.weight", "output_layer.0.bias"}
    for name, ref in ref_grads.items():
        got = params[name].grad.detach().double().cpu()
        assert got.shape == ref.shape
        rel = float((got - ref).norm() / ref.norm())
        print("%d classes: %s relative distance %.2e" % (k, name, rel))
        assert rel < 1e-2, (name, rel)


def _capture_trunk(net):
    """Forward hook on the output layer: the fp64 head inputs of the last call."""
    seen = {}

    def hook(_m, _inp, out):
        seen["feats"] = out.features.detach().double()
    return seen, net.output_layer.register_forward_hook(hook)


def _check_predictions(pred, feats, net, p2v):
    scores = feats[p2v.long()] @ net.linear.weight.detach().double().t() + net.linear.bias.detach().double()
    want = scores.argmax(1)
    top2 = scores.topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]) / scores.abs().max()
    diff = pred.long() != want
    assert pred.shape == want.shape
    assert not bool((diff & (margin > 1e-5)).any()), int(diff.sum())     # (ties to fp32 rounding aside)
    assert int(diff.sum()) <= max(1, want.numel() // 10000)


@pytest.mark.parametrize("route", ["voxel_head", "point_linear", "torch_linear", "unfused"])
def test_point_predictions_follow_the_current_batch(native_lib, route):
    """point_predictions() after a `labels=` call of voxelize_and_run equals the argmax of this batch's scores in fp64 on every
    head route — also after a fused-voxel-head call on another batch (no stale voxel argmax) — and the stored score matrix
    holds no autograd graph."""
    from doda_amd.model import SparseConvNet, default_cfg, point_predictions, voxelize_and_run
    from doda_amd.scene import make_batch
    from tests.util import deterministic_init
    width, n_cls, fused = {"voxel_head": (16, 20, True), "point_linear": (32, 20, True), "torch_linear": (32, 11, True),
                           "unfused": (16, 20, False)}[route]
    d = dev()
    cfg = default_cfg(mid_channel=width, n_classes=n_cls)
    net = deterministic_init(SparseConvNet(cfg), seed=0).to(d).train()
    first, second = make_batch(2, 8000, 5), make_batch(2, 9000, 6)
    if route == "unfused":    # an earlier fused-head call leaves voxel_pred behind
        voxelize_and_run(cfg, net, first, d, labels=first["labels"].to(d)).backward()
        assert net.voxel_pred is not None
    seen, h = _capture_trunk(net)
    try:
        for batch in ((first, second) if route != "unfused" else (second,)):
            loss = voxelize_and_run(cfg, net, batch, d, feature_dtype=torch.float32, fused_head=fused,
                                    labels=batch["labels"].to(d))
            assert (net.voxel_pred is not None) == (route == "voxel_head")
            if route != "voxel_head":
                assert net.point_scores.grad_fn is None and not net.point_scores.requires_grad
            pred = point_predictions(net, batch["p2v_map"].to(d))
            _check_predictions(pred, seen["feats"], net, batch["p2v_map"].to(d))
            loss.backward()
    finally:
        h.remove()


# ---------------------------------------------------------------- kernels at the width-32 shapes

@pytest.fixture(scope="module")
def pyramid():
    """{level: (indices, SubM table, shape)} for levels 1-7 and the k2 s2 child tables: 4 x 150k voxels, Z order"""
    from doda_amd import ops
    from doda_amd.collate import reorder_voxels
    from doda_amd.scene import make_batch
    d = dev()
    b = reorder_voxels(make_batch(4, 150000, 1000, 50), "morton")
    idx = b["voxel_locs"].int().to(d)
    shape = [int(s) for s in b["spatial_shape"]]
    levels, child = {}, {}
    for lvl in range(1, 8):
        levels[lvl] = (idx, ops.rulebook_subm(idx, shape, 4, 3), list(shape))
        if lvl < 7:
            idx, child[lvl], _, shape = ops.rulebook_down2(idx, shape, 4)
    return levels, child


@pytest.mark.parametrize("n", [8400, 40000])
def test_layers_batchnorm_256_channels_two_segments_vs_torch(native_lib, n):
    """STATS -> BNFWD -> BNBWD at c = 256 = 128 + 128 (the level-4 concatenation of width 32: the full LDS channel vectors of
    lay_bn; 40000 rows: the register sweeps of bn.hip) — tests/test_gpu_layers.py::test_batchnorm_ops_vs_torch."""
    _batchnorm_ops_vs_torch(native_lib, n, 128)


@pytest.mark.parametrize("n", [8400, 40000])
def test_layers_batchnorm_256_channels_one_segment_vs_fp64(native_lib, n):
    """The same ops over one 256-channel segment, training forward and backward with an added skip gradient, against
    F.batch_norm + autograd in fp64."""
    from doda_amd import ops
    import torch.nn.functional as F
    d = dev()
    c = 256
    g = torch.Generator().manual_seed(n + 5)
    x = (torch.randn(n, c, generator=g) * 1.5 + 0.3).bfloat16().to(d)
    gamma = (1.0 + 0.1 * torch.randn(c, generator=g)).to(d)
    beta = (0.1 * torch.randn(c, generator=g)).to(d)
    rm, rv = torch.zeros(c, device=d), torch.ones(c, device=d)
    st = ops.stats_totals(c, d)
    mean, invstd = torch.zeros(c, device=d), torch.zeros(c, device=d)
    y = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    assert ops.layers_run([
        dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=c, x_ld=c, x=x, stats=st),
        dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU | ops.CX_F_TRAINING, rows=n, c_in=c, x_ld=c, y_ld=c, c_split=0, eps=1e-4,
             momentum=0.1, x=x, y=y, stats=st, gamma=gamma, beta=beta, mean=mean, invstd=invstd, running_mean=rm, running_var=rv),
    ], d) == 2
    xd = x.double().requires_grad_(True)
    gd, bd_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_ref, rv_ref = torch.zeros(c, dtype=torch.float64, device=d), torch.ones(c, dtype=torch.float64, device=d)
    y_ref = torch.relu(F.batch_norm(xd, rm_ref, rv_ref, gd, bd_, True, 0.1, 1e-4))
    torch.cuda.synchronize()
    assert _scale_err(y, y_ref.detach()) < 2.0 ** -7
    assert torch.allclose(mean.double(), xd.detach().mean(0), rtol=1e-5, atol=1e-5)
    assert torch.allclose(rm.double(), rm_ref, rtol=1e-4, atol=1e-5) and torch.allclose(rv.double(), rv_ref, rtol=1e-4, atol=1e-5)
    dy = torch.randn(n, c, generator=g).bfloat16().to(d)
    add = torch.randn(n, c, generator=g).bfloat16().to(d)
    (y_ref * dy.double()).sum().backward()
    xh = (x.float() - mean) * invstd
    dz = dy.double() * ((xh * gamma + beta) > 0).double()
    sb = ops.stats_totals(c, d)
    sb[0, 0, :, :4] = dz.sum(0).reshape(-1, 4)
    sb[0, 1, :, :4] = (dz * xh.double()).sum(0).reshape(-1, 4)
    dx = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    dg, db = torch.zeros(c, device=d), torch.zeros(c, device=d)
    ops.layers_run([dict(kind=ops.CX_BNBWD, flags=ops.CX_F_RELU, rows=n, c_in=c, x_ld=c, aux_ld=c, res_ld=c, y_ld=c, c_split=0,
                         x=dy, aux=x, res=add, y=dx, stats=sb, mean=mean, invstd=invstd, gamma=gamma, beta=beta, dgamma=dg,
                         dbeta=db)], d)
    torch.cuda.synchronize()
    assert _scale_err(dx, xd.grad + add.double()) < 2.0 ** -6
    assert _scale_err(dg, gd.grad) < 2e-2 and _scale_err(db, bd_.grad) < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c", [320, 384, 448])
def test_module_batchnorm_wider_than_256_vs_fp64(native_lib, dtype, c):
    """The module path's BatchNorm + ReLU (doda_amd.nn.batch_norm_relu) over the concatenations of levels 4-6 at width 32,
    fed the epilogue statistics of the conv that produced them, forward and backward against fp64."""
    from doda_amd import ops
    from doda_amd.nn import batch_norm_relu
    import torch.nn.functional as F
    d = dev()
    n = 3000
    g = torch.Generator().manual_seed(c)
    a = (torch.randn(n, 64, generator=g)).to(dtype).to(d)
    w = (torch.randn(1, 64, c, generator=g) * 0.15).to(d)
    ident = torch.arange(n, dtype=torch.int32, device=d).view(1, n)
    x, st = ops.spconv_gather(a, w, ident, n, 0, c, want_stats="totals")        # 1x1 conv with its epilogue statistics
    bn = torch.nn.BatchNorm1d(c, eps=1e-4, momentum=0.1).to(d).train()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.1 * torch.randn(c, generator=g))
        bn.bias.copy_(0.1 * torch.randn(c, generator=g))
    xg = x.detach().clone().requires_grad_(True)
    y = batch_norm_relu(xg, bn, True, stats=st)
    dy = torch.randn(n, c, generator=g).to(dtype).to(d)
    (y.float() * dy.float()).sum().backward()
    torch.cuda.synchronize()
    xd = x.detach().double().requires_grad_(True)
    gd = bn.weight.detach().double().requires_grad_(True)
    bd_ = bn.bias.detach().double().requires_grad_(True)
    rm, rv = torch.zeros(c, dtype=torch.float64, device=d), torch.ones(c, dtype=torch.float64, device=d)
    y_ref = torch.relu(F.batch_norm(xd, rm, rv, gd, bd_, True, 0.1, 1e-4))
    (y_ref * dy.double()).sum().backward()
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-5
    assert y.dtype == dtype and _scale_err(y, y_ref.detach()) < tol
    assert _scale_err(xg.grad, xd.grad) < (2.0 ** -6 if dtype == torch.bfloat16 else 1e-4)
    assert _scale_err(bn.weight.grad, gd.grad) < (2e-2 if dtype == torch.bfloat16 else 1e-4)
    assert _scale_err(bn.bias.grad, bd_.grad) < (2e-2 if dtype == torch.bfloat16 else 1e-4)
    # running statistics (momentum 0.1 from mean 0 / var 1, unbiased variance)
    var_u = x.double().var(0, unbiased=True)
    assert torch.allclose(bn.running_mean.double(), 0.1 * x.double().mean(0), rtol=1e-3, atol=1e-5)
    assert torch.allclose(bn.running_var.double(), 0.9 + 0.1 * var_u, rtol=1e-3, atol=1e-5)


def _operands(n, ca, cb, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, ca, generator=g).bfloat16().to(dev()), torch.randn(n, cb, generator=g).bfloat16().to(dev()))


def test_wgrad_level1_width32_jobs_vs_fp64(native_lib, pyramid):
    """Level 1 at width 32: the 16 -> 32 (padded input layer), 32 -> 32 and 64 -> 32 (tail) SubM weight gradients over the
    tilebook (wgrad_dma16 at ~600 k rows), every dW entry against fp64, overwrite and accumulate mode."""
    from doda_amd import ops
    levels, _ = pyramid
    _, tbl, _ = levels[1]
    n = tbl.shape[1]
    assert n > 500000
    tb = ops.tilebook_build(tbl)
    for k, (ca, cb) in enumerate([(16, 32), (32, 32), (64, 32)]):
        x, dy = _operands(n, ca, cb, 100 + k)
        ref = _ref_dw(x, dy, tbl)
        got, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, None, tb)])
        _check_dw(got, ref)
        base = torch.randn_like(got)
        acc, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, base.clone(), tb)])
        _check_dw(acc, ref + base.double())
        dense, = ops.spconv_wgrad_multi([(x, dy, tbl, n)])
        _check_dw(dense, ref)


def test_wgrad_level2_width32_wide_jobs_vs_fp64_and_gather_table(native_lib, pyramid):
    """Level 2 at width 32: 64 -> 64 and 128 -> 64 with a tilebook and no pair lists (~150 k rows: the wide kernel's class),
    against fp64 and bit-equal to the gather-table kernel in overwrite and accumulate mode."""
    from doda_amd import ops
    levels, _ = pyramid
    _, tbl, _ = levels[2]
    n = tbl.shape[1]
    assert n > 100000
    tb = ops.tilebook_build(tbl)
    for k, (ca, cb) in enumerate([(64, 64), (128, 64)]):
        x, dy = _operands(n, ca, cb, 110 + k)
        wide, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, None, tb)])
        _check_dw(wide, _ref_dw(x, dy, tbl))
        dense, = ops.spconv_wgrad_multi([(x, dy, tbl, n)])
        assert torch.equal(wide, dense), (ca, cb)
        base = torch.randn_like(wide)
        wide_acc, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, base.clone(), tb)])
        dense_acc, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, base.clone())])
        assert torch.equal(wide_acc, dense_acc), (ca, cb)


def _sample_rows(n, g):
    return torch.cat([torch.randint(0, n, (4000,), generator=g), torch.arange(max(0, n - 300), n),
                      torch.arange(0, min(300, n))]).unique()


def _gather_ref(x, w, tbl, rows, res=None, wq_dtype=torch.bfloat16):
    """fp64 y[rows] = sum_o x[tbl[o][rows]] W[o] (+ res[rows]); W rounded as the pre-pack rounds it."""
    nb = tbl[:, rows].long()
    present = (nb >= 0).unsqueeze(-1)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    xs = torch.where(present, x[nb.clamp_min(0)].double(), zero)
    ref = torch.einsum("orc,ocd->rd", xs, w.to(wq_dtype).double())
    return ref + res[rows].double() if res is not None else ref


def _check_totals(st, y):
    """Epilogue totals against fp64 column sums of the stored rows (bf16 stores: rounding of the stored values aside)."""
    from doda_amd import ops
    s = ops.totals_sums(st)
    yd = y.double()
    n = yd.shape[0]
    slack = (2.0 ** -8 if y.dtype == torch.bfloat16 else 1e-6) * n ** 0.5 * float(yd.abs().max())
    assert float((s[0] - yd.sum(0)).abs().max()) <= slack + 1e-5 * float(yd.sum(0).abs().max())
    s2 = (yd * yd).sum(0)
    assert float(((s[1] - s2).abs() / s2.clamp(min=1e-30)).max()) < (1e-2 if y.dtype == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gather_level1_32_to_32_stats_residual_vs_fp64(native_lib, pyramid, dtype):
    """Level 1 at width 32 (600 k rows): 32 -> 32 with the tilebook (conv_tile mode 1, two channel blocks), residual and
    epilogue totals; fp32 rows with fp32 output.  Sampled rows against fp64, totals against fp64 column sums."""
    from doda_amd import ops
    levels, _ = pyramid
    _, tbl, _ = levels[1]
    n = tbl.shape[1]
    tb = ops.tilebook_build(tbl)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, 32, generator=g).to(dtype).to(dev())
    res = torch.randn(n, 32, generator=g).to(dtype).to(dev())
    w = (torch.randn(27, 32, 32, generator=g) * 0.06).to(dev())
    y, st = ops.spconv_gather(x, w, tbl, n, 0, 32, tilebook=tb, residual=res, want_stats="totals")
    assert y.dtype == dtype
    rows = _sample_rows(n, g).to(dev())
    ref = _gather_ref(x, w, tbl, rows, res, torch.bfloat16 if dtype == torch.bfloat16 else torch.float32)
    err = float((y[rows].double() - ref).abs().max() / ref.abs().max())
    assert err < (2.0 ** -7 if dtype == torch.bfloat16 else 2e-5), err
    _check_totals(st, y)
    if dtype == torch.float32:   # fp32 output of a bf16 gather (the head's form)
        xb = x.bfloat16()
        y32 = ops.spconv_gather(xb, w, tbl, n, 0, 32, out_f32=True)
        assert y32.dtype == torch.float32
        ref = _gather_ref(xb, w, tbl, rows)
        assert float((y32[rows].double() - ref).abs().max() / ref.abs().max()) < 1e-5


@pytest.mark.parametrize("level,ca,cb,tiled", [(1, 64, 32, True), (2, 64, 64, True), (2, 128, 64, True), (5, 160, 160, False),
                                               (6, 192, 192, False), (7, 224, 224, False)])
def test_gather_subm_width32_levels_vs_fp64(native_lib, pyramid, level, ca, cb, tiled):
    """The SubM gathers of width 32 at levels 1-2 (tilebook passed: 64-byte tiles or a fall-through to conv_fast) and 5-7,
    bf16 with epilogue totals, sampled rows against fp64."""
    from doda_amd import ops
    levels, _ = pyramid
    _, tbl, _ = levels[level]
    n = tbl.shape[1]
    g = torch.Generator().manual_seed(level * 1000 + ca)
    x = torch.randn(n, ca, generator=g).bfloat16().to(dev())
    w = (torch.randn(27, ca, cb, generator=g) * (1.5 / (27 * ca)) ** 0.5).to(dev())
    kw = dict(tilebook=ops.tilebook_build(tbl)) if tiled else {}
    y, st = ops.spconv_gather(x, w, tbl, n, 0, cb, want_stats="totals", **kw)
    rows = _sample_rows(n, g).to(dev())
    ref = _gather_ref(x, w, tbl, rows)
    err = float((y[rows].double() - ref).abs().max() / ref.abs().max())
    assert err < 2.0 ** -7, err
    _check_totals(st, y)


@pytest.mark.parametrize("level,ca,cb", [(5, 320, 160), (6, 384, 192)])
def test_gather_1x1_skip_width32_vs_fp64(native_lib, pyramid, level, ca, cb):
    """The 1x1 skip convolutions of the width-32 tail blocks (identity table), every row against fp64."""
    from doda_amd import ops
    levels, _ = pyramid
    n = levels[level][0].shape[0]
    g = torch.Generator().manual_seed(ca)
    x = torch.randn(n, ca, generator=g).bfloat16().to(dev())
    w = (torch.randn(1, ca, cb, generator=g) * (1.5 / ca) ** 0.5).to(dev())
    ident = torch.arange(n, dtype=torch.int32, device=dev()).view(1, n)
    y, st = ops.spconv_gather(x, w, ident, n, 0, cb, want_stats="totals")
    ref = x.double() @ w[0].bfloat16().double()
    assert _scale_err(y, ref) < 2.0 ** -7
    _check_totals(st, y)


def test_folded_batchnorm_prologue_kc224_vs_fp64(native_lib, pyramid):
    """BatchNorm + ReLU folded into the gather of the next SubM conv at kc = 224 (level 7 of width 32: the op list folds
    BNFWD into the GEMM's prologue), the normalised side output and the conv against fp64."""
    from doda_amd import ops
    import torch.nn.functional as F
    levels, _ = pyramid
    d = dev()
    lvl = 5
    _, tbl, _ = levels[lvl]
    n = tbl.shape[1]
    assert n <= 16384
    c, co = 224, 224
    g = torch.Generator().manual_seed(224)
    x = (torch.randn(n, c, generator=g) * 1.3 + 0.2).bfloat16().to(d)
    gamma = (1.0 + 0.1 * torch.randn(c, generator=g)).to(d)
    beta = (0.1 * torch.randn(c, generator=g)).to(d)
    w = (torch.randn(27, c, co, generator=g) * (1.5 / (27 * c)) ** 0.5).to(d)
    wp = _pack(w, 27, c, co, 0, d)
    st = ops.stats_totals(c, d)
    mean, invstd = torch.zeros(c, device=d), torch.zeros(c, device=d)
    xn = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    y = torch.zeros((n, co), dtype=torch.bfloat16, device=d)
    launches = ops.layers_run([
        dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=c, x_ld=c, x=x, stats=st),
        dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU | ops.CX_F_TRAINING, rows=n, c_in=c, x_ld=c, y_ld=c, c_split=0, eps=1e-4,
             momentum=0.1, x=x, y=xn, stats=st, gamma=gamma, beta=beta, mean=mean, invstd=invstd,
             running_mean=torch.zeros(c, device=d), running_var=torch.ones(c, device=d)),
        dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=n, c_in=c, c_out=co, K=27, tbl_ld=n, x_ld=c, y_ld=co, x=xn, w=wp,
             tbl=tbl, y=y, stats=None),
    ], d)
    assert launches == 2, launches                  # STATS + the GEMM with the BatchNorm in its prologue
    torch.cuda.synchronize()
    ref_xn = torch.relu(F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.1, 1e-4))
    assert _scale_err(xn, ref_xn) < 2.0 ** -7
    rows = torch.arange(n, device=d)
    ref = _gather_ref(ref_xn, w, tbl, rows)
    assert _scale_err(y, ref) < 2.0 ** -6


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n_cls", [8, 20])
def test_point_linear_32_channels_vs_fp64(native_lib, dtype, n_cls):
    """_PointLinear (the width-32 head: voxel -> point gather + Linear as one gather-GEMM) forward and backward against fp64."""
    from doda_amd.model import _PointLinear
    from doda_amd.scene import make_batch
    d = dev()
    b = make_batch(2, 10000, 4242)
    p2v, v2p = b["p2v_map"].to(d), b["v2p_map"].to(d)
    v2p_t = v2p[:, 1:].t().contiguous()
    m = v2p.shape[0]
    g = torch.Generator().manual_seed(n_cls)
    feats = torch.randn(m, 32, generator=g).to(dtype).to(d).requires_grad_(True)
    weight = (torch.randn(n_cls, 32, generator=g) * 0.2).to(d).requires_grad_(True)
    bias = (0.1 * torch.randn(n_cls, generator=g)).to(d).requires_grad_(True)
    scores = _PointLinear.apply(feats, weight, bias, p2v, v2p_t)
    ds = torch.randn(scores.shape, generator=g).to(d)
    scores.backward(ds)
    torch.cuda.synchronize()
    wq = weight.detach().to(dtype).double()
    f64 = feats.detach().double()
    ref = f64[p2v.long()] @ wq.t() + bias.detach().double()
    assert scores.dtype == torch.float32
    assert _scale_err(scores, ref) < 1e-5, _scale_err(scores, ref)
    dsq = ds.to(dtype).double()                      # (the gradient operand is stored in the features' dtype)
    ref_df = torch.zeros_like(f64).index_add_(0, p2v.long(), dsq @ wq)
    assert _scale_err(feats.grad, ref_df) < (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5)
    ref_dw = dsq.t() @ f64[p2v.long()]
    assert _scale_err(weight.grad, ref_dw) < (1e-4 if dtype == torch.bfloat16 else 1e-5)
    assert _scale_err(bias.grad, ds.double().sum(0)) < 1e-5

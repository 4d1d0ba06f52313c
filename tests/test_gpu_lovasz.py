"""GPU tests of the voxel-level Lovasz-softmax head (include/doda_loss.h, csrc/lovasz.hip, doda_amd.lovasz._VoxelHeadLovasz) on the
cases of tests/lovasz_cases.py: features, weights and bias are exact in bf16 and their products and sums exact in fp32, so the
case's fp64 logits are the logits the device computes in either type.

Bounds: the loss against doda_amd.lovasz.lovasz_softmax in fp64 on those logits within 4 x the distance the reference's own fp32
code keeps from that fp64 value on the same case (tests/golden/lovasz_golden.npz), floor 2^-22; d_feats, dW, db against torch
autograd of the fp64 restatement through an fp64 Linear within the tolerances of the cross-entropy head's test
(tests/test_gpu_round6.py test_voxel_level_head_and_loss_equals_the_score_matrix_path) for the same three outputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_cases as lc   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lovasz_golden.npz")
_REF = {}


def dev():
    return torch.device("cuda:0")


def _reference(case):
    """fp64, CPU, once per case: (case, loss, d_feats, dW, db) of the restatement through an fp64 Linear."""
    if case not in _REF:
        from doda_amd.lovasz import lovasz_softmax
        c = lc.make_case(case)
        f = torch.from_numpy(c["feats"]).requires_grad_(True)
        w = torch.from_numpy(c["weight"]).requires_grad_(True)
        b = torch.from_numpy(c["bias"]).requires_grad_(True)
        scores = f[torch.from_numpy(c["p2v"])] @ w.t() + b
        assert torch.equal(scores.detach(), torch.from_numpy(c["z"])[torch.from_numpy(c["p2v"])])      # (the sums are exact)
        loss = lovasz_softmax(scores, torch.from_numpy(c["labels"]), lc.IGNORE)
        loss.backward()
        _REF[case] = (c, float(loss.detach()), f.grad.clone(), w.grad.clone(), b.grad.clone())
    return _REF[case]


def _device_run(c, dtype, labels=None):
    from doda_amd.lovasz import _VoxelHeadLovasz
    d = dev()
    feats = torch.from_numpy(c["feats"]).to(d).to(dtype).requires_grad_(True)
    w = torch.from_numpy(c["weight"]).float().to(d).requires_grad_(True)
    b = torch.from_numpy(c["bias"]).float().to(d).requires_grad_(True)
    v2p = torch.from_numpy(c["v2p"]).to(d)
    lab = torch.from_numpy(c["labels"] if labels is None else labels).to(d)
    loss, pred = _VoxelHeadLovasz.apply(feats, w, b, v2p, lab, lc.IGNORE)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), pred, feats.grad.clone(), w.grad.clone(), b.grad.clone(), (feats, w, b, v2p, lab)


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", range(lc.N_CASES))
def test_loss_gradients_pred_and_repeatability(native_lib, case, dtype):
    """Classes 11, 2, 13, 8, 20, 11, 11, 32; every case has a voxel with v2p_ld - 1 points.

    bf16 dW: dz reaches doda_head_dw_bf16 as bf16(dz) plus a second pass over bf16(dz - bf16(dz)); with one pass the one-voxel case
    (case 2) carried the rounding of a single dz value (3.02e-3 against the 3e-3 bound)."""
    from doda_amd import ops
    gold = np.load(GOLD)
    c, ref_loss, ref_df, ref_dw, ref_db = _reference(case)
    assert int(c["v2p"][:, 0].max()) == c["v2p"].shape[1] - 1
    loss, pred, df, dw, db, (feats, w, b, v2p, lab) = _device_run(c, dtype)
    d_loss = abs(float(loss.double()) - ref_loss)
    bound = max(4 * float(gold["dist_loss_%d" % case]), 2.0 ** -22)
    e_df, e_dw, e_db = _rel(df, ref_df), _rel(dw, ref_dw), _rel(db, ref_db)
    print("case %d %s: loss %.9f off by %.3e (bound %.3e); d_feats %.3e dW %.3e db %.3e" % (
        case + 1, dtype, float(loss), d_loss, bound, e_df, e_dw, e_db))
    assert d_loss <= bound
    assert e_df < (1e-4 if dtype == torch.float32 else 2.0 ** -7)
    assert e_db < 1e-4
    assert e_dw < (1e-4 if dtype == torch.float32 else 3e-3)
    # the meters' prediction: the cross-entropy head's, bit for bit
    _, pred_ce = ops.head_ce_fwd(feats.detach(), w.detach(), b.detach(), v2p, lab, lc.IGNORE)
    assert torch.equal(pred, pred_ce)
    # a second call: the same bits
    loss2, pred2, df2, dw2, db2, _ = _device_run(c, dtype)
    assert torch.equal(loss, loss2) and torch.equal(pred, pred2) and torch.equal(df, df2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_voxel_that_fills_its_point_list(native_lib, dtype):
    """Case 4's voxels, with voxel 7 given 40 more points (the widest row of the map: v2p_ld - 1 = its count) of mixed labels, some
    ignored; against the fp64 restatement as above (bounds: the 2^-22 floor; the cross-entropy head's gradient tolerances)."""
    from doda_amd.lovasz import lovasz_softmax
    c = dict(lc.make_case(3))
    n0, extra = c["labels"].shape[0], 40
    rng = np.random.RandomState(5)
    c["p2v"] = np.concatenate([c["p2v"], np.full(extra, 7, dtype=np.int64)])
    c["labels"] = np.concatenate([c["labels"], np.where(rng.rand(extra) < 0.2, lc.IGNORE, rng.randint(0, c["n_cls"], extra))]).astype(np.int64)
    row = c["v2p"][7]
    wide = np.zeros((c["m"], 1 + int(row[0]) + extra), dtype=np.int32)
    wide[:, :c["v2p"].shape[1]] = c["v2p"]
    wide[7, 1 + row[0]:1 + row[0] + extra] = np.arange(n0, n0 + extra)
    wide[7, 0] = row[0] + extra
    c["v2p"] = wide
    assert wide[7, 0] == wide.shape[1] - 1
    f = torch.from_numpy(c["feats"]).requires_grad_(True)
    w = torch.from_numpy(c["weight"]).requires_grad_(True)
    b = torch.from_numpy(c["bias"]).requires_grad_(True)
    ref = lovasz_softmax(f[torch.from_numpy(c["p2v"])] @ w.t() + b, torch.from_numpy(c["labels"]), lc.IGNORE)
    ref.backward()
    loss, _, df, dw, db, _ = _device_run(c, dtype)
    print("wide voxel %s: loss off by %.3e; d_feats %.3e dW %.3e db %.3e" % (
        dtype, abs(float(loss.double()) - float(ref)), _rel(df, f.grad), _rel(dw, w.grad), _rel(db, b.grad)))
    assert abs(float(loss.double()) - float(ref)) <= 2.0 ** -22
    assert _rel(df, f.grad) < (1e-4 if dtype == torch.float32 else 2.0 ** -7)
    assert _rel(db, b.grad) < 1e-4
    assert _rel(dw, w.grad) < (1e-4 if dtype == torch.float32 else 3e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_label_ignored(native_lib, dtype):
    """The stated deviation from the reference (an empty [0, C] tensor there): loss 0, every gradient 0, no NaN."""
    c = lc.make_case(0)
    loss, pred, df, dw, db, _ = _device_run(c, dtype, labels=np.full_like(c["labels"], lc.IGNORE))
    assert float(loss) == 0.0
    for g in (df, dw, db):
        assert float(g.float().abs().max()) == 0.0
    assert int(pred.min()) >= 0 and int(pred.max()) < c["n_cls"]


def test_two_training_steps_with_the_lovasz_config(native_lib, tmp_path, monkeypatch):
    """Trainer on tiny synthetic scenes under cfgs/synthetic/spconv_lovasz.yaml, fp32, two optimizer steps: the voxel-level head
    against the same steps with the fused head off (score matrix + the torch restatement).  First-step loss within 1e-4 relative,
    the bound tests/test_gpu_unet.py puts on its fused and its unfused head against their common golden loss."""
    from doda_amd import model, st
    from doda_amd.spconv import functional as Fsp
    from doda_amd.train import Trainer, adjust_lr
    argv = ["--cfg_file", os.path.join(ROOT, "doda_amd/cfgs/synthetic/spconv_lovasz.yaml"), "--output_root", str(tmp_path),
            "--scene_cache", str(tmp_path / "scenes"), "--manual_seed", "3", "--synthetic_scenes", "4", "--synthetic_base", "4",
            "--synthetic_voxels", "5000", "--batch_size", "2", "--dtype", "f32"]
    losses = {}
    for fused in (True, False):
        monkeypatch.setattr(model, "FUSED_HEAD_LOSS", fused)
        args, cfg = st.parse_config(list(argv))
        assert cfg.OPTIMIZATION.loss == "lovasz"
        torch.manual_seed(11)
        tr = Trainer(args, cfg, dev(), 0, 1, log=lambda *_: None)
        try:
            net = tr.model
            assert net.loss_kind == "lovasz"
            tr.model.train()
            out = []
            for i, (batch, pyramid) in enumerate(tr._batches(0, "train")):
                adjust_lr(cfg.OPTIMIZATION, tr.optimizer, None, 1, 2, 0, i)
                tr.optimizer.zero_grad(set_to_none=True)
                loss, _, _ = tr._pass(batch, pyramid, None)
                assert (net.voxel_pred is not None) == fused
                tr.optimizer.step()
                out.append(float(loss))
                if len(out) == 2:
                    break
            losses[fused] = out
        finally:
            if tr.prefetch is not None:
                tr.prefetch.shutdown()
            Fsp.set_deferred_wgrad(False)
    print("lovasz training losses: fused %s, matrix path %s" % (losses[True], losses[False]))
    assert all(np.isfinite(v) and 0.0 < v <= 1.0 for v in losses[True] + losses[False])
    assert abs(losses[True][0] - losses[False][0]) < 1e-4 * abs(losses[False][0])
    assert losses[True][1] != losses[True][0]

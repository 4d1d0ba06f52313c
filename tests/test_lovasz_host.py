"""CPU tests of OPTIMIZATION.loss: lovasz: the plain-torch restatement (doda_amd.lovasz.lovasz_softmax) against what the reference's
own util/lovasz_loss.py computed (tests/golden/lovasz_golden.npz, made by tests/golden/make_lovasz_golden.py on the inputs of
tests/lovasz_cases.py), its invariances, the config plumbing of SparseConvNet and the companion ABI's version."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_cases as lc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lovasz_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", range(lc.N_CASES))
def test_restatement_against_the_reference(gold, case, dtype):
    """Loss and gradient to the voxel logits within 4 x the reference's recorded own distance from fp64 (its fp32 rounding is the only
    error source on both sides, hence the factor)."""
    from doda_amd.lovasz import lovasz_softmax
    c = lc.make_case(case)
    p2v, labels = torch.from_numpy(c["p2v"]), torch.from_numpy(c["labels"])
    z = torch.from_numpy(c["z"]).to(dtype).requires_grad_(True)
    loss = lovasz_softmax(z[p2v], labels, lc.IGNORE)
    loss.backward()
    assert loss.dtype == dtype
    ref_loss, ref_dz = float(gold["loss_%d" % case]), torch.from_numpy(gold["dz_%d" % case]).double()
    d_loss = abs(float(loss.detach()) - ref_loss)
    d_dz = float((z.grad.double() - ref_dz).norm() / ref_dz.norm())
    print("case %d %s: loss off by %.3e (recorded %.3e), dz by %.3e (recorded %.3e)" % (
        case + 1, dtype, d_loss, float(gold["dist_loss_%d" % case]), d_dz, float(gold["dist_dz_%d" % case])))
    assert d_loss <= 4 * float(gold["dist_loss_%d" % case])
    assert d_dz <= 4 * float(gold["dist_dz_%d" % case])


def test_loss_does_not_depend_on_the_order_of_the_points():
    from doda_amd.lovasz import lovasz_softmax
    c = lc.make_case(0)
    p2v, labels = torch.from_numpy(c["p2v"]), torch.from_numpy(c["labels"])
    scores = torch.from_numpy(c["z"])[p2v]
    a = lovasz_softmax(scores, labels, lc.IGNORE)
    perm = torch.randperm(labels.numel(), generator=torch.Generator().manual_seed(3))
    b = lovasz_softmax(scores[perm], labels[perm], lc.IGNORE)
    assert abs(float(a) - float(b)) < 1e-13      # (fp64: the sums run in another order, tied points swap places)


def test_all_labels_ignored_gives_zero_loss_and_zero_gradients():
    """Deviation from the reference, which returns an empty [0, C] tensor here."""
    from doda_amd.lovasz import lovasz_softmax
    scores = torch.randn(50, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    loss = lovasz_softmax(scores, torch.full((50,), 255, dtype=torch.int64), 255)
    loss.backward()
    assert loss.dim() == 0 and float(loss) == 0.0 and float(scores.grad.abs().max()) == 0.0


def test_absent_classes_are_left_out_of_the_mean():
    """Two classes present out of four: the loss is the mean of THEIR two Lovasz extensions, evaluated here by hand."""
    from doda_amd.lovasz import lovasz_softmax
    g = torch.Generator().manual_seed(5)
    scores = torch.randn(40, 4, dtype=torch.float64, generator=g)
    labels = torch.randint(0, 2, (40,), generator=g) * 2          # classes 0 and 2
    p = torch.softmax(scores, 1)
    per_class = []
    for c in (0, 2):
        fg = (labels == c).double()
        err, order = torch.sort((fg - p[:, c]).abs(), descending=True)
        fs = fg[order]
        G = fs.sum()
        jac = 1 - (G - fs.cumsum(0)) / (G + (1 - fs).cumsum(0))
        per_class.append(float((err * torch.diff(jac, prepend=torch.zeros(1, dtype=torch.float64))).sum()))
    assert abs(float(lovasz_softmax(scores, labels, 255)) - sum(per_class) / 2) < 1e-14


def _cfg(name):
    from doda_amd.config import cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, "doda_amd", "cfgs", "synthetic", name))


def test_config_selects_the_loss():
    from doda_amd import lovasz, model
    cfg = _cfg("spconv_lovasz.yaml")
    assert cfg.OPTIMIZATION.loss == "lovasz" and cfg.OPTIMIZATION.base_lr == _cfg("spconv.yaml").OPTIMIZATION.base_lr
    net = model.SparseConvNet(cfg)
    assert net.loss_kind == "lovasz" and net.criterion is lovasz.lovasz_softmax and net.voxel_head is lovasz._VoxelHeadLovasz
    assert model.criterion_of(net) is lovasz.lovasz_softmax
    # the matrix path's fallback branch (CPU tensors: no native op involved) returns the configured criterion's value
    g = torch.Generator().manual_seed(2)
    scores, labels = torch.randn(30, 20, generator=g), torch.randint(0, 20, (30,), generator=g)
    assert float(net.criterion(scores, labels, 255)) == float(lovasz.lovasz_softmax(scores, labels, 255))


def test_unknown_loss_raises_not_implemented():
    from doda_amd import model
    cfg = _cfg("spconv.yaml")
    cfg.OPTIMIZATION.loss = "focal"
    with pytest.raises(NotImplementedError):
        model.SparseConvNet(cfg)


def test_default_and_cross_entropy_keep_the_parents_objects():
    from doda_amd import model
    plain = _cfg("spconv.yaml")
    assert "loss" not in plain.OPTIMIZATION
    named = _cfg("spconv.yaml")
    named.OPTIMIZATION.loss = "cross_entropy"
    for cfg in (plain, named, model.default_cfg()):
        net = model.SparseConvNet(cfg)
        assert net.loss_kind == "cross_entropy" and net.criterion is model.cross_entropy and net.voxel_head is model._VoxelHeadCE
    assert set(model.SparseConvNet(plain).state_dict()) == set(model.SparseConvNet(_cfg("spconv_lovasz.yaml")).state_dict())


def test_loss_abi_version(native_lib):
    assert native_lib.doda_loss_abi_version() == 1 and native_lib.doda_abi_version() == 13
    assert native_lib.doda_lovasz_workspace_bytes(1000, 11) > 0 and native_lib.doda_lovasz_workspace_bytes(1 << 30, 32) == 0

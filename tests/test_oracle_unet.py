"""The oracle's own U-Net restatement (used for the CPU baseline) against the golden output of the
REFERENCE's model files: same state-dict layout, same logits / loss / gradient norms."""
import json
import os

import numpy as np
import torch

from tests.util import deterministic_init

G = os.path.join(os.path.dirname(__file__), "golden")


def test_oracle_unet_reproduces_reference_golden(native_lib, oracle):
    from doda_amd.scene import make_batch
    from oracle.unet_cpu import OracleUNet, forward_backward
    g = np.load(os.path.join(G, "unet_golden.npz"))
    net = deterministic_init(OracleUNet(), seed=0).double().train()
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert keys == json.load(open(os.path.join(G, "unet_state_keys.json")))
    batch = make_batch(2, 10000, 4242)
    assert int(batch["voxel_locs"].numpy().astype(np.int64).sum()) == int(g["voxel_checksum"])
    scores, loss = forward_backward(net, batch)
    assert np.abs(scores[:4096].detach().numpy() - g["scores_head"]).max() < 1e-5
    assert abs(float(loss) - float(g["loss"])) < 1e-9
    grads = {k: float(p.grad.norm()) for k, p in net.named_parameters()}
    for name, ref in zip(g["grad_names"], g["grad_norms"]):
        assert abs(grads[str(name)] - ref) <= 1e-8 * max(ref, 1.0)


def test_oracle_unet_width32_11_classes_reproduces_reference_golden(native_lib, oracle):
    """The second backbone width and a domain-adaptation class count (reference cfgs: `mid_channel: 16 # or 32`, 8 / 11 / 13
    classes): OracleUNet(mid=32, n_classes=11) in fp64 against tests/golden/unet_golden_m32c11.npz."""
    from doda_amd.scene import make_batch
    from oracle.unet_cpu import OracleUNet, forward_backward
    g = np.load(os.path.join(G, "unet_golden_m32c11.npz"))
    assert int(g["mid_channel"]) == 32 and int(g["n_classes"]) == 11
    net = deterministic_init(OracleUNet(mid=32, n_classes=11), seed=0).double().train()
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert keys == json.load(open(os.path.join(G, "unet_state_keys_m32c11.json")))
    assert keys["linear.weight"] == [11, 32] and keys["unet.u.u.u.u.u.u.blocks.block0.conv_branch.2.weight"][-1] == 224
    batch = make_batch(2, 10000, 4242)
    assert int(batch["voxel_locs"].numpy().astype(np.int64).sum()) == int(g["voxel_checksum"])
    scores, loss = forward_backward(net, batch)
    assert scores.shape[1] == 11
    assert np.abs(scores[:4096].detach().numpy() - g["scores_head"]).max() < 1e-5
    assert abs(float(loss) - float(g["loss"])) < 1e-9
    grads = {k: float(p.grad.norm()) for k, p in net.named_parameters()}
    assert set(grads) == {str(n) for n in g["grad_names"]}
    for name, ref in zip(g["grad_names"], g["grad_norms"]):
        assert abs(grads[str(name)] - ref) <= 1e-8 * max(ref, 1.0)

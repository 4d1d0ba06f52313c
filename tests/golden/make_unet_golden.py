"""Generates tests/golden/unet_golden.npz (+ unet_state_keys.json) and tests/golden/unet_golden_120k.npz.

Run in the BUILD container only (needs /root/reference):
    python tests/golden/make_unet_golden.py            # the 2 x 10k-voxel golden (logits, loss; BASELINE config 1 size)
    python tests/golden/make_unet_golden.py 60000      # the 2 x 60k-voxel golden (gradient norms)
The second supported backbone width and a domain-adaptation class count (configs: `mid_channel: 16 # or 32`, 8 / 11 / 13
classes) -> unet_golden_m32c11.npz (+ unet_state_keys_m32c11.json) and unet_golden_m32c11_120k.npz:
    python tests/golden/make_unet_golden.py --mid-channel 32 --n-classes 11
    python tests/golden/make_unet_golden.py 60000 --mid-channel 32 --n-classes 11 --grad-sample N
--fp32-distance also runs the same reference model in fp32 on the same batch and prints its distance from the fp64 run (the
numbers the GPU tolerances rest on).
Why two: the U-Net's deepest levels shrink the voxel set by ~4.3 per level, so the 20k-voxel batch leaves 5 rows at level 7
and a BatchNorm over 5 rows (1/sqrt(var + 1e-4) up to 100) makes every parameter gradient ill-conditioned — fp32 and fp64
runs of the SAME CPU oracle differ by 14 % (median) there, by 1e-4 (median) / 1.4e-3 (worst) on the 120k-voxel batch.
Gradient parity is therefore asserted on the larger golden, at a tolerance that catches a 1 % error.
At width 32 / 11 classes (--fp32-distance on the 2 x 60k batch) the CPU oracle's fp32 run differs from its fp64 run by:
logits 2.1e-6 of the range, loss 1.4e-7; gradient norms 2.0e-4 median / 1.4e-3 worst (a level-6 BatchNorm bias); the
2048-element gradient sample 6.6e-3 median / 1.1e-2 worst relative distance (unet.u.u.u.u.u.deconv.2.weight), its largest
deviation 5.3e-3 median / 4.4e-2 worst of the tensor's largest entry (a level-6 tail BatchNorm bias).  The 2 x 10k file
stores a 256-element sample and the 120k file a 2048-element one (grad_sample_count), to stay small.

It imports the REFERENCE's own model/unet.py + model/unet_block.py (unmodified, from
/root/reference) on top of the CPU oracle's spconv surface (oracle/spconv_cpu.py), builds the
reference SparseConvNet for cfgs/scannet/spconv.yaml's backbone settings, and records its output
on a seeded synthetic batch: logits, loss, per-parameter gradient norms.  The GPU tests then
require doda_amd.model.SparseConvNet over the HIP path to reproduce these numbers.
Only data is stored (inputs are regenerated from the seed; weights from tests.util.deterministic_init).
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

GOLDEN_SCENES, GOLDEN_VOXELS, GOLDEN_SEED = 2, 10000, 4242
GRAD_SAMPLE = 4096


def grad_sample_index(name, numel, count=GRAD_SAMPLE):
    """Positions of the elementwise gradient sample of parameter `name`: a fixed multiplicative sequence
    through the flattened tensor — reproduced by the test, so only the VALUES are stored.  Small tensors are taken whole.
    count: the sample size (a golden that stores `grad_sample_count` was made with that value; the older ones with 4096)."""
    import zlib
    if numel <= count:
        return np.arange(numel, dtype=np.int64)
    start = zlib.crc32(name.encode()) % numel
    return (start + np.arange(count, dtype=np.int64) * 2654435761) % numel


def import_reference_model():
    from oracle import spconv_cpu
    spconv_cpu.install("spconv")
    # extension modules the reference wrappers import at module scope; the model class itself
    # never calls them (SparseConvNet.forward uses spconv only)
    for name in ("PG_OP", "pointops2_cuda"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import model.unet as ref_unet  # noqa: E402  (the reference's file, imported in place)
    return ref_unet


def golden_batch(voxels=GOLDEN_VOXELS):
    from doda_amd.scene import make_batch
    return make_batch(GOLDEN_SCENES, voxels, GOLDEN_SEED)


def _run_reference(ref_unet, cfg, batch, dtype):
    from oracle import oracle as orc
    from oracle import spconv_cpu
    from tests.util import deterministic_init
    torch.manual_seed(0)
    net = deterministic_init(ref_unet.SparseConvNet(cfg), seed=0).to(dtype)
    net.train()
    vf = orc.voxelize_fp(batch["feats"].numpy(), batch["v2p_map"].numpy(), True)
    inp = spconv_cpu.SparseConvTensor(torch.from_numpy(vf).to(dtype), batch["voxel_locs"].int(),
                                      batch["spatial_shape"], GOLDEN_SCENES)
    scores = net(inp, batch["p2v_map"])
    loss = torch.nn.functional.cross_entropy(scores, batch["labels"], ignore_index=255)
    loss.backward()
    return net, scores, loss


def _fp32_distance(ref_unet, cfg, batch, net64, scores64, loss64, count):
    """The same reference model in fp32 against the fp64 run: the metrics the GPU tests assert."""
    net32, scores32, loss32 = _run_reference(ref_unet, cfg, batch, torch.float32)
    s64, s32 = scores64.detach()[:4096], scores32.detach().double()[:4096]
    p64, p32 = dict(net64.named_parameters()), dict(net32.named_parameters())
    norm_err, rel, el = [], [], []
    for n in sorted(p64):
        g64, g32 = p64[n].grad, p32[n].grad.double()
        norm_err.append((abs(float(g32.norm()) - float(g64.norm())) / (float(g64.norm()) + 1e-30), n))
        idx = torch.from_numpy(grad_sample_index(n, g64.numel(), count))
        a, b = g32.reshape(-1)[idx], g64.reshape(-1)[idx]
        rel.append((float((a - b).norm() / (b.norm() + 1e-30)), n))
        el.append((float((a - b).abs().max() / (g64.abs().max() + 1e-30)), n))
    norm_err.sort()
    rel.sort()
    el.sort()
    print("fp32 vs fp64: logits head %.2e of the range, loss %.2e relative" % (
        float((s32 - s64).abs().max() / s64.abs().max()), abs(float(loss32) - float(loss64)) / float(loss64)))
    print("  gradient norms: median %.2e, worst %.2e (%s)" % (norm_err[len(norm_err) // 2][0], *norm_err[-1]))
    print("  elementwise sample: relative distance median %.2e, worst %.2e (%s)" % (rel[len(rel) // 2][0], *rel[-1]))
    print("  largest deviation / tensor max: median %.2e, worst %.2e (%s)" % (el[len(el) // 2][0], *el[-1]))


def main(voxels=GOLDEN_VOXELS, mid_channel=16, n_classes=20, count=GRAD_SAMPLE, fp32_distance=False):
    from doda_amd.model import default_cfg
    ref_unet = import_reference_model()
    cfg = default_cfg(mid_channel=mid_channel, n_classes=n_classes)
    batch = golden_batch(voxels)
    net, scores, loss = _run_reference(ref_unet, cfg, batch, torch.float64)
    grads = {k: float(p.grad.norm()) for k, p in net.named_parameters()}
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    small = voxels == GOLDEN_VOXELS
    # the default model keeps the original file names; other widths / class counts carry "_m<width>c<classes>"
    tag = "" if (mid_channel, n_classes) == (16, 20) else "_m%dc%d" % (mid_channel, n_classes)
    if small:
        with open(os.path.join(HERE, "unet_state_keys%s.json" % tag), "w") as f:
            json.dump(keys, f, indent=0, sort_keys=True)
    names = sorted(grads)
    params = dict(net.named_parameters())
    # elementwise sample of every parameter gradient (a permuted or sign-flipped block inside a weight gradient keeps its norm)
    sample = [params[n].grad.reshape(-1)[torch.from_numpy(grad_sample_index(n, params[n].numel(), count))].numpy()
              for n in names]
    gs_off = np.cumsum([0] + [len(v) for v in sample]).astype(np.int64)
    extra = {} if count == GRAD_SAMPLE and not tag else dict(grad_sample_count=count, mid_channel=mid_channel,
                                                             n_classes=n_classes)
    np.savez_compressed(
        os.path.join(HERE, ("unet_golden%s.npz" % tag) if small
                     else "unet_golden%s_%dk.npz" % (tag, GOLDEN_SCENES * voxels // 1000)),
        scores_head=scores[:4096].detach().numpy().astype(np.float32),
        scores_colsum=scores.detach().sum(0).numpy(), scores_abssum=float(scores.detach().abs().sum()),
        loss=float(loss), grad_names=np.array(names), grad_norms=np.array([grads[n] for n in names]),
        grad_sample_offsets=gs_off, grad_sample_values=np.concatenate(sample).astype(np.float32),
        grad_absmax=np.array([float(params[n].grad.abs().max()) for n in names]),
        n_points=batch["locs"].shape[0], n_voxels=batch["voxel_locs"].shape[0],
        voxel_checksum=int(batch["voxel_locs"].numpy().astype(np.int64).sum()),
        running_mean_l1=float(net.state_dict()["output_layer.0.running_mean"].abs().sum()), **extra)
    print("golden written: N=%d M=%d loss=%.6f" % (batch["locs"].shape[0], batch["voxel_locs"].shape[0], float(loss)))
    if fp32_distance:
        _fp32_distance(ref_unet, cfg, batch, net, scores, loss, count)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("voxels", nargs="?", type=int, default=GOLDEN_VOXELS, help="target voxels per scene")
    ap.add_argument("--mid-channel", type=int, default=16)
    ap.add_argument("--n-classes", type=int, default=20)
    ap.add_argument("--grad-sample", type=int, default=GRAD_SAMPLE, help="elementwise gradient sample size per parameter")
    ap.add_argument("--fp32-distance", action="store_true")
    a = ap.parse_args()
    main(a.voxels, a.mid_channel, a.n_classes, a.grad_sample, a.fp32_distance)

"""The domain-adaptation scenario of tests/golden/dsnorm_step_golden.npz, shared by its generator
(tests/golden/make_dsnorm_golden.py) and the tests (tests/test_gpu_dsnorm_step.py, tests/test_dsnorm_host.py): a
DSNorm-converted U-Net whose two domains start from DIFFERENT seeded statistics in every layer, one two-pass self-training
step (source pass, then target pass on pseudo labels, gradients summed), then an eval forward per domain.

Order of construction (the generator and the tests follow it): SparseConvNet -> tests.util.deterministic_init (BEFORE the
conversion: it keys on names ending in running_mean / running_var) -> convert_dsnorm -> dtype / device move -> seed_domains.
"""
import zlib

import numpy as np
import torch

W_SRC, W_TAR = 1.0, 0.5                 # loss weights of the two passes (SELF_TRAIN.SRC / TAR.loss_weight)
IGNORE = 255
SOURCE_BATCH = (2, 60000, 4242)         # the batch of unet_golden_120k.npz
TARGET_BATCH = (2, 60000, 4243)
EVAL_BATCH = (1, 10000, 4244)           # a single scene, as pseudo-label generation and evaluation see it
HEAD_ROWS = 4096
MARGIN_UNIT = 1e-3                      # the stored top-2 margins count multiples of this share of the logit range (uint8, saturating)
MARGIN_MIN = 2                          # arg-max is compared where the stored margin is at least MARGIN_MIN * MARGIN_UNIT
VECTORS = ("running_mean_source", "running_var_source", "running_mean_target", "running_var_target")


def domain_stats(name, c):
    """Seeded initial statistics of the DSNorm layer called `name` -> (mean_s, var_s, mean_t, var_t), float64 [c] each.
    The two domains differ in every layer, so the choice of domain is visible in every output."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mean_s = 0.3 * rng.standard_normal(c)
    var_s = 0.5 + rng.random(c)
    mean_t = 0.3 * rng.standard_normal(c)
    var_t = 0.5 + rng.random(c)
    return mean_s, var_s, mean_t, var_t


def dsnorm_layers(net):
    """(name, module) of every module whose class name contains DSNorm (the rule of set_ds_source / set_ds_target), in
    named_modules() order."""
    return [(n, m) for n, m in net.named_modules() if "DSNorm" in type(m).__name__]


def shares_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def seed_domains(net):
    """Give every DSNorm layer its domain_stats.  convert_dsnorm leaves the two domains on the SAME tensors; they part only if a
    later .to() really copies (a device move does, .to(torch.float32) of an fp32 model does not), so a target pair that still
    shares its storage with the source pair is replaced by clones first.  -> the layer names."""
    names = []
    with torch.no_grad():
        for name, m in dsnorm_layers(net):
            for kind in ("running_mean_", "running_var_"):
                if shares_storage(getattr(m, kind + "source"), getattr(m, kind + "target")):
                    setattr(m, kind + "target", getattr(m, kind + "source").clone())
            for key, v in zip(VECTORS, domain_stats(name, m.num_features)):
                buf = getattr(m, key)
                buf.copy_(torch.from_numpy(v).to(buf.dtype))
            names.append(name)
    return names


def running_vectors(net):
    """{layer name: [4, c] clone of VECTORS} of every DSNorm layer."""
    return {n: torch.stack([getattr(m, k).detach().clone() for k in VECTORS]) for n, m in dsnorm_layers(net)}


def batches():
    """(source, target, eval) batch dictionaries (CPU tensors)."""
    from doda_amd.scene import make_batch
    return make_batch(*SOURCE_BATCH), make_batch(*TARGET_BATCH), make_batch(*EVAL_BATCH)


def pseudo_labels(labels):
    """The target pass's labels: 40 % of the points ignored, as a confidence threshold leaves them."""
    drop = np.random.default_rng(7).random(labels.shape[0]) < 0.4
    out = labels.clone()
    out[torch.from_numpy(drop)] = IGNORE
    return out


def logit_range(scores):
    """The scale every logit distance is a share of: the largest magnitude."""
    return float(np.abs(np.asarray(scores)).max())


def top2_margin_units(scores, rng):
    """Top-2 margin of every row in multiples of MARGIN_UNIT * rng, rounded down, saturating at 255 -> uint8."""
    s = np.sort(np.asarray(scores, dtype=np.float64), axis=1)
    return np.minimum(np.floor((s[:, -1] - s[:, -2]) / (MARGIN_UNIT * rng)), 255).astype(np.uint8)


def row_distance(a, b, rng):
    """Median and maximum over rows of the largest logit difference of the row, as a share of rng."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max(1) / rng
    return float(np.median(d)), float(d.max())

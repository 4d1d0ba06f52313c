"""Pseudo labels of the self-training stage (reference util/pseudo_labels_util.py:15-165, model/unet.py:115-132, tool/st.py:345-366).

The reference runs the model over the target training set, gathers every point's softmax confidence into per-class Python lists
(pandas groupby, list.sort), takes a per-class quantile as the threshold and keeps a point's argmax only where its confidence is
above its class threshold.  Here:

  1. voxel level on the device: SparseConvNet.voxel_confidence (doda_st_voxel_confidence) gives each voxel's argmax and its
     largest softmax probability — every point of a voxel has its voxel's logits, so no [points, classes] matrix exists;
  2. doda_st_point_store expands them through p2v into a per-rank store (class uint8, confidence fp32 per point) and counts the
     first radix level of every class in the same launch;
  3. ratio mode: the k-th largest confidence per class, k = max(1, int(r * n)), EXACTLY, by a radix select over the fp32 bit
     patterns (select_thresholds): DODA_ST_RADIX_LEVELS levels of 8 bits, the small int64 histograms read back (and summed over
     ranks: integer sums are exact) between levels; global mode: the float64 thresholds rounded toward -inf to fp32 (a strict
     lower bound that compares the same against every fp32 confidence: global_thresholds);
  4. doda_st_label writes `conf > t[pred] ? pred : ignore_label` and counts the kept points per class;
  5. one `%d` text file per scene, class_ratio.txt and done.txt, as the reference lays them out.
"""
import os

import numpy as np
import torch

RADIX_BITS, RADIX_LEVELS = 8, 4      # include/doda_selftrain.h
BINS = 1 << RADIX_BITS


# ------------------------------------------------------------------------------------------------ thresholds (host)
def per_class(values, n_cls):
    """A config list of length 1 (broadcast) or n_cls -> list of n_cls Python floats (util/pseudo_labels_util.py:129-131,147-149)."""
    values = list(values)
    if len(values) == 1:
        values = values * n_cls
    if len(values) != n_cls:
        raise ValueError("expected 1 or %d per-class values, got %d" % (n_cls, len(values)))
    return [float(v) for v in values]


def ratio_ranks(counts, thres_ratio):
    """1-based rank from the top of each class's threshold: max(1, int(r_c * n_c)) (the product in float64), at most n_c; 0 for
    an empty class (util/pseudo_labels_util.py:132-136: sorted[:k][-1], IndexError -> 0.0)."""
    ratios = per_class(thres_ratio, len(counts))
    ks = []
    for n, r in zip(counts, ratios):
        n = int(n)
        ks.append(0 if n == 0 else min(max(1, int(r * n)), n))
    return ks


def select_thresholds(counts, thres_ratio, level_hist):
    """The ratio-mode thresholds: per class the k-th largest confidence (k = ratio_ranks), exactly, by radix select.

    level_hist(level, prefix) -> int64 [n_cls, 256]: for each class c the histogram of bits [24 - 8 level, 32 - 8 level) of the
    keys (fp32 bit patterns) of class c whose bits above equal prefix[c] (int32 array; -1 = class finished).  Returns float32
    [n_cls] (0.0 for an empty class)."""
    counts = np.asarray(counts, dtype=np.int64)
    n_cls = counts.shape[0]
    k = np.array(ratio_ranks(counts, thres_ratio), dtype=np.int64)
    active = k > 0
    prefix = np.zeros(n_cls, dtype=np.int64)
    for level in range(RADIX_LEVELS):
        hist = np.asarray(level_hist(level, np.where(active, prefix, -1).astype(np.int32)), dtype=np.int64)
        for c in np.nonzero(active)[0]:
            from_top = np.cumsum(hist[c, ::-1])          # points in the bins at and above each bin, from the top bin down
            j = int(np.searchsorted(from_top, k[c]))     # first bin (from the top) whose running count reaches rank k
            if j >= BINS:
                raise RuntimeError("radix select: class %d has %d keys under its prefix, rank %d wanted" % (c, from_top[-1], k[c]))
            b = BINS - 1 - j
            k[c] -= from_top[j] - hist[c, b]            # rank within the chosen bin
            prefix[c] = (prefix[c] << RADIX_BITS) | b
    out = np.zeros(n_cls, dtype=np.float32)
    out[active] = prefix[active].astype(np.uint32).view(np.float32)
    return out


def global_thresholds(thres, n_cls):
    """float64 thresholds (SELF_TRAIN.thres, length 1 or n_cls) -> float32 [n_cls] strict lower bounds: t64 rounded toward -inf,
    so that for every fp32 x, x > t64 exactly when x > t32 (model/unet.py:129 compares fp32 confidences to fp64 thresholds)."""
    t64 = np.array(per_class(thres, n_cls), dtype=np.float64)
    t32 = t64.astype(np.float32)
    over = t32.astype(np.float64) > t64
    t32[over] = np.nextafter(t32[over], np.float32(-np.inf))
    return t32


def class_ratio(kept):
    """Kept points per class over their sum (util/pseudo_labels_util.py:152-158), float64."""
    kept = np.asarray(kept, dtype=np.float64)
    total = kept.sum()
    return kept / total if total > 0 else kept


# ------------------------------------------------------------------------------------------------ files
def scene_name(path):
    """A base scene's name: its file's stem (reference: data_list[idx].split('/')[-1].split('.')[0])."""
    return os.path.basename(str(path)).split(".")[0]


def txt_dir(pseudo_dir):
    return os.path.join(str(pseudo_dir), "txt")


def is_done(pseudo_dir):
    return os.path.exists(os.path.join(str(pseudo_dir), "done.txt"))


def write_scene_labels(pseudo_dir, name, labels):
    """<pseudo_dir>/txt/<name>.txt, one `%d` per line; an existing file is kept (util/common_utils.py:304-313)."""
    os.makedirs(txt_dir(pseudo_dir), exist_ok=True)
    path = os.path.join(txt_dir(pseudo_dir), name + ".txt")
    return write_label_file(path, labels)


def write_label_file(path, labels):
    """One `%d` per line into `path`, written under a temporary name and renamed; an existing file is kept (-> False).  Shared with
    the evaluation entry point's --save_to_file (doda_amd.test)."""
    if os.path.exists(path):
        return False
    tmp = path + ".tmp.%d" % os.getpid()
    np.savetxt(tmp, np.asarray(labels).astype(np.uint8), fmt="%d")
    os.replace(tmp, path)
    return True


def write_summary(pseudo_dir, kept):
    """class_ratio.txt (np.savetxt) and done.txt (the flag set_pseudo_labels tests)."""
    np.savetxt(os.path.join(str(pseudo_dir), "class_ratio.txt"), class_ratio(kept))
    np.savetxt(os.path.join(str(pseudo_dir), "done.txt"), np.array([1]))


def read_scene_labels(pseudo_dir, paths):
    """One int32 array per base scene path from <pseudo_dir>/txt/<name>.txt."""
    out = []
    for p in paths:
        f = os.path.join(txt_dir(pseudo_dir), scene_name(p) + ".txt")
        with open(f, "rb") as fh:
            out.append(np.array(fh.read().split(), dtype=np.int32))
    return out


# ------------------------------------------------------------------------------------------------ generation (device)
def _all_reduce(t, world):
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(t)
    return t


def _scene_batches(paths, voxel_scale, batch_size):
    """Unaugmented, unshuffled items of the given base scenes, `batch_size` per batch: (xyz int voxel coordinates, xyz_mid,
    labels, index) as SyntheticScenes returns them with augment=False (dataset/scannet.py:76-78 without the augmentor)."""
    from .loader import SyntheticScenes
    ds = SyntheticScenes(paths, len(paths), voxel_scale, seed=0, augment=False)
    for b0 in range(0, len(paths), batch_size):
        yield [ds[k] for k in range(b0, min(len(paths), b0 + batch_size))]


@torch.no_grad()
def generate(model, cfg, paths, pseudo_dir, device, rank=0, world=1, feature_dtype=torch.float32, batch_size=1, log=print):
    """Pseudo labels of the target base scenes `paths` into pseudo_dir (reference set_pseudo_labels, util/pseudo_labels_util.py:
    145-165): nothing when done.txt exists.  Scenes are sharded over ranks (rank r: paths[r::world]); every rank takes part.
    batch_size: scenes per forward pass; the default 1 makes every scene's labels independent of how the scenes are batched and
    sharded (the same files for any number of ranks).
    -> dict(thresholds float32 [n_cls], kept int64 [n_cls]) or None when the files were already there."""
    from . import dist as ddist
    from . import ops
    from .collate import collate_device
    from .dsnorm import set_ds_target
    from .model import sparse_input, unwrap
    if is_done(pseudo_dir):
        return None
    net = unwrap(model)
    n_cls = int(net.linear.out_features)
    ignore = int(cfg.DATA_CONFIG.DATA_CLASS.ignore_label)
    st = cfg.SELF_TRAIN
    dp = cfg.DATA_CONFIG_TAR.DATA_PROCESSOR if "DATA_CONFIG_TAR" in cfg else cfg.DATA_CONFIG.DATA_PROCESSOR
    mine = list(paths)[rank::world]
    # store sized from the scene files (one read of each label array's shape)
    sizes = []
    for p in mine:
        with np.load(p) as f:
            sizes.append(int(f["labels"].shape[0]))
    total = sum(sizes)
    store_cls = torch.empty(total, dtype=torch.uint8, device=device)
    store_conf = torch.empty(total, dtype=torch.float32, device=device)
    hist0 = torch.zeros((n_cls, BINS), dtype=torch.int64, device=device)
    was_training = net.training
    domains = [(m, m.domain_label) for m in net.modules() if hasattr(m, "domain_label")]
    net.eval()
    if cfg.MODEL.get("dsnorm", False):
        net.apply(set_ds_target)
    try:
        off = 0
        for items in _scene_batches(mine, dp.voxel_scale, max(1, int(batch_size))):
            batch = collate_device(items, device, voxel_mode=dp.voxel_mode, full_scale=dp.get("full_scale", [128, 512]))
            inp, p2v, _ = sparse_input(cfg, net, batch, device, feature_dtype)
            pred, conf = net.voxel_confidence(inp)
            ops.st_point_store(pred, conf, p2v.to(torch.int32).contiguous(), store_cls, store_conf, off, n_cls, hist0)
            off += p2v.numel()
        assert off == total, (off, total)
    finally:
        net.train(was_training)
        for m, d in domains:
            m.domain_label = d
    _all_reduce(hist0, world)
    if st.get("global_thres", False):
        thres = global_thresholds(st.thres, n_cls)
    else:
        h0 = hist0.cpu().numpy()

        def level_hist(level, prefix):
            if level == 0:
                return h0
            h = ops.st_radix_hist(store_cls, store_conf, n_cls, level, torch.from_numpy(prefix).to(device))
            return _all_reduce(h, world).cpu().numpy()
        thres = select_thresholds(h0.sum(1), st.thres_ratio, level_hist)
    log("per class thres: %s" % [float(t) for t in thres])
    labels, kept = ops.st_label(store_cls, store_conf, torch.from_numpy(thres).to(device), ignore)
    _all_reduce(kept, world)
    labels_h, kept_h = labels.cpu().numpy(), kept.cpu().numpy()
    off = 0
    for p, n in zip(mine, sizes):
        write_scene_labels(pseudo_dir, scene_name(p), labels_h[off:off + n])
        off += n
    ddist.barrier()
    if rank == 0:
        write_summary(pseudo_dir, kept_h)
    ddist.barrier()
    return {"thresholds": thres, "kept": kept_h}

"""Training entry point with the reference's command line, YAML configs and checkpoint format
(tool/train.py:29-62 arguments, :69-158 train_epoch, :235-268 epoch loop / checkpoints, :271-361 main;
tool/st.py:100-200 for the two-pass self-training step) on top of the MI355X-native hot path.

    python -m doda_amd.train --cfg_file cfgs/scannet/spconv.yaml [--batch_size 4] [--epochs N]
           [--resume ckpt | --weight ckpt] [--launcher pytorch] [--set KEY VALUE ...]
           [--synthetic_scenes 64] [--dtype bf16] [--self_train]

What is the same: every reference flag, `_BASE_CONFIG_` / `--set` config handling (doda_amd.config),
SGD / Adam / AdamW + step / poly / cos learning-rate schedules (util/common_utils.py:154-215), DSNorm
conversion and per-domain switching (tool/train.py:89-90,332; tool/st.py:137-164), the checkpoint
dictionary `{epoch, state_dict, optimizer, commit_id, metric}` and its `module.` stripping
(util/model_utils.py:22-94), auto-resume from the newest `train_epoch_*.pth`, best-mIoU checkpoint.

What is different on purpose (SURVEY §7 "harness overheads that cap DDP scaling"): no
`torch.cuda.empty_cache()` per iteration (tool/train.py:82), no `.item()` / CPU `histc` round trip per
iteration (tool/train.py:107-118, util/common_utils.py:242-246) — loss and the intersection / union /
target histograms accumulate ON THE DEVICE and are read back every `--print_freq` iterations —, batches
are collated on the GPU (doda_amd.collate), the rulebooks of the next batch are built during the
current step (PyramidPrefetcher), gradients are averaged by doda_amd.dist.GradAllReduce.

Data: the dataset config's DATASET decides (doda_amd.loader.dataset_for): `synthetic` draws seeded
ScanNet-shaped scenes (doda_amd.scene); `scannet`, `s3dis` and `front3d` read the reference's prepared files
under DATA_ROOT, converted once into the same pool of base scenes (doda_amd.datasets, cfgs/files/)."""
import argparse
import glob
import math
import os
import subprocess
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from .config import Config, cfg_from_list, cfg_from_yaml_file
from .model import PyramidPrefetcher, SparseConvNet, point_predictions, tile_levels_for, unwrap, voxelize_and_run


# ------------------------------------------------------------------------------------------------ CLI
def build_parser():
    """tool/train.py:29-52, flag for flag; the last group is this harness's own."""
    p = argparse.ArgumentParser(description="arg parser")
    p.add_argument("--cfg_file", type=str, default=None, help="specify the config for training")
    p.add_argument("--batch_size", type=int, default=None, required=False, help="batch size for training")
    p.add_argument("--epochs", type=int, default=None, required=False, help="number of epochs to train for")
    p.add_argument("--workers", type=int, default=4, help="number of workers for dataloader")
    p.add_argument("--extra_tag", type=str, default="default", help="extra tag for this experiment")
    p.add_argument("--start_epoch", type=int, default=0)
    p.add_argument("--resume", type=str, default=None, help="checkpoint to start from")
    p.add_argument("--weight", type=str, default=None, help="pretrained_model")
    p.add_argument("--launcher", choices=["none", "pytorch", "slurm"], default="none")
    p.add_argument("--tcp_port", type=int, default=18867, help="tcp port for distrbuted training")
    p.add_argument("--sync_bn", action="store_true", default=False, help="whether to use sync bn")
    p.add_argument("--reserve_old_ckpt", action="store_true", default=False)
    p.add_argument("--manual_seed", type=int, default=None)
    p.add_argument("--ckpt_save_freq", type=int, default=1, help="number of training epochs")
    p.add_argument("--print_freq", type=int, default=5, help="printing log frequency")
    p.add_argument("--local_rank", type=int, default=0, help="local rank for distributed training")
    p.add_argument("--max_ckpt_save_num", type=int, default=30, help="max number of saved checkpoint")
    p.add_argument("--pretrain_not_strict", action="store_true", default=False,
                   help="(the reference reads this attribute at tool/train.py:344 without defining it)")
    p.add_argument("--pin_memory", action="store_true", default=False)
    p.add_argument("--synthetic_scenes", type=int, default=32, help="scenes per epoch of the synthetic loader")
    p.add_argument("--synthetic_voxels", type=int, default=150000, help="active voxels per synthetic scene")
    p.add_argument("--synthetic_base", type=int, default=16, help="procedural base scenes per split (samples = augmented base scenes)")
    p.add_argument("--scene_cache", type=str, default=None, help="directory of the base scenes (default: /dev/shm/doda_amd_scenes_<uid>)")
    p.add_argument("--host_loader", action="store_true", default=False,
                   help="DataLoader worker processes + uploads per batch (reference dataset/__init__.py:62-75) instead of the "
                        "dataset resident in HBM with the augmentation on the device (doda_amd.loader.DeviceScenes)")
    p.add_argument("--inline_loader", action="store_true", default=False,
                   help="generate and collate every batch in the training loop's own thread (the pre-round-5 loader)")
    p.add_argument("--voxel_order", choices=["auto", "first", "morton"], default="auto",
                   help="numbering of a batch's voxels (doda_amd.collate.reorder_voxels): the reference's first-appearance order, a "
                        "Z-order renumbering, or decided from the first batch's tile overflow (per-point outputs do not depend on it)")
    p.add_argument("--dtype", choices=["f32", "bf16"], default="f32", help="feature storage dtype")
    p.add_argument("--self_train", action="store_true", default=False,
                   help="step-shape benchmark of tool/st.py: a source pass and a target pass per optimizer step, the target pass "
                        "trained on the target split's GROUND-TRUTH labels (self-training with pseudo labels: python -m doda_amd.st)")
    p.add_argument("--output_root", type=str, default=None, help="default: <cfg root>/output")
    p.add_argument("--max_iters", type=int, default=None, help="stop after this many iterations (smoke runs)")
    p.add_argument("--timing_warmup", type=int, default=10, help="iterations of an epoch before its steady-state clock starts")
    p.add_argument("--timing_json", type=str, default=None, help="write {iterations, seconds, ms_per_iter, voxels_per_s} here at exit")
    p.add_argument("--curve_json", type=str, default=None,
                   help="write the run's curve here at exit: per epoch the mean training loss and, when evaluated, the held-out "
                        "loss / mIoU / per-class IoU (tools/trajectory.sh: bf16 against fp32 on the same data and seed)")
    p.add_argument("--set", dest="set_cfgs", default=None, nargs=argparse.REMAINDER,
                   help="set extra config keys if needed")
    return p


def parse_config(argv=None, parser=None):
    args = (parser or build_parser()).parse_args(argv)
    cfg = Config()
    cfg_from_yaml_file(args.cfg_file, cfg)
    cfg.TAG = Path(args.cfg_file).stem
    cfg.EXP_GROUP_PATH = "/".join(args.cfg_file.split("/")[1:-1])  # remove 'cfgs' and 'xxxx.yaml'
    cfg.LOCAL_RANK = 0
    if args.set_cfgs is not None:
        cfg_from_list(args.set_cfgs, cfg)
    return args, cfg


# ------------------------------------------------------------------------------ optimizer / LR / checkpoints
def step_learning_rate(optimizer, base_lr, epoch, step_epoch, multiplier=0.1, clip=1e-6):
    lr = max(base_lr * (multiplier ** (epoch // step_epoch)), clip)
    for g in optimizer.param_groups:
        g["lr"] = lr
    return lr


def poly_learning_rate(optimizer, base_lr, curr_iter, max_iter, power=0.9):
    lr = base_lr * (1 - float(curr_iter) / max_iter) ** power
    for g in optimizer.param_groups:
        g["lr"] = lr
    return lr


def cos_learning_rate(optimizer, base_lr, curr_iter, max_iter, warm_iter, hold_base_iter):
    lr = 0.5 * base_lr * (1 + math.cos(math.pi * (curr_iter - warm_iter - hold_base_iter) /
                                       float(max_iter - warm_iter - hold_base_iter)))
    for g in optimizer.param_groups:
        g["lr"] = lr
    return lr


def adjust_lr(optim_cfg, optimizer, scheduler, total_epochs, total_iters_per_epoch, epoch, it):
    """util/common_utils.py:176-193 (note the reference's `epoch - 1` in the step schedule)."""
    if optim_cfg.lr_decay == "step":
        return step_learning_rate(optimizer, optim_cfg.base_lr, epoch - 1, optim_cfg.step_epoch, optim_cfg.multiplier)
    if optim_cfg.lr_decay == "poly":
        return poly_learning_rate(optimizer, optim_cfg.base_lr, epoch * total_iters_per_epoch + it + 1,
                                  total_iters_per_epoch * total_epochs)
    if optim_cfg.lr_decay == "cos":
        return cos_learning_rate(optimizer, optim_cfg.base_lr, epoch * total_iters_per_epoch + it + 1,
                                 total_iters_per_epoch * total_epochs, 0, 0)
    if optim_cfg.lr_decay == "adam_onecycle":
        scheduler.step(epoch * total_iters_per_epoch + it + 1)
        return optimizer.param_groups[0]["lr"]
    if optim_cfg.lr_decay in ("multistep",):
        return optimizer.param_groups[0]["lr"]
    raise NotImplementedError(optim_cfg.lr_decay)


CLIP_GRAD_NORM = 10   # tool/train.py:100-104


def build_optimizer(optim_cfg, model, fused=None):
    """util/common_utils.py:196-215.  fused: on fp32 HIP parameters the optimizers of doda_amd.optim (torch's SGD / Adam / AdamW
    with the update of all tensors in one native launch; the packed conv weights follow it — doda_amd.spconv.conv), which also
    take OPTIMIZATION.clip_grad (tool/train.py:100-104: clip_grad_norm_(parameters, 10)) into step(); elsewhere torch's fused
    multi-tensor kernels.  fused=False and CPU parameters: plain torch optimizers, the clip left to the training loop."""
    params = [p for p in model.parameters() if p.requires_grad]
    kind = optim_cfg.get("optim", "sgd")
    kw = {}
    if fused is None:
        fused = bool(params) and params[0].is_cuda
    if fused:
        kw["fused"] = True
    native = fused and all(p.is_cuda and p.dtype == torch.float32 for p in params)
    clip = {"max_grad_norm": CLIP_GRAD_NORM} if optim_cfg.get("clip_grad", False) else {}
    if kind == "sgd":
        if native:
            from .optim import FusedSGD
            return FusedSGD(params, lr=optim_cfg.base_lr, momentum=optim_cfg.momentum,
                            weight_decay=optim_cfg.weight_decay, **clip)
        return torch.optim.SGD(params, lr=optim_cfg.base_lr, momentum=optim_cfg.momentum,
                               weight_decay=optim_cfg.weight_decay, **kw)
    if kind == "adam":
        if native:
            from .optim import FusedAdam
            return FusedAdam(params, lr=optim_cfg.base_lr, **clip)
        return torch.optim.Adam(params, lr=optim_cfg.base_lr, **kw)
    if kind == "adamw":
        if native:
            from .optim import FusedAdamW
            return FusedAdamW(params, lr=optim_cfg.base_lr, **clip)
        return torch.optim.AdamW(params, lr=optim_cfg.base_lr, **kw)
    raise NotImplementedError(kind)


def get_git_commit_id():
    if not os.path.exists(".git"):
        return "0000000"
    out = subprocess.run(["git", "rev-parse", "HEAD"], stdout=subprocess.PIPE)
    return out.stdout.decode("utf-8")[:7]


def save_params(filename, model, optimizer, epoch_log, metric=None):
    """util/model_utils.py:87-94: the reference's checkpoint dictionary, model state on the CPU."""
    net = unwrap(model)
    state = OrderedDict((k, v.cpu()) for k, v in net.state_dict().items())
    torch.save({"epoch": epoch_log, "state_dict": state, "optimizer": optimizer.state_dict(),
                "commit_id": get_git_commit_id(), "metric": metric}, filename)


def get_ckpt(path, to_cpu=True):
    ckpt = torch.load(path, map_location=torch.device("cpu") if to_cpu else None, weights_only=False)
    if "state_dict" in ckpt:   # checkpoints written from a DistributedDataParallel wrapper
        ckpt["state_dict"] = OrderedDict((k.replace("module.", ""), v) for k, v in ckpt["state_dict"].items())
    return ckpt


def load_params_from_ckpt(path, model, optimizer=None, logger=None):
    ckpt = get_ckpt(path)
    unwrap(model).load_state_dict(ckpt["state_dict"])
    if optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    if logger:
        logger("=> loaded checkpoint '%s' (epoch %s, commit %s)" % (path, ckpt["epoch"], ckpt.get("commit_id")))
    return model, optimizer, ckpt["epoch"]


def load_params_from_pretrain(path, model, strict=True, logger=None):
    ckpt = get_ckpt(path)
    unwrap(model).load_state_dict(ckpt["state_dict"], strict=strict)
    if logger:
        logger("=> loaded pretrained model '%s' (epoch %s)" % (path, ckpt["epoch"]))
    return model


def load_metric_from_ckpt(path):
    ckpt = get_ckpt(path)
    return ckpt.get("metric"), ckpt["epoch"]


# ------------------------------------------------------------------------------------------------ meters
class DeviceMeters:
    """Loss and intersection / union / target histograms accumulated on the device (the reference syncs
    with the host three times per iteration for the same numbers)."""

    def __init__(self, n_classes, ignore_label, device):
        self.k, self.ignore = n_classes, ignore_label
        self.cnt = torch.zeros(3, n_classes, dtype=torch.int64, device=device)     # intersection, prediction area, target area
        self.loss = torch.zeros(2, dtype=torch.float64, device=device)   # sum of loss * n, sum of n

    @property
    def hist(self):
        """float64 [3, k]: intersection, union, target (the reference's three meters)."""
        c = self.cnt.to(torch.float64)
        return torch.stack((c[0], c[1] + c[2] - c[0], c[2]))

    @torch.no_grad()
    def update(self, loss, preds, labels, p2v=None):
        """No host synchronisation.  preds: class per point — or per VOXEL with p2v (the fused head's argmax: the gather rides in the
        kernel).  Device tensors: one launch (ops.seg_meters; three scatter_add_ over 800 k points onto 21 addresses took 612 us per
        iteration); otherwise fixed-shape torch ops (boolean-mask indexing and bincount would each read a size back).  Ignored /
        out-of-range labels are dropped, predictions clamped to [0, k - 1]."""
        k = self.k
        if labels.is_cuda and labels.dtype == torch.int64 and k <= 256 and preds.dtype in (torch.int32, torch.int64):
            from . import ops
            ops.seg_meters(self.cnt, preds, labels, k, self.ignore, p2v=p2v)
        else:
            if p2v is not None:
                preds = preds[p2v.long()]
            preds = preds.long()
            valid = (labels != self.ignore) & (labels >= 0) & (labels < k)
            t = torch.where(valid, labels, k)
            p = torch.where(valid, preds.clamp(0, k - 1), k)
            hit = torch.where(p == t, t, k)
            ones = torch.ones_like(t)
            cnt = torch.zeros(3, k + 1, dtype=torch.int64, device=t.device)
            cnt[0].scatter_add_(0, hit, ones)
            cnt[1].scatter_add_(0, p, ones)
            cnt[2].scatter_add_(0, t, ones)
            self.cnt += cnt[:, :k]
        n = float(labels.shape[0])
        self.loss[0] += loss.detach().double() * n
        self.loss[1] += n

    def all_reduce(self):
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.cnt)
            dist.all_reduce(self.loss)

    def read(self):
        """One host read-back: (mean loss, mIoU, mAcc, allAcc, per-class IoU)."""
        h = self.hist.cpu().numpy()
        l = self.loss.cpu().numpy()
        iou = h[0] / (h[1] + 1e-10)
        acc = h[0] / (h[2] + 1e-10)
        return float(l[0] / max(l[1], 1.0)), float(iou.mean()), float(acc.mean()), float(h[0].sum() / (h[2].sum() + 1e-10)), iou


# ------------------------------------------------------------------------------------------------ data
def make_loader(cfg, args, device, rank, world, epoch, split="train"):
    """Yields collate dictionaries resident on `device` (reference dataset/dataset.py:121-187 contract).
    Synthetic stand-in for the ScanNet / 3D-FRONT / S3DIS loaders: seeded procedural scenes, a different
    set per epoch, rank and split."""
    from .collate import collate_device
    from .scene import make_scene
    bs = args.batch_size
    n_batches = max(1, args.synthetic_scenes // (bs * world))
    base = {"train": 0, "target": 500000, "val": 900000}[split] + (0 if split == "val" else epoch * 10007)
    for b in range(n_batches):
        items = []
        for k in range(bs):
            sid = base + (b * world + rank) * bs + k
            xyz, xyz_mid, lab = make_scene(1000 + sid, args.synthetic_voxels, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_scale)
            items.append((xyz, xyz_mid, lab, sid))
        yield collate_device(items, device, voxel_mode=cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_mode,
                             full_scale=cfg.DATA_CONFIG.DATA_PROCESSOR.get("full_scale", [128, 512]))


# ------------------------------------------------------------------------------------------------ training

def aug_config_of(cfg, split, class_names=None):
    """doda_amd.aug.AugConfig of a split's dataset config: DATA_CONFIG_TAR for the target split (where the experiment has one),
    DATA_CONFIG otherwise.  No DATA_AUG.aug_list there = disabled = the loaders' own rigid augmentation.  class_names: the names
    of the split's labels where a class mapper gave them (vss looks up wall / floor / ceiling); otherwise COMMON_CLASSES' names
    where the dataset config has none of its own."""
    from .aug import AugConfig
    key = "DATA_CONFIG_TAR" if (split == "target" and "DATA_CONFIG_TAR" in cfg) else "DATA_CONFIG"
    own = (cfg[key].get("DATA_CLASS", {}) or {}).get("class_names", None)
    common = (cfg.get("COMMON_CLASSES", {}) or {}).get("class_names", None)
    return AugConfig.from_cfg(cfg[key], class_names=list(class_names or own or common or []))


def check_aug_loader(cfg, args):
    """DATA_AUG.aug_list runs on the device-resident loader only, as DATA_AUG.tacm does."""
    if (getattr(args, "host_loader", False) or getattr(args, "inline_loader", False)) and \
            any(aug_config_of(cfg, split).enabled for split in ("train", "target")):
        raise ValueError("DATA_AUG.aug_list is set: scene_aug / elastic / crop run on the device-resident loader only "
                         "(drop --host_loader / --inline_loader, or remove the aug_list)")


def downsampling_scale_of(cfg, split):
    """DATA_PROCESSOR.downsampling_scale of a split's dataset config (default 1: no subsample).  The target split reads
    DATA_CONFIG_TAR, the source split DATA_CONFIG; the validation split validates the TARGET domain where the experiment has one
    (reference tool/train.py:369 builds its val loader from DATA_CONFIG_TAR, as doda_amd.test does), else DATA_CONFIG."""
    key = "DATA_CONFIG_TAR" if (split in ("target", "val") and "DATA_CONFIG_TAR" in cfg) else "DATA_CONFIG"
    scale = cfg[key].DATA_PROCESSOR.get("downsampling_scale", 1)
    return scale if scale else 1


def file_splits(cfg, args):
    """The splits of this run whose dataset config names a file dataset (DATASET: scannet | s3dis | front3d)."""
    from . import datasets
    return [split for split in used_splits(args) if datasets.kind_of(datasets.dataset_config(cfg, split)) != "synthetic"]


def used_splits(args):
    return ("train", "target", "val") if getattr(args, "self_train", False) else ("train", "val")


def check_subsample_loader(cfg, args):
    """DATA_PROCESSOR.downsampling_scale is drawn on the device-resident loader only, as DATA_AUG.aug_list is."""
    if (getattr(args, "host_loader", False) or getattr(args, "inline_loader", False)) and \
            any(downsampling_scale_of(cfg, split) > 1 for split in used_splits(args)):
        raise ValueError("DATA_PROCESSOR.downsampling_scale is above 1: the subsample is drawn on the device-resident loader only "
                         "(drop --host_loader / --inline_loader, or remove the downsampling_scale)")


class Trainer:
    def __init__(self, args, cfg, device, rank=0, world=1, log=print):
        from . import dist as ddist
        from .dsnorm import DSNorm
        from .spconv import functional as Fsp
        self.args, self.cfg, self.device, self.rank, self.world, self.log = args, cfg, device, rank, world, log
        model = SparseConvNet(cfg)
        if args.sync_bn:
            # tool/train.py:329-330, literally: torch's SyncBatchNorm (statistics all-gathered over the process
            # group, RCCL on GPUs).  It is not nn.BatchNorm1d, so SparseSequential applies it as a plain module:
            # torch's kernels, no conv-epilogue statistics.  As in the reference it takes precedence over DSNorm.
            model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        elif cfg.MODEL.get("dsnorm", False):
            model = DSNorm.convert_dsnorm(model)
        self.model = model.to(device)
        self.fdt = torch.float32 if args.dtype == "f32" else torch.bfloat16
        self.optimizer = build_optimizer(cfg.OPTIMIZATION, self.model)
        self.curve = []      # per epoch: mean training loss (+ the held-out metrics when evaluated): --curve_json
        self.deferred = Fsp.set_deferred_wgrad(True)
        self.reducer = None
        if world > 1:
            if self.deferred:
                self.reducer = ddist.GradAllReduce(self.model)
            else:
                self.model = ddist.wrap_ddp(self.model, device.index)
        self.with_pairs = bool(Fsp.WGRAD_PAIRS and self.fdt == torch.bfloat16)
        self.with_tiles = tile_levels_for(self.fdt)
        net = unwrap(self.model)
        self.n_levels = len(net.unet.nPlanes)
        self.prefetch = PyramidPrefetcher(device, self.n_levels) if device.type == "cuda" else None
        self.iters_done = 0
        self._loaders, self._datasets, self._labels = {}, {}, {}
        # tail-aware cuboid mixing of the target batches (DATA_CONFIG_TAR.DATA_AUG.tacm; absent = the plain target loader)
        from .tacm import SplitSampler, TacmConfig
        self.tacm = TacmConfig.from_cfg(cfg)
        self.split_sampler = SplitSampler(self.tacm) if self.tacm.enabled else None
        if self.tacm.enabled and (args.host_loader or args.inline_loader):
            raise ValueError("DATA_AUG.tacm is enabled: cuboid mixing runs on the device-resident loader only "
                             "(drop --host_loader / --inline_loader, or disable tacm)")
        check_aug_loader(cfg, args)
        check_subsample_loader(cfg, args)
        if args.inline_loader and file_splits(cfg, args):
            raise ValueError("DATASET of split %s is a file dataset: --inline_loader generates synthetic scenes in the training loop "
                             "(drop --inline_loader)" % file_splits(cfg, args)[0])
        self.subsampled = any(downsampling_scale_of(cfg, split) > 1 for split in used_splits(args))
        self.step_times = []      # (iterations, seconds) of the steady part of every epoch (see train_epoch)

    # one forward + backward of one batch; `domain`: None | "source" | "target" (DSNorm statistics)
    def _pass(self, batch, pyramid, domain, weight=1.0):
        from .dsnorm import set_ds_source, set_ds_target
        if self.cfg.MODEL.get("dsnorm", False) and domain is not None:
            self.model.apply(set_ds_source if domain == "source" else set_ds_target)
        labels = batch["labels"]
        # head + CrossEntropyLoss at voxel level (no [points, classes] matrix); the meters' prediction = the voxel's argmax
        loss = voxelize_and_run(self.cfg, self.model, batch, self.device, feature_dtype=self.fdt, inputs_ready=True, pyramid=pyramid,
                                labels=labels, ignore_index=self.cfg.DATA_CONFIG.DATA_CLASS.ignore_label)
        (loss * weight if weight != 1.0 else loss).backward()
        # predictions for the meters: the fused head's per-VOXEL argmax with the point -> voxel map (the gather rides in the meters'
        # kernel), or a class per point
        net = unwrap(self.model)
        vp, p2v = getattr(net, "voxel_pred", None), batch["p2v_map"]
        if vp is not None and p2v.is_cuda and p2v.dtype == torch.int32:
            return loss, (vp, p2v), labels
        return loss, (point_predictions(self.model, p2v), None), labels

    def _loader(self, split):
        """(iterable of host / device batches, object with set_epoch) per split, made once: the dataset resident in HBM
        (default) or a persistent DataLoader with worker processes (--host_loader; reference dataset/__init__.py:62-75)."""
        from . import dist as ddist
        from .loader import DeviceScenes, dataset_for, host_loader
        if split not in self._loaders:
            if self.rank == 0:
                ds = dataset_for(self.cfg, self.args, split, log=self.log)      # (generates / converts missing base scenes)
            ddist.barrier()
            if self.rank != 0:
                ds = dataset_for(self.cfg, self.args, split)
            self._datasets[split] = ds
            min_extent = getattr(ds, "min_extent", 0)
            if min_extent and self.args.host_loader:
                raise ValueError("DATASET front3d: a training sample narrower than %d voxels is drawn again on the device-resident "
                                 "loader only (drop --host_loader)" % min_extent)
            seed = self.args.manual_seed or 0
            fs0 = self.cfg.DATA_CONFIG.DATA_PROCESSOR.get("full_scale", [128, 512])[0]
            if self.args.host_loader:   # (same sampler seed and the same spatial-shape clip as the HBM-resident loader below)
                self._loaders[split] = host_loader(ds, self.args.batch_size, self.rank, self.world, self.args.workers,
                                                   shuffle=split != "val", seed=ds.seed + seed, full_scale0=fs0)
            elif split == "target" and self.tacm.enabled:
                # the mixed target loader (reference dataset/__init__.py:141-143): target scenes + the source split's base scenes
                from .loader import MixedDeviceScenes
                self._loader("train")
                src = self._datasets["train"]
                dsc = MixedDeviceScenes(ds.paths, src.paths, ds.length, ds.voxel_scale, ds.seed + seed, self.args.batch_size, self.rank,
                                        self.world, self.device, self.tacm, self.split_sampler, augment=ds.augment, shuffle=True,
                                        full_scale0=fs0, source_seed=src.seed + seed + 1,
                                        aug_cfg=aug_config_of(self.cfg, split, getattr(ds, "class_names", None)),
                                        downsampling_scale=downsampling_scale_of(self.cfg, split),
                                        source_downsampling_scale=downsampling_scale_of(self.cfg, "train"))
                self._loaders[split] = (dsc, dsc)
            else:
                dsc = DeviceScenes(ds.paths, ds.length, ds.voxel_scale, ds.seed + seed, self.args.batch_size, self.rank, self.world,
                                   self.device, augment=ds.augment, shuffle=split != "val",
                                   full_scale0=fs0, aug_cfg=aug_config_of(self.cfg, split, getattr(ds, "class_names", None)),
                                   downsampling_scale=downsampling_scale_of(self.cfg, split), subsample_seed=seed, min_extent=min_extent)
                self._loaders[split] = (dsc, dsc)
            if split in self._labels:
                self._apply_labels(split)
        return self._loaders[split]

    def epoch_items(self):
        """Items of a training epoch: --synthetic_scenes, or the scenes of a file dataset's source split (one pass)."""
        if self.args.inline_loader or self.device.type != "cuda":
            return int(self.args.synthetic_scenes)
        self._loader("train")
        return int(self._datasets["train"].length)

    def split_paths(self, split):
        """The base scene files of a split (made on first use, as the split's loader is)."""
        self._loader(split)
        return list(self._datasets[split].paths)

    def set_split_labels(self, split, labels):
        """Replace the labels of a split's base scenes (one device int32 tensor per base scene, in split_paths order): every
        augmented sample drawn from base scene k then carries labels[k] — the pseudo labels of the self-training stage
        (doda_amd.st), never the split's ground truth.  Needs the resident or the worker loader (not --inline_loader)."""
        if self.args.inline_loader:
            raise RuntimeError("split label override: --inline_loader draws scenes outside the base-scene pool")
        self._labels[split] = [t.to(self.device, torch.int32) for t in labels]
        if split in self._loaders:
            self._apply_labels(split)

    def _apply_labels(self, split):
        labels = self._labels[split]
        dl, sampler = self._loaders[split]
        if isinstance(dl, torch.utils.data.DataLoader):
            # worker processes hold a pickled copy of the dataset: a fresh loader carries the new labels to them
            self._datasets[split].set_labels([t.cpu().numpy() for t in labels])
            if getattr(dl, "_iterator", None) is not None:
                del self._loaders[split]
                self._loader(split)
        else:
            dl.set_labels(labels)

    def update_split_sampler(self, batch):
        """After the target pass (tool/st.py:82-97): the batch's tail-class cuboids, regrouped per tail class, go into the queues;
        the class counts of the queue cuboids it used, summed over ranks, move the sampler's class ratio.  Each rank keeps its own
        queue (the reference all-gathers pickled cuboids)."""
        num_c = self.tacm.num_class
        tail = batch.get("tar_tail_splits", [])
        if len(tail):
            self.split_sampler.update([[c for lst in tail[i::num_c] for c in lst] for i in range(num_c)])
        ratio = batch.get("tar_splits_class_ratio", [])
        if self.tacm.update_class_ratio and len(ratio):
            ratio = np.asarray(ratio, dtype=np.float64)
            if self.world > 1:
                import torch.distributed as dist
                t = torch.from_numpy(ratio).to(self.device)
                dist.all_reduce(t)
                ratio = t.cpu().numpy()
            self.split_sampler.update_class_ratio(ratio)

    def _batches(self, epoch, split):
        """(batch, prebuilt rulebooks): worker processes produce the scenes, a feeder thread collates them on the device and
        builds their rulebooks two batches ahead (doda_amd.loader); --inline_loader: everything in this thread, as before."""
        if not self.args.inline_loader and self.device.type == "cuda":
            from .loader import DeviceFeeder
            dl, sampler = self._loader(split)
            sampler.set_epoch(epoch)
            feeder = DeviceFeeder(iter(dl), self.device, prefetcher=self.prefetch, with_pairs=self.with_pairs,
                                  with_tiles=self.with_tiles, voxel_mode=self.cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_mode,
                                  full_scale=self.cfg.DATA_CONFIG.DATA_PROCESSOR.get("full_scale", [128, 512]),
                                  voxel_order=getattr(self, "voxel_order", None) or getattr(self.args, "voxel_order", "auto"))
            try:
                for pair in feeder:
                    yield pair
            finally:
                feeder.close()
                self.voxel_order = feeder.voxel_order      # ("auto" is decided once, from the first batch)
                if feeder.batches:
                    self.feeder_ms = (1e3 * feeder.wait_host_s / feeder.batches, 1e3 * feeder.collate_s / feeder.batches)
            return
        it = make_loader(self.cfg, self.args, self.device, self.rank, self.world, epoch, split)
        nxt = next(it, None)
        fut = self.prefetch.submit(nxt, self.with_pairs, self.with_tiles, now=True) if (nxt is not None and self.prefetch) else None
        while nxt is not None:
            cur, cur_fut = nxt, fut
            nxt = next(it, None)
            fut = self.prefetch.submit(nxt, self.with_pairs, self.with_tiles) if (nxt is not None and self.prefetch) else None
            yield cur, (PyramidPrefetcher.take(cur_fut, self.device) if cur_fut is not None else None)

    def train_epoch(self, epoch, total_epochs):
        args, cfg = self.args, self.cfg
        self.model.train()
        meters = DeviceMeters(cfg.COMMON_CLASSES.n_classes, cfg.DATA_CONFIG.DATA_CLASS.ignore_label, self.device)
        n_iter = max(1, self.epoch_items() // (args.batch_size * self.world))
        target = self._batches(epoch, "target") if args.self_train else None
        target_passes = 0
        t0 = time.time()
        warm = min(getattr(args, "timing_warmup", 10), max(0, n_iter - 2))
        t_steady = None
        for i, (batch, pyramid) in enumerate(self._batches(epoch, "train")):
            if i == warm:   # steady-state clock: from here to the end of the epoch, device drained on both sides
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                t_steady = (time.time(), i)
                vox_steady = 0
            if t_steady is not None:
                vox_steady += int(batch["voxel_locs"].shape[0])
            lr = adjust_lr(cfg.OPTIMIZATION, self.optimizer, None, total_epochs, n_iter, epoch, i)
            self.optimizer.zero_grad(set_to_none=True)
            if args.self_train:   # tool/st.py:136-198: source pass, then target pass, ONE optimizer step
                st = cfg.get("SELF_TRAIN", Config())
                loss, preds, labels = self._pass(batch, pyramid, "source",
                                                 st.get("SRC", Config()).get("loss_weight", 1.0))
                nxt = next(target, None)
                if nxt is None:
                    # a target split with fewer batches than the source split starts over under another shuffle (the reference's
                    # DataReader.read_data does this for the shorter side, util/common_utils.py:31-38)
                    target_passes += 1
                    target = self._batches(epoch + target_passes * total_epochs, "target")
                    nxt = next(target)
                tb, tp = nxt
                if self.subsampled:      # (host sizes: no read-back)
                    self.log("Subsampled batch: source %d points, target %d points" % (labels.shape[0], tb["labels"].shape[0]))
                if self.reducer is not None:
                    self.reducer.arm()      # (the second backward pass completes the gradients: its hook may start the exchange)
                self._pass(tb, tp, "target", st.get("TAR", Config()).get("loss_weight", 1.0))
                if self.tacm.enabled:
                    self.update_split_sampler(tb)
            else:
                if self.reducer is not None:
                    self.reducer.arm()
                loss, preds, labels = self._pass(batch, pyramid, "source")
                if self.subsampled:
                    self.log("Subsampled batch: source %d points" % labels.shape[0])
            if self.reducer is not None:
                self.reducer.reduce()
            if cfg.OPTIMIZATION.get("clip_grad", False) and not getattr(self.optimizer, "clips_in_step", False):
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=CLIP_GRAD_NORM)
            self.optimizer.step()
            meters.update(loss, preds[0], labels, p2v=preds[1])
            self.iters_done += 1
            if (i + 1) % args.print_freq == 0 or i == n_iter - 1:
                l, miou, macc, allacc, _ = meters.read()   # the iteration's only host read-back
                self.log("Epoch: [%d/%d][%d/%d] Batch %.3f s Loss %.4f Accuracy %.4f lr %.6f" % (
                    epoch + 1, total_epochs, i + 1, n_iter, (time.time() - t0) / (i + 1), l, allacc, lr))
            if args.max_iters is not None and self.iters_done >= args.max_iters:
                break
        if t_steady is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            done = i + 1 - t_steady[1]
            if done > 0:
                self.step_times.append((done, time.time() - t_steady[0], vox_steady))
                self.log("Steady state: %d iterations, %.3f ms per iteration" % (done, 1e3 * self.step_times[-1][1] / done))
        meters.all_reduce()
        l, miou, macc, allacc, _ = meters.read()
        self.log("Train result at epoch [%d/%d]: mIoU/mAcc/allAcc %.4f/%.4f/%.4f." % (epoch + 1, total_epochs, miou, macc, allacc))
        self.curve.append({"epoch": epoch + 1, "iterations": self.iters_done, "train_loss": l, "train_miou": miou})
        return l

    @torch.no_grad()
    def validate_epoch(self, epoch):
        from .dsnorm import set_ds_target
        from .evaluate import has_full_cloud, score_batch
        cfg = self.cfg
        self.model.eval()
        if self.reducer is not None:
            self.reducer.sync_buffers()   # evaluation with rank 0's running statistics on every rank
        if cfg.MODEL.get("dsnorm", False):
            self.model.apply(set_ds_target)
        meters = DeviceMeters(cfg.COMMON_CLASSES.n_classes, cfg.DATA_CONFIG.DATA_CLASS.ignore_label, self.device)
        full = [0, 0]
        for batch, pyramid in self._batches(epoch, "val"):
            score_batch(cfg, self.model, batch, meters, self.device, self.fdt, pyramid=pyramid)      # (OPTIMIZATION.loss's criterion)
            if has_full_cloud(batch):
                full = [full[0] + int(batch["offsets"][-1]), full[1] + int(batch["offsets_all"][-1])]
        if full[1]:
            self.log("Val full clouds: %d points scored through %d processed points" % (full[1], full[0]))
        meters.all_reduce()
        l, miou, macc, allacc, iou = meters.read()
        self.log("Val result: mIoU/mAcc/allAcc %.4f/%.4f/%.4f." % (miou, macc, allacc))
        self.log("Val IoU per class: " + " ".join("%.4f" % v for v in iou))
        if self.curve and self.curve[-1]["epoch"] == epoch + 1:
            self.curve[-1].update({"val_loss": l, "val_miou": miou, "val_allacc": allacc, "val_iou": [float(v) for v in iou]})
        return miou


def setup(args, cfg):
    """Process group, device, NUMA pinning, per-rank batch size, epochs and seeds (tool/train.py:271-300) -> (world, rank, device)."""
    from . import dist as ddist
    world, rank, local_rank = (1, 0, 0)
    if args.launcher != "none":
        world, rank, local_rank = ddist.setup()
        cfg.LOCAL_RANK = local_rank
    if not torch.cuda.is_available():
        raise RuntimeError("doda_amd.train needs an MI355X: the native ops have no CPU fallback")
    torch.cuda.set_device(local_rank % torch.cuda.device_count())
    device = torch.device("cuda", local_rank % torch.cuda.device_count())
    from .host import pin_to_device_numa
    pin_to_device_numa(device.index)     # issuing threads on the GPU's NUMA node (doda_amd/host.py)
    if args.batch_size is None:
        args.batch_size = cfg.OPTIMIZATION.BATCH_SIZE_PER_GPU
    else:
        assert args.batch_size % world == 0, "Batch size should match the number of gpus"
        args.batch_size //= world
    args.epochs = cfg.OPTIMIZATION.NUM_EPOCHS if args.epochs is None else args.epochs
    if args.manual_seed is not None:
        np.random.seed(args.manual_seed)
        torch.manual_seed(args.manual_seed)
        torch.cuda.manual_seed_all(args.manual_seed)
    return world, rank, device


def rank_logger(rank):
    def log(msg):
        if rank == 0:
            print(msg, flush=True)
    return log


def restore(trainer, args, ckpt_dir, log):
    """--weight, --resume or the newest train_epoch_*.pth of ckpt_dir, and the best metric so far -> (best_miou, best_epoch)."""
    best_miou, best_epoch = 0.0, 0
    if args.weight:
        load_params_from_pretrain(args.weight, trainer.model, strict=not args.pretrain_not_strict, logger=log)
    if args.resume:
        _, _, args.start_epoch = load_params_from_ckpt(args.resume, trainer.model, trainer.optimizer, log)
    else:
        ckpts = sorted(glob.glob(str(ckpt_dir / "*train_epoch_*.pth")), key=os.path.getmtime)
        if ckpts:
            _, _, args.start_epoch = load_params_from_ckpt(ckpts[-1], trainer.model, trainer.optimizer, log)
    if (ckpt_dir / "best_train.pth").exists():
        best_miou, best_epoch = load_metric_from_ckpt(str(ckpt_dir / "best_train.pth"))
        best_miou = best_miou or 0.0
    log("optimizer LR: %s" % trainer.optimizer.param_groups[0]["lr"])
    return best_miou, best_epoch


def run_epochs(trainer, args, cfg, ckpt_dir, rank, log, best_miou, best_epoch, after_epoch=None):
    """tool/train.py:235-268: epochs from args.start_epoch, checkpoints, evaluation and the best checkpoint.  after_epoch(epoch_log):
    called after every training epoch (doda_amd.st saves the split sampler there)."""
    for epoch in range(args.start_epoch, args.epochs):
        trainer.train_epoch(epoch, args.epochs)
        epoch_log = epoch + 1
        if after_epoch is not None:
            after_epoch(epoch_log)
        if rank == 0 and epoch_log % args.ckpt_save_freq == 0:
            filename = ckpt_dir / ("train_epoch_%d.pth" % epoch_log)
            log("Saving checkpoint to: %s" % filename)
            save_params(filename, trainer.model, trainer.optimizer, epoch_log)
            if not args.reserve_old_ckpt:
                old = ckpt_dir / ("train_epoch_%d.pth" % (epoch_log - args.ckpt_save_freq * 2))
                if old.exists():
                    old.unlink()
        if cfg.get("EVALUATION", Config()).get("evaluate", False) and epoch_log % cfg.EVALUATION.eval_freq == 0:
            miou = trainer.validate_epoch(epoch)
            if rank == 0 and miou > best_miou:
                best_miou, best_epoch = miou, epoch_log
                save_params(ckpt_dir / "best_train.pth", trainer.model, trainer.optimizer, epoch_log, metric=best_miou)
        log("Best epoch: %d, best mIoU: %s" % (best_epoch, best_miou))
        if args.max_iters is not None and trainer.iters_done >= args.max_iters:
            break
    return best_miou, best_epoch


def finish(trainer, args, rank, world):
    """Stop the helper threads and the reducer, write --timing_json / --curve_json, final barrier."""
    from . import dist as ddist
    if trainer.prefetch is not None:
        trainer.prefetch.shutdown()
    if trainer.reducer is not None:
        trainer.reducer.close()      # the gradient homes live in a process-wide map: drop this reducer's
    if args.timing_json and rank == 0 and trainer.step_times:
        import json
        its = sum(t[0] for t in trainer.step_times)
        sec = sum(t[1] for t in trainer.step_times)
        vox = sum(t[2] for t in trainer.step_times)
        with open(args.timing_json, "w") as f:
            json.dump({"iterations": its, "seconds": sec, "ms_per_iter": 1e3 * sec / its, "world": world,
                       "voxels_per_s": vox * world / sec if sec > 0 else None,   # (this rank's voxels x ranks: weak scaling)
                       "batch_size_per_gpu": args.batch_size, "workers": args.workers, "dtype": args.dtype,
                       "voxels_per_scene": args.synthetic_voxels,
                       "feeder_wait_for_workers_ms": getattr(trainer, "feeder_ms", (None, None))[0],
                       "feeder_collate_and_rulebooks_ms": getattr(trainer, "feeder_ms", (None, None))[1]}, f)
    if args.curve_json and rank == 0:
        import json
        with open(args.curve_json, "w") as f:
            json.dump({"dtype": args.dtype, "seed": args.manual_seed, "batch_size_per_gpu": args.batch_size, "world": world,
                       "scenes_per_epoch": args.synthetic_scenes, "voxels_per_scene": args.synthetic_voxels, "curve": trainer.curve}, f)
    ddist.barrier()


def output_root(args):
    return Path(args.output_root) if args.output_root else Path(os.getcwd()) / "output"


def main(argv=None):
    from . import dist as ddist
    args, cfg = parse_config(argv)
    world, rank, device = setup(args, cfg)
    output_dir = output_root(args) / cfg.EXP_GROUP_PATH / cfg.TAG / args.extra_tag
    ckpt_dir = output_dir / "ckpt"
    if rank == 0:
        ckpt_dir.mkdir(parents=True, exist_ok=True)
    ddist.barrier()
    log = rank_logger(rank)
    trainer = Trainer(args, cfg, device, rank, world, log)
    log("#classifier parameters: %d" % sum(p.nelement() for p in trainer.model.parameters()))
    best_miou, best_epoch = restore(trainer, args, ckpt_dir, log)
    run_epochs(trainer, args, cfg, ckpt_dir, rank, log, best_miou, best_epoch)
    finish(trainer, args, rank, world)


if __name__ == "__main__":
    main()

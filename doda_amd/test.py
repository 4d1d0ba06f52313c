"""Evaluation entry point: a checkpoint scored on a split, with the reference's command line (tool/test.py:33-74, :103-200, :225-306).

    python -m doda_amd.test --cfg_file doda_amd/cfgs/synthetic/spconv_eval_ds.yaml --ckpt <checkpoint> [--batch_size 4]
           [--eval_src] [--eval_tag default] [--save_to_file] [--launcher pytorch] [--set KEY VALUE ...]

The dataset config is DATA_CONFIG_TAR (DATA_CONFIG with --eval_src, or where the experiment has no target config); with
DATA_PROCESSOR.downsampling_scale > 1 the network runs on each scene's subsample and the scene's FULL cloud is scored through the
nearest processed point (doda_amd.evaluate).  Output: <root>/<group>/<tag>/<extra_tag>/eval/epoch_<last number in the checkpoint's
file name | best>/<test split>/<eval_tag>/ with log_eval_<time>.txt (the reference's `Val result` and per-class lines) and
result.json; --save_to_file adds <split>_<start_epoch>/txt/<scene>.txt, one `%d` per line, the prediction of every point of the
scored cloud (an existing file is kept).

Multi-rank: rank r scores scenes r, r + world, ... in batches of --batch_size, the last one short — every scene exactly once for any
world size and batch size (the reference pads the sampler and deletes the repeats) —, and the integer class counts are summed over
ranks, so mIoU does not depend on the rank count.  --save_logit / --save_feat would materialise the [points, classes] matrix this
path does away with: NotImplementedError."""
import datetime
import json
import os
import re

import numpy as np
import torch

from . import train as tr


def build_parser():
    """tool/test.py:33-64, flag for flag (on top of doda_amd.train's parser: the shared reference flags, --dtype, --output_root and
    the synthetic-data ones), with the reference's evaluation defaults."""
    p = tr.build_parser()
    p.description = "evaluation (tool/test.py)"
    p.add_argument("--ckpt", type=str, default=None, help="checkpoint to test")
    p.add_argument("--max_waiting_mins", type=int, default=30, help="max waiting minutes (parsed, unused: as in tool/test.py)")
    p.add_argument("--eval_tag", type=str, default="default", help="eval tag for this experiment")
    p.add_argument("--save_to_file", action="store_true", default=False, help="write the per-point predictions of every scene")
    p.add_argument("--save_logit", action="store_true", default=False, help="(reference flag; not implemented: see the module text)")
    p.add_argument("--save_feat", action="store_true", default=False, help="(reference flag; not implemented)")
    p.add_argument("--eval_src", action="store_true", default=False, help="score the source dataset config with source statistics")
    p.set_defaults(workers=16, tcp_port=18888, manual_seed=666, print_freq=1)
    return p


def parse_config(argv=None):
    return tr.parse_config(argv, build_parser())


def check_supported(args):
    for flag in ("save_logit", "save_feat"):
        if getattr(args, flag, False):
            raise NotImplementedError("--%s writes the [points, classes] matrix (or the point features) that doda_amd.test never "
                                      "builds; --save_to_file writes the predictions" % flag)


def dataset_config(cfg, eval_src=False):
    """DATA_CONFIG_TAR, or DATA_CONFIG with --eval_src or where the experiment has no target config (tool/test.py:257)."""
    return cfg.DATA_CONFIG if (eval_src or "DATA_CONFIG_TAR" not in cfg) else cfg.DATA_CONFIG_TAR


def split_name(dataset_cfg):
    split = dataset_cfg.get("DATA_SPLIT", None)
    return str(split["test"]) if split is not None and "test" in split else "val"


def epoch_id(ckpt):
    """The last number in the checkpoint's file name, or `best` (tool/test.py:259-260 searches the whole path: a digit in a
    directory name then names the epoch; here the file name decides)."""
    nums = re.findall(r"\d+", os.path.basename(str(ckpt))) if ckpt is not None else []
    return nums[-1] if nums else "best"


def eval_dir(args, cfg, dataset_cfg):
    d = tr.output_root(args) / cfg.EXP_GROUP_PATH / cfg.TAG / args.extra_tag / "eval" / ("epoch_%s" % epoch_id(args.ckpt)) / split_name(dataset_cfg)
    return d / args.eval_tag if args.eval_tag is not None else d


def shard_batches(n_scenes, world, rank, batch_size):
    """The scene indices rank `rank` of `world` scores, in batches: scenes rank, rank + world, ... cut into lists of batch_size, the
    last one short.  Over the ranks every scene appears exactly once."""
    mine = list(range(int(n_scenes)))[int(rank)::int(world)]
    bs = max(1, int(batch_size))
    return [mine[i:i + bs] for i in range(0, len(mine), bs)]


def results_of(meters, class_names=None):
    """result.json's dictionary from all-reduced DeviceMeters (tool/test.py:94-100 calc_metrics)."""
    cnt = meters.cnt.cpu().numpy().astype(np.int64)
    inter, union, target = cnt[0], cnt[1] + cnt[2] - cnt[0], cnt[2]
    loss = meters.loss.cpu().numpy()
    iou, acc = inter / (union + 1e-10), inter / (target + 1e-10)
    out = {"mIoU": float(iou.mean()), "mAcc": float(acc.mean()), "allAcc": float(inter.sum() / (target.sum() + 1e-10)),
           "loss": float(loss[0] / max(loss[1], 1.0)), "iou": [float(v) for v in iou], "acc": [float(v) for v in acc],
           "intersection": [int(v) for v in inter], "union": [int(v) for v in union], "target": [int(v) for v in target]}
    if class_names is not None:
        out["class_names"] = [str(c) for c in class_names]
    return out


def main(argv=None):
    from . import dist as ddist
    from . import pseudo_labels as pl
    from .collate import collate_device
    from .dsnorm import DSNorm, set_ds_source, set_ds_target
    from .evaluate import score_batch
    from .loader import EvalScenes, dataset_for
    from .model import SparseConvNet
    args, cfg = parse_config(argv)
    check_supported(args)
    if not args.ckpt:
        raise ValueError("--ckpt: the checkpoint to test")
    world, rank, device = tr.setup(args, cfg)
    dataset_cfg = dataset_config(cfg, args.eval_src)
    out_dir = eval_dir(args, cfg, dataset_cfg)
    if rank == 0:
        out_dir.mkdir(parents=True, exist_ok=True)
    ddist.barrier()
    log_file = out_dir / ("log_eval_%s.txt" % datetime.datetime.now().strftime("%Y%m%d-%H%M%S"))

    def log(msg):
        if rank == 0:
            print(msg, flush=True)
            with open(log_file, "a") as f:
                f.write(msg + "\n")
    log("*********************************** Start Logging*********************************")
    for key, val in vars(args).items():
        log("{:16} {}".format(key, val))

    # network (tool/test.py:285-291, :211-213)
    model = SparseConvNet(cfg)
    if args.sync_bn:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    elif cfg.MODEL.get("dsnorm", False):
        model = DSNorm.convert_dsnorm(model)
    model = model.to(device)
    tr.load_params_from_pretrain(args.ckpt, model, strict=not args.pretrain_not_strict, logger=log)
    model.eval()
    if cfg.MODEL.get("dsnorm", False):
        model.apply(set_ds_source if args.eval_src else set_ds_target)
    fdt = torch.float32 if args.dtype == "f32" else torch.bfloat16

    # dataset: the split's base scenes, unaugmented, in order
    if rank == 0:
        ds = dataset_for(cfg, args, "test", log=log)      # (generates / converts missing base scenes)
    ddist.barrier()
    if rank != 0:
        ds = dataset_for(cfg, args, "test")
    dp = dataset_cfg.DATA_PROCESSOR
    source = EvalScenes(ds.paths, dp.voxel_scale, dp.get("downsampling_scale", 1), seed=args.manual_seed or 0)
    split, epoch = split_name(dataset_cfg), args.start_epoch
    log("**********************Start testing %s/%s(%s)**********************" % (cfg.EXP_GROUP_PATH, cfg.TAG, args.extra_tag))
    log(">>>>>>>>>>>>>>>>>>>> START EVALUATION %d>>>>>>>>>>>>>>>>>>>" % epoch)

    meters = tr.DeviceMeters(cfg.COMMON_CLASSES.n_classes, cfg.DATA_CONFIG.DATA_CLASS.ignore_label, device)
    groups = shard_batches(len(source), world, rank, args.batch_size)
    for i, (ids, items) in enumerate(zip(groups, source.batches(groups))):
        batch = collate_device(items, device, voxel_mode=dp.voxel_mode, full_scale=dp.get("full_scale", [128, 512]))
        preds = score_batch(cfg, model, batch, meters, device, fdt, want_preds=args.save_to_file,
                            cell_side=4.0 / float(dp.voxel_scale))
        if args.save_to_file:
            offsets = (batch["offsets_all"] if "offsets_all" in batch else batch["offsets"]).tolist()
            preds_h = preds.cpu().numpy()
            for b, k in enumerate(ids):
                pl.write_scene_labels(out_dir / ("%s_%s" % (split, epoch)), pl.scene_name(source.paths[k]), preds_h[offsets[b]:offsets[b + 1]])
        if (i + 1) % max(1, args.print_freq) == 0:
            l, _, _, allacc, _ = meters.read()
            log("Test: [%d/%d] Loss %.4f Accuracy %.4f." % (i + 1, len(groups), l, allacc))
    meters.all_reduce()
    names = cfg.COMMON_CLASSES.get("class_names", None) or list(getattr(ds, "class_names", None) or []) or \
        [str(c) for c in range(cfg.COMMON_CLASSES.n_classes)]
    res = results_of(meters, names)
    log("Val result: mIoU/mAcc/allAcc {:.4f}/{:.4f}/{:.4f}.".format(res["mIoU"], res["mAcc"], res["allAcc"]))
    for c, name in enumerate(names):
        log("Class {} : iou/accuracy {:.4f}/{:.4f}.".format(name, res["iou"][c], res["acc"][c]))
    log("<<<<<<<<<<<<<<<<< END EVALUATION <<<<<<<<<<<<<<<<<")
    if rank == 0:
        tmp = str(out_dir / "result.json") + ".tmp.%d" % os.getpid()
        with open(tmp, "w") as f:
            json.dump(res, f, indent=1)
        os.replace(tmp, out_dir / "result.json")
    ddist.barrier()
    return res


if __name__ == "__main__":
    main()

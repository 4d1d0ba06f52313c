"""Self-training entry point: the second stage of DODA with the reference's command line (tool/st.py:34-75, :345-406, :409-530).

    python -m doda_amd.st --cfg_file doda_amd/cfgs/synthetic/spconv_st.yaml --weight <stage-1 checkpoint> [--epochs N]
           [--extra_tag default] [--st_extra_tag st] [--preserve_pseudo_labels] [--launcher pytorch] [--set KEY VALUE ...]

Output: output/<group>/<tag>/<extra_tag>/<st_extra_tag>/{ckpt,pseudo_labels}.  The run loads --weight (a path, or a file name
under the stage-1 run's ckpt/ directory: the reference's default is best_train.pth), auto-resumes from the newest
train_epoch_*.pth, validates, generates the target split's pseudo labels once (doda_amd.pseudo_labels: only when
pseudo_labels/done.txt is absent, so a resumed run reuses the files), puts them in place of the target split's labels, and trains
the two-pass step of doda_amd.train.Trainer (source pass weighted by SELF_TRAIN.SRC.loss_weight, target pass by
SELF_TRAIN.TAR.loss_weight).  Without --preserve_pseudo_labels the pseudo-label directory is removed at the end
(tool/st.py:403-405).  --pseudo_labels_freq is parsed and unused, as in the reference (tool/st.py:56)."""
import os
import shutil
from pathlib import Path

import torch

from . import train as tr


def build_parser():
    """tool/st.py:34-62, flag for flag (on top of doda_amd.train's parser: the same reference flags plus the synthetic-data ones)."""
    p = tr.build_parser()
    p.description = "self-training (tool/st.py)"
    p.add_argument("--st_extra_tag", type=str, default="st", help="extra tag for this experiment")
    p.add_argument("--pseudo_labels_freq", type=int, default=5, help="pseudo labels saving frequency (parsed, unused: tool/st.py:56)")
    p.add_argument("--preserve_pseudo_labels", action="store_true", default=False, help="keep the pseudo labels after training")
    p.add_argument("--weight_ema", type=str, default=None, help="(reference flag; the EMA teacher is not implemented: a run with it stops)")
    p.set_defaults(weight="best_train.pth", self_train=True)
    return p


def parse_config(argv=None):
    args, cfg = tr.parse_config(argv, build_parser())
    args.self_train = True        # (the stage IS the two-pass step; the target pass reads pseudo labels)
    return args, cfg


def run_dirs(args, cfg):
    """(pretrain_dir, output_dir, ckpt_dir, pseudo_labels_dir) (tool/st.py:438-441)."""
    pretrain_dir = tr.output_root(args) / cfg.EXP_GROUP_PATH / cfg.TAG / args.extra_tag
    output_dir = pretrain_dir / args.st_extra_tag
    return pretrain_dir, output_dir, output_dir / "ckpt", output_dir / "pseudo_labels"


def resolve_weight(weight, pretrain_dir):
    """--weight as given, else under the stage-1 run's ckpt directory (the default `best_train.pth`)."""
    if not weight or os.path.exists(weight):
        return weight
    cand = Path(pretrain_dir) / "ckpt" / weight
    if cand.exists():
        return str(cand)
    raise FileNotFoundError("--weight %s: neither a file nor %s" % (weight, cand))


SAMPLER_FILE = "split_sampler.pth"


def init_split_sampler(trainer, pseudo_dir, ckpt_dir, resumed, log=print):
    """tool/st.py:362-369: the split sampler's class ratio from the pseudo labels' class_ratio.txt, its thresholds into the mixing
    configuration; a resumed run takes the saved queues and ratios of ckpt/split_sampler.pth instead."""
    import numpy as np
    sampler = trainer.split_sampler
    sampler.init_class_ratio(np.loadtxt(Path(pseudo_dir) / "class_ratio.txt"))
    saved = Path(ckpt_dir) / SAMPLER_FILE
    if resumed and saved.exists():
        sampler.load_sampler(saved, device=trainer.device)
        log("split sampler: loaded %s" % saved)
    sampler.update_cfg(trainer.tacm)
    log("split sampler: tail classes %s, ratio %s" % (list(sampler.tail_class_idx), list(sampler.tail_class_ratio)))


def check_pseudo_label_clouds(cfg):
    """Pseudo labels are generated on the FULL clouds of the target scenes and subsampled with the points (reference
    util/pseudo_labels_util.py:49-51,85-87 with DATA_PROCESSOR.no_downsample_infer: True, dataset/s3dis.py:48-63).  A target config
    with a downsampling_scale above 1 and no_downsample_infer false or absent makes the reference write label files of subsample
    length that it cannot read back: rejected here, before any work."""
    dp = (cfg.DATA_CONFIG_TAR if "DATA_CONFIG_TAR" in cfg else cfg.DATA_CONFIG).DATA_PROCESSOR
    if tr.downsampling_scale_of(cfg, "target") > 1 and not dp.get("no_downsample_infer", False):
        raise ValueError("DATA_PROCESSOR.downsampling_scale is above 1 on the target config: set DATA_PROCESSOR.no_downsample_infer: True "
                         "(pseudo labels are generated on the full clouds and subsampled with the points)")


def main(argv=None):
    from . import dist as ddist
    from . import pseudo_labels as pl
    args, cfg = parse_config(argv)
    if args.weight_ema:
        raise NotImplementedError("--weight_ema: the EMA teacher of tool/st.py is not part of doda_amd.st")
    if "SELF_TRAIN" not in cfg:
        raise ValueError("doda_amd.st needs a SELF_TRAIN section (cfgs/synthetic/spconv_st.yaml)")
    from .tacm import TacmConfig
    from .train import check_aug_loader
    check_aug_loader(cfg, args)
    tr.check_subsample_loader(cfg, args)
    check_pseudo_label_clouds(cfg)
    if TacmConfig.from_cfg(cfg).enabled and (args.host_loader or args.inline_loader):
        raise ValueError("DATA_AUG.tacm is enabled: cuboid mixing runs on the device-resident loader only "
                         "(drop --host_loader / --inline_loader, or disable tacm)")
    world, rank, device = tr.setup(args, cfg)
    pretrain_dir, output_dir, ckpt_dir, pseudo_dir = run_dirs(args, cfg)
    if rank == 0:
        ckpt_dir.mkdir(parents=True, exist_ok=True)
        pseudo_dir.mkdir(parents=True, exist_ok=True)
    ddist.barrier()
    log = tr.rank_logger(rank)
    trainer = tr.Trainer(args, cfg, device, rank, world, log)
    log("#classifier parameters: %d" % sum(p.nelement() for p in trainer.model.parameters()))
    args.weight = resolve_weight(args.weight, pretrain_dir)
    best_miou, best_epoch = tr.restore(trainer, args, ckpt_dir, log)
    trainer.validate_epoch(args.start_epoch)        # (tool/st.py:345: before the first epoch, whatever EVALUATION says)
    st = cfg.SELF_TRAIN
    log("thres: %s" % (st.thres,) if st.get("global_thres", False) else "thres ratio: %s" % (st.thres_ratio,))
    if args.start_epoch < args.epochs:
        paths = trainer.split_paths("target")
        out = pl.generate(trainer.model, cfg, paths, pseudo_dir, device, rank, world, feature_dtype=trainer.fdt, log=log)
        log("pseudo labels: %s" % ("generated" if out is not None else "reused from %s" % pseudo_dir))
        labels = pl.read_scene_labels(pseudo_dir, paths)
        trainer.set_split_labels("target", [torch.from_numpy(a) for a in labels])
        if trainer.tacm.enabled:
            init_split_sampler(trainer, pseudo_dir, ckpt_dir, args.start_epoch > 0, log)
    tr.run_epochs(trainer, args, cfg, ckpt_dir, rank, log, best_miou, best_epoch,
                  after_epoch=(lambda _e: trainer.split_sampler.save_sampler(ckpt_dir / SAMPLER_FILE))
                  if (trainer.tacm.enabled and rank == 0) else None)      # (tool/st.py:396-398)
    tr.finish(trainer, args, rank, world)
    if not args.preserve_pseudo_labels and rank == 0:
        shutil.rmtree(pseudo_dir, ignore_errors=True)
    ddist.barrier()


if __name__ == "__main__":
    main()

"""Scoring one evaluation batch (reference model/unet.py:115-152 test_model_fn + tool/test.py:81-91 update_meter), shared by the
evaluation entry point (doda_amd.test) and Trainer.validate_epoch.

A batch whose processed cloud is a SUBSET of its full cloud — it carries `offsets_all` and offsets[-1] < offsets_all[-1], the
reference's own condition (model/unet.py:135) — is scored on the full cloud: the trunk runs on the processed points, every full
point takes the scores of its nearest processed point (ops.eval_nn: doda_eval_nn, the exact grid search instead of the
reference's brute-force pointops.knnquery) and predictions, class histograms and cross-entropy come from ops.eval_score without
the [full points, classes] matrix `output[point_idx]`.  Any other batch takes the validation computation as it was."""
import torch


def has_full_cloud(batch):
    return "offsets_all" in batch and int(batch["offsets"][-1]) < int(batch["offsets_all"][-1])


def default_cell_side(voxel_scale):
    """Cell side of the nearest-neighbour grid in metres: four voxels (8 cm at the 2 cm voxels of the shipped configs — a cell then
    holds a handful of processed points and the first shell usually decides)."""
    return 4.0 / float(voxel_scale)


@torch.no_grad()
def score_batch(cfg, model, batch, meters, device, feature_dtype, want_preds=False, pyramid=None, cell_side=None):
    """Add one batch to `meters` (doda_amd.train.DeviceMeters).  -> the class per point of the cloud that was scored (the full cloud
    where the batch has one; uint8 there, int64 otherwise) when want_preds, else None.  cell_side: metres, default
    default_cell_side(DATA_CONFIG.DATA_PROCESSOR.voxel_scale)."""
    from . import ops
    from .model import criterion_of, sparse_input, unwrap, voxelize_and_run
    ignore = cfg.DATA_CONFIG.DATA_CLASS.ignore_label
    if not has_full_cloud(batch):
        scores = voxelize_and_run(cfg, model, batch, device, feature_dtype=feature_dtype, inputs_ready=True, pyramid=pyramid)
        loss = criterion_of(model)(scores, batch["labels"], ignore_index=ignore)
        preds = scores.argmax(1)
        meters.update(loss, preds, batch["labels"])
        return preds if want_preds else None
    net = unwrap(model)
    inp, p2v, _ = sparse_input(cfg, model, batch, device, feature_dtype, inputs_ready=True, pyramid=pyramid)
    feats = net._trunk(inp).features.contiguous()
    if cell_side is None:
        cell_side = default_cell_side(cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_scale)
    xyz = batch["locs_float"].to(device, non_blocking=True)
    xyz_all = batch["locs_float_all"].to(device, non_blocking=True)
    labels_all = batch["labels_all"].to(device, non_blocking=True)
    idx, _ = ops.eval_nn(xyz, xyz_all, batch["offsets"][1:].to(device), batch["offsets_all"][1:].to(device), cell_side=cell_side)
    weight, bias = net.linear.weight.detach(), net.linear.bias.detach() if net.linear.bias is not None else None
    out, preds = ops.eval_score(feats, weight, bias, p2v.to(torch.int32), idx, labels_all, ignore, meters.cnt, want_pred=want_preds)
    if getattr(net, "loss_kind", "cross_entropy") == "lovasz":
        # the slow but correct route, for a log line: point scores gathered with torch, the existing criterion
        scores = net.linear(feats[p2v.long()].to(net.linear.weight.dtype))[idx.long()]
        loss = criterion_of(model)(scores, labels_all, ignore_index=ignore).double()
    else:
        loss = out[0] / out[1].clamp(min=1.0)
    n = float(labels_all.shape[0])      # (weighted as DeviceMeters.update weighs a batch: by its points)
    meters.loss[0] += loss * n
    meters.loss[1] += n
    return preds

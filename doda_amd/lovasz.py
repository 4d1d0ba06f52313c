"""Lovasz-softmax loss (OPTIMIZATION.loss: lovasz; reference model/unet.py:109-111 -> util/loss_utils.py
lovasz_softmax_with_logit -> util/lovasz_loss.py lovasz_softmax(softmax(scores), labels, classes='present', ignore=...)).

Per class c, with fg_i = [label_i == c] over the valid points, the errors e_i = |fg_i - p_i[c]| sorted in descending order and
G = sum fg:

    J_k    = 1 - (G - cumfg_k) / (G + cumbg_k)          (cumfg / cumbg: fg / non-fg points among the first k)
    loss_c = sum_k e_(k) (J_k - J_(k-1)),  J_0 = 0
    loss   = mean of loss_c over the classes with G > 0

The loss does not depend on the order of tied errors: across a run of ties the factors J_k - J_(k-1) telescope.

* `lovasz_softmax(scores, labels, ignore_index)`: that formula at point level in plain torch, any float dtype, any device — the
  fallback where the fused form does not apply (as model.cross_entropy has one), the fp64 yardstick of the tests and what
  tools/lovaszbench.py times the device path against.
* `_VoxelHeadLovasz`: Linear head + loss at VOXEL level over include/doda_loss.h (csrc/lovasz.hip): all points of a voxel share
  its logits, so a class sees two weighted items per voxel and the [points, classes] matrix is never built.

Deviation from the reference: with every point ignored the reference returns an empty [0, C] tensor that cannot be
back-propagated; both forms here return a scalar 0 with zero gradients."""
import torch
from torch.autograd import Function

from . import ops as _ops


def lovasz_softmax(scores, labels, ignore_index=255, compute_dtype=torch.float64):
    """scores [N, C] logits (softmax is applied here, as lovasz_softmax_with_logit does), labels int64 [N] -> the loss in the scores'
    dtype (float32 for half types).  All classes are sorted at once along the point axis; the integer prefix counts are exact; no
    host read-back.
    compute_dtype: the evaluation runs in fp64 whatever the scores' type and is rounded once at the end.  An fp32 evaluation
    inherits half an ulp of every probability (3e-8 at p >= 0.5) with nothing to average it out when the voxels are few — more
    than the distance the reference's own fp32 code happens to keep from the exact value there — and the reference's function has
    no fp64 form to fall back on (torch.dot raises).  torch.float32 gives the plain fp32 evaluation (tools/lovaszbench.py times
    both)."""
    out_dtype = scores.dtype if scores.dtype in (torch.float32, torch.float64) else torch.float32
    n_cls = scores.shape[1]
    valid = (labels != ignore_index) & (labels >= 0) & (labels < n_cls)
    idx = valid.nonzero().squeeze(1)
    probs = torch.softmax(scores.index_select(0, idx).to(compute_dtype), dim=1)
    fg = labels.index_select(0, idx).unsqueeze(1) == torch.arange(n_cls, device=labels.device).unsqueeze(0)      # [n, C]
    errors = (fg.to(probs.dtype) - probs).abs()
    errors_sorted, order = torch.sort(errors, dim=0, descending=True)
    fg_sorted = fg.gather(0, order).long()
    total = fg_sorted.sum(0, keepdim=True)                                                                       # G [1, C]
    cumfg, cumbg = fg_sorted.cumsum(0), (1 - fg_sorted).cumsum(0)
    jac = 1.0 - (total - cumfg).to(probs.dtype) / (total + cumbg).to(probs.dtype)   # (G + cumbg >= 1 on every row: cumfg + cumbg = row + 1)
    grad = jac.clone()
    grad[1:] -= jac[:-1]
    per_class = (errors_sorted * grad).sum(0)
    present = (total.squeeze(0) > 0).to(probs.dtype)
    return ((per_class * present).sum() / present.sum().clamp(min=1)).to(out_dtype)


class _VoxelHeadLovasz(Function):
    """loss = lovasz_softmax(Linear(feats[p2v]), labels, ignore_index) computed at VOXEL level (csrc/lovasz.hip): per class a stable
    radix sort of 2 m weighted (voxel, fg | bg) items, integer prefix sums, J in fp64.  Same returns as model._VoxelHeadCE:
    (loss, per-voxel argmax class)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, v2p, labels, ignore_index):
        want = any(ctx.needs_input_grad[:3])
        out, pred, gitem = _ops.lovasz_fwd(feats, weight, bias, v2p, labels, ignore_index, want_grad=want)
        ctx.save_for_backward(feats, weight, bias, gitem, out)
        ctx.mark_non_differentiable(pred)
        return out[0], pred

    @staticmethod
    def backward(ctx, grad, _grad_pred):
        feats, weight, bias, gitem, out = ctx.saved_tensors
        bwd = _ops.lovasz_bwd(feats, weight, bias, gitem, out, grad.reshape(1).to(torch.float32))
        return _ops.head_grads(ctx.needs_input_grad, feats, weight, bias, *bwd)   # (dW: the cross-entropy head's kernels on dz and dz_lo)

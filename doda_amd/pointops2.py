"""The reference's `pointops` wrappers (lib/pointops2/functions/pointops2.py:33-237) over doda_amd.ops: knnquery as DODA calls it
(model/unet.py:135-138), and the point backbone's operators — furthest point sampling, grouping, query-and-group, subtraction,
aggregation and kNN interpolation — with the reference's argument lists and return shapes.

Offsets arrive as int32 [B + 1] with a leading 0 (stripped before the native call, as the reference does).  Features are float32
only: anything else is a TypeError.  Every backward sums in a fixed order (include/doda_pointops.h), through the index of `idx` by
destination.  That index is built in the first backward that needs it and remembered on the idx tensor while `idx._version` and the
destination count stay the same, so a block that passes one idx to subtraction, aggregation and grouping builds it once."""
import torch
from torch.autograd import Function

from . import ops as _ops


@torch.no_grad()
def knnquery(nsample, xyz, new_xyz, offset, new_offset):
    """For each row of new_xyz [m,3] (None: xyz itself) its `nsample` nearest rows of xyz [n,3] inside the same batch
    segment; offset / new_offset: int32 [B+1] segment ends with a leading 0 (stripped before the native call, as the
    reference does).  Returns (idx int32 [m,nsample] ascending by distance, dist float32 [m,nsample] = sqrt of the
    squared distance)."""
    queries = xyz if new_xyz is None else new_xyz
    if not (xyz.is_contiguous() and queries.is_contiguous()):
        raise AssertionError("knnquery: contiguous xyz / new_xyz expected")
    m = queries.shape[0]
    idx = xyz.new_zeros((m, nsample), dtype=torch.int32)
    dist2 = xyz.new_zeros((m, nsample), dtype=torch.float32)
    _ops.knnquery(m, nsample, xyz, queries, offset[1:], new_offset[1:], idx, dist2)
    return idx, dist2.sqrt_()


class KNNQuery:   # `KNNQuery.apply(...)`: the reference's class name for the same call
    apply = staticmethod(knnquery)


def transposed(idx, n):
    """(start, pos) of ops.po_transpose(idx, n), remembered on the idx tensor for as long as it is not written to."""
    key = (idx._version, int(n))
    memo = getattr(idx, "_doda_po_transposed", None)
    if memo is None or memo[0] != key:
        memo = (key, _ops.po_transpose(idx, n))
        idx._doda_po_transposed = memo
    return memo[1]


def _empty(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


@torch.no_grad()
def furthestsampling(xyz, offset, new_offset):
    """xyz [n, dim] (dim 1..8), offset / new_offset int32 [B + 1] -> idx int32 [new_offset[-1]]: per segment the first point, then
    always the point furthest from the samples so far; exact ties go to the lowest index.  Nothing differentiable."""
    if xyz.dtype != torch.float32:
        raise TypeError("furthestsampling: float32 xyz expected, got %s" % xyz.dtype)
    if not xyz.is_contiguous():
        raise AssertionError("furthestsampling: contiguous xyz expected")
    m = int(new_offset[-1].item())
    idx = torch.empty(m, dtype=torch.int32, device=xyz.device)
    tmp = torch.empty(xyz.shape[0], dtype=torch.float32, device=xyz.device)
    _ops.po_furthestsampling(xyz, offset[1:].contiguous(), new_offset[1:].contiguous(), tmp, idx)
    return idx


class FurthestSampling:   # `FurthestSampling.apply(...)`: no graph, as the reference's forward-only Function
    apply = staticmethod(furthestsampling)


class Grouping(Function):
    @staticmethod
    def forward(ctx, input, idx):
        """input [n, c], idx [m, nsample] -> [m, nsample, c]"""
        input = input.contiguous()
        out = _empty(input, idx.shape[0], idx.shape[1], input.shape[1])
        _ops.po_grouping_fwd(input, idx, out)
        ctx.n, ctx.idx = input.shape[0], idx
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        ctx.saved_tensors   # (autograd's check that idx was not written to since the forward)
        m, nsample, c = grad_output.shape
        grad_input = _empty(grad_output, ctx.n, c)
        start, pos = transposed(ctx.idx, ctx.n)
        _ops.po_grouping_bwd(grad_output.contiguous().view(m * nsample, c), start, pos, grad_input)
        return grad_input, None


grouping = Grouping.apply


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """xyz [n, 3], new_xyz [m, 3] (None: xyz), feat [n, c], idx [m, nsample] (None: knnquery) -> [m, nsample, 3 + c], or
    [m, nsample, c] without use_xyz.  Both gathers go through `grouping`, so gradients reach xyz, new_xyz and feat as they do
    through the reference's indexing."""
    if new_xyz is None:
        new_xyz = xyz
    if not (xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()):
        raise AssertionError("queryandgroup: contiguous xyz / new_xyz / feat expected")
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    grouped_feat = grouping(feat, idx)
    if not use_xyz:
        return grouped_feat
    grouped_xyz_diff = grouping(xyz, idx) - new_xyz.unsqueeze(1)
    return torch.cat((grouped_xyz_diff, grouped_feat), -1)


class Subtraction(Function):
    @staticmethod
    def forward(ctx, input1, input2, idx):
        """input1 [n, c], input2 [n, c], idx [n, nsample] -> [n, nsample, c] = input1[r] - input2[idx[r, i]]"""
        input1, input2 = input1.contiguous(), input2.contiguous()
        out = _empty(input1, idx.shape[0], idx.shape[1], input1.shape[1])
        _ops.po_subtraction_fwd(input1, input2, idx, out)
        ctx.n2, ctx.idx = input2.shape[0], idx
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        ctx.saved_tensors
        n, nsample, c = grad_output.shape
        grad_input1, grad_input2 = _empty(grad_output, n, c), _empty(grad_output, ctx.n2, c)
        start, pos = transposed(ctx.idx, ctx.n2)
        _ops.po_subtraction_bwd(grad_output.contiguous(), start, pos, grad_input1, grad_input2)
        return grad_input1, grad_input2, None


subtraction = Subtraction.apply


class Aggregation(Function):
    @staticmethod
    def forward(ctx, input, position, weight, idx):
        """input [n, c], position [n, nsample, c], weight [n, nsample, c'], idx [n, nsample] -> [n, c]"""
        input, position, weight = input.contiguous(), position.contiguous(), weight.contiguous()
        out = _empty(input, position.shape[0], position.shape[2])
        _ops.po_aggregation_fwd(input, position, weight, idx, out)
        ctx.idx = idx
        ctx.save_for_backward(input, position, weight, idx)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        input, position, weight, idx = ctx.saved_tensors
        grad_input, grad_position, grad_weight = torch.empty_like(input), torch.empty_like(position), torch.empty_like(weight)
        start, pos = transposed(ctx.idx, input.shape[0])
        _ops.po_aggregation_bwd(input, position, weight, idx, start, pos, grad_output.contiguous(), grad_input, grad_position,
                                grad_weight)
        return grad_input, grad_position, grad_weight, None


aggregation = Aggregation.apply


def _interpolation_weights(xyz, new_xyz, offset, new_offset, k):
    """kNN of new_xyz in xyz and the normalised inverse distances: elementwise torch, as in the reference."""
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)
    dist_recip = 1.0 / (dist + 1e-8)
    norm = torch.sum(dist_recip, dim=1, keepdim=True)
    return idx, (dist_recip / norm).contiguous()


class Interpolation(Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, input, offset, new_offset, k=3):
        """xyz [m, 3], new_xyz [n, 3], input [m, c] -> [n, c]"""
        if not (xyz.is_contiguous() and new_xyz.is_contiguous() and input.is_contiguous()):
            raise AssertionError("interpolation: contiguous xyz / new_xyz / input expected")
        idx, weight = _interpolation_weights(xyz, new_xyz, offset, new_offset, k)
        out = _empty(input, new_xyz.shape[0], input.shape[1])
        _ops.po_interpolation_fwd(input, idx, weight, out)
        ctx.m, ctx.idx = input.shape[0], idx
        ctx.save_for_backward(idx, weight)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        _, weight = ctx.saved_tensors
        grad_input = _empty(grad_output, ctx.m, grad_output.shape[1])
        start, pos = transposed(ctx.idx, ctx.m)
        _ops.po_interpolation_bwd(grad_output.contiguous(), weight, start, pos, grad_input)
        return None, None, grad_input, None, None, None


interpolation2 = Interpolation.apply


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """The reference's first form (pointops2.py:187-201): the same interpolation; its gradient reaches feat alone, as the
    reference's index-and-multiply loop lets it (idx and the weights come from a query without a graph)."""
    return Interpolation.apply(xyz, new_xyz, feat, offset, new_offset, k)

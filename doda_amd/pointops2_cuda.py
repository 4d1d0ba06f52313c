"""`pointops2_cuda`-shaped module (reference lib/pointops2/src/pointops_api.cpp:12-23): the eleven functions with the reference's raw
signatures — sizes first, caller-allocated outputs — over doda_amd.ops (include/doda_hip.h for knnquery, include/doda_pointops.h for
the rest).

Differences from the reference, all deliberate (include/doda_pointops.h):
* The reference's kernels ADD into the output buffers, which its wrappers always pass zeroed; these OVERWRITE every output element.
* The backwards sum in a fixed order (no float atomic), through an index by destination that is built from `idx` on each call here;
  doda_amd.pointops2 remembers it on the idx tensor instead.
* Furthest point sampling resolves exact ties to the lowest point index; `tmp` is used as the workspace and is initialised by the
  kernel, so its contents on entry do not matter.
* Indices outside the indexed array read as 0 and receive no gradient."""
from . import ops as _ops


def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    """knnquery/knnquery_cuda.cpp:8-17: offset/new_offset are END offsets per batch item."""
    _ops.knnquery(m, nsample, xyz.contiguous(), new_xyz.contiguous(), offset.contiguous(),
                  new_offset.contiguous(), idx, dist2)


def furthestsampling_dim_cuda(b, n, dim, xyz, offset, new_offset, tmp, idx):
    """sampling/sampling_cuda.cpp:18: b batch items, n the largest segment (unused here: one workgroup shape serves every size),
    offset / new_offset END offsets, tmp float32 [total points], idx int32 [new_offset[-1]] written in full."""
    xyz = xyz.contiguous()
    if xyz.dim() != 2 or xyz.shape[1] != int(dim) or offset.numel() != int(b):
        raise RuntimeError("furthestsampling: xyz [n, dim] and b offsets expected")
    _ops.po_furthestsampling(xyz, offset.contiguous(), new_offset.contiguous(), tmp, idx)


def furthestsampling_cuda(b, n, xyz, offset, new_offset, tmp, idx):
    """sampling/sampling_cuda.cpp:8: the 3-D case of furthestsampling_dim_cuda."""
    furthestsampling_dim_cuda(b, n, 3, xyz, offset, new_offset, tmp, idx)


def _sized(what, t, *shape):
    if t.numel() != _prod(shape):
        raise RuntimeError("%s: a tensor of %s elements expected, got %s" % (what, "x".join(map(str, shape)), tuple(t.shape)))
    return t.contiguous().view(*shape)


def _prod(shape):
    p = 1
    for s in shape:
        p *= int(s)
    return p


def grouping_forward_cuda(m, nsample, c, input, idx, output):
    _ops.po_grouping_fwd(input.contiguous(), _sized("grouping_forward", idx, m, nsample), output)


def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
    start, pos = _ops.po_transpose(_sized("grouping_backward", idx, m, nsample), grad_input.shape[0])
    _ops.po_grouping_bwd(_sized("grouping_backward", grad_output, m * nsample, c), start, pos, grad_input)


def interpolation_forward_cuda(n, c, k, input, idx, weight, output):
    _ops.po_interpolation_fwd(input.contiguous(), _sized("interpolation_forward", idx, n, k),
                              _sized("interpolation_forward", weight, n, k), output)


def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
    start, pos = _ops.po_transpose(_sized("interpolation_backward", idx, n, k), grad_input.shape[0])
    _ops.po_interpolation_bwd(_sized("interpolation_backward", grad_output, n, c), _sized("interpolation_backward", weight, n, k),
                              start, pos, grad_input)


def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
    _ops.po_subtraction_fwd(_sized("subtraction_forward", input1, n, c), input2.contiguous(),
                            _sized("subtraction_forward", idx, n, nsample), output)


def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
    start, pos = _ops.po_transpose(_sized("subtraction_backward", idx, n, nsample), grad_input2.shape[0])
    _ops.po_subtraction_bwd(_sized("subtraction_backward", grad_output, n, nsample, c), start, pos, grad_input1, grad_input2)


def aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output):
    _ops.po_aggregation_fwd(input.contiguous(), _sized("aggregation_forward", position, n, nsample, c),
                            _sized("aggregation_forward", weight, n, nsample, w_c), _sized("aggregation_forward", idx, n, nsample),
                            output)


def aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input, grad_position, grad_weight):
    idx = _sized("aggregation_backward", idx, n, nsample)
    start, pos = _ops.po_transpose(idx, grad_input.shape[0])
    _ops.po_aggregation_bwd(input.contiguous(), _sized("aggregation_backward", position, n, nsample, c),
                            _sized("aggregation_backward", weight, n, nsample, w_c), idx, start, pos,
                            _sized("aggregation_backward", grad_output, n, c), grad_input, grad_position, grad_weight)

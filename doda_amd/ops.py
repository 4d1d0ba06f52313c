"""Tensor-level entry points over the C ABI (include/doda_hip.h).

Each function validates tensors, allocates outputs/workspaces from PyTorch's caching allocator,
and makes exactly the native calls — no arithmetic happens in Python and there is no CPU fallback
(device tensors are required wherever the ABI takes device pointers).
"""
import ctypes as C

import numpy as np
import torch

from ._lib import LOVASZ_MAX_POINTS_PER_VOXEL, DodaNativeError, check, lib  # noqa: F401
from ._lib import (CX_BNBWD, CX_BNFWD, CX_F_ACCUM, CX_F_BARRIER, CX_F_IDENTITY, CX_F_RELU, CX_F_TRAINING, CX_GEMM, CX_STATS,  # noqa: F401
                   PACK_DESC, STATS_SLOTS, WGRAD_ACCUMULATE)
from ._lib import ConvEpilogue as _ConvEpilogue, CxOp as _CxOp, SgdTensor as _SgdTensor, WgradJob as _WgradJob


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter is ~30x cheaper
    than torch.cuda.current_stream(), which dominated the host time of a U-Net step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("doda_amd native ops need device (ROCm) tensors; got a %s tensor — "
                               "there is no CPU fallback" % t.device)


_WS = {}


def _ws(nbytes, device):
    """Scratch for ONE native call.  Calls on a stream execute in order, so a single grow-only
    buffer per (device, stream) is reused instead of allocating per call."""
    nbytes = max(int(nbytes), 256)
    key = (device, _stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


# ------------------------------------------------------------------------------------------
# voxelisation
# ------------------------------------------------------------------------------------------
def voxelize_idx_host(coords, batch_size, mode=4):
    """CPU point->voxel maps; reference PG_OP.voxelize_idx (voxelize.cpp:10-31).

    coords: int64 CPU [N, 3|4].  Returns (output_coords int64 [M,ncol], input_map int32 [N],
    output_map int32 [M, 1+maxActive])."""
    if coords.is_cuda or coords.dtype != torch.int64 or coords.dim() != 2:
        raise RuntimeError("voxelize_idx_host: coords must be a CPU int64 [N,3|4] tensor")
    coords = coords.contiguous()
    n, ncol = coords.shape
    input_map = torch.zeros(n, dtype=torch.int32)
    handle = C.c_void_p()
    n_active, max_active = C.c_int32(), C.c_int32()
    check(lib().doda_voxelize_idx_h(_p(coords), n, ncol, int(batch_size), int(mode), _p(input_map),
                                    C.byref(handle), C.byref(n_active), C.byref(max_active)),
          "doda_voxelize_idx_h")
    out_coords = torch.zeros((n_active.value, ncol), dtype=torch.int64)
    out_map = torch.zeros((n_active.value, max_active.value + 1), dtype=torch.int32)
    check(lib().doda_voxelize_idx_fill_h(handle, _p(coords), _p(out_coords), _p(out_map)),
          "doda_voxelize_idx_fill_h")
    return out_coords, input_map, out_map


def voxelize_idx_device(coords, batch_size, mode=4, sizes=None):
    """Device version of voxelize_idx (same results); coords int64 device [N,3|4].
    sizes = (n_voxels, max_active) known to the caller — the EXACT values a previous call on the same points returned
    (out_map.shape[0], out_map.shape[1] - 1): the D2H read-back of the two output sizes between the assign and the fill
    kernel is skipped.  The outputs are allocated from them; the fill kernels bound every write by them, so a wrong
    size cannot write outside the outputs, but it does not give the reference's result: too small drops the voxels /
    points that do not fit, too large leaves trailing rows empty (count 0, index -1, coordinates 0)."""
    _need_cuda(coords)
    if coords.dtype != torch.int64 or coords.dim() != 2:
        raise RuntimeError("voxelize_idx_device: coords must be int64 [N,3|4]")
    coords = coords.contiguous()
    n, ncol = coords.shape
    dev = coords.device
    input_map = torch.empty(n, dtype=torch.int32, device=dev)      # (every entry is written by the assign kernel)
    counts = torch.empty(2, dtype=torch.int32, device=dev)          # (zeroed by doda_voxelize_idx_assign itself)
    nbytes = lib().doda_voxelize_idx_workspace_bytes(n)
    ws = _ws(nbytes, dev)
    check(lib().doda_voxelize_idx_assign(_p(coords), n, ncol, int(mode), _p(input_map), _p(counts),
                                         _p(ws), ws.numel(), _stream()), "doda_voxelize_idx_assign")
    if sizes is not None:
        m, max_active = int(sizes[0]), int(sizes[1])
    else:
        m, max_active = (int(v) for v in counts.tolist())  # one D2H sync: sizes of the outputs
    max_active = max(max_active, 1)
    # (the fill kernels write every element of both outputs: rows_init all of out_map, finish all of out_coords)
    out_coords = torch.empty((m, ncol), dtype=torch.int64, device=dev)
    out_map = torch.empty((m, max_active + 1), dtype=torch.int32, device=dev)
    if n == 0 or m == 0:
        out_coords.zero_(); out_map.zero_()
    check(lib().doda_voxelize_idx_fill(_p(coords), n, ncol, int(mode), m, max_active,
                                       _p(out_coords), _p(out_map), _p(ws), ws.numel(), _stream()),
          "doda_voxelize_idx_fill")
    return out_coords, input_map, out_map


def _pool_args(feats, out, rules):
    _need_cuda(feats, out, rules)
    if feats.dtype != torch.float32 or out.dtype != torch.float32 or rules.dtype != torch.int32:
        raise RuntimeError("voxel pooling: feats/out must be float32 and rules int32")
    if not (feats.is_contiguous() and out.is_contiguous() and rules.is_contiguous()):
        raise RuntimeError("voxel pooling: tensors must be contiguous")


def voxelize_fp(feats, out, rules, mode, n_active, max_active, n_plane):
    _pool_args(feats, out, rules)
    check(lib().doda_voxelize_fp(_p(feats), _p(out), _p(rules), int(mode), int(n_active),
                                 int(max_active), int(n_plane), _stream()), "doda_voxelize_fp")


def voxelize_fp_rows(feats_a, feats_b, rules, mode, c_out, dtype):
    """The network's input rows in ONE launch (doda_voxelize_fp_rows): voxelization(cat(feats_a, feats_b), rules, mode) cast to
    `dtype` (float32 / bfloat16) and zero-padded to c_out channels.  feats_b may be None.  No gradient."""
    cb = 0 if feats_b is None else feats_b.shape[1]
    for t in (feats_a, feats_b):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.device != rules.device):
            raise RuntimeError("voxelize_fp_rows: point features must be contiguous float32 [N, C] on the rules' device")
    if feats_b is not None and feats_b.shape[0] != feats_a.shape[0]:
        raise RuntimeError("voxelize_fp_rows: the two feature matrices differ in rows")
    if rules.dtype != torch.int32 or not rules.is_contiguous() or rules.dim() != 2:
        raise RuntimeError("voxelize_fp_rows: rules must be contiguous int32 [M, 1 + maxActive]")
    if dtype not in (torch.float32, torch.bfloat16) or c_out < feats_a.shape[1] + cb:
        raise RuntimeError("voxelize_fp_rows: dtype float32 / bfloat16, c_out >= the pooled channels")
    m = rules.shape[0]
    out = torch.empty((m, c_out), dtype=dtype, device=rules.device)
    check(lib().doda_voxelize_fp_rows(_p(feats_a), int(feats_a.shape[1]), _p(feats_b) if feats_b is not None else None, int(cb),
                                      _p(rules), int(mode), int(m), int(rules.shape[1] - 1), _p(out), int(c_out),
                                      out.element_size(), _stream()), "doda_voxelize_fp_rows")
    return out


def voxelize_bp(d_out, d_feats, rules, mode, n_active, max_active, n_plane):
    _pool_args(d_out, d_feats, rules)
    check(lib().doda_voxelize_bp(_p(d_out), _p(d_feats), _p(rules), int(mode), int(n_active),
                                 int(max_active), int(n_plane), _stream()), "doda_voxelize_bp")


def point_recover_fp(feats, out, rules, n_active, max_active, n_plane):
    _pool_args(feats, out, rules)
    check(lib().doda_point_recover_fp(_p(feats), _p(out), _p(rules), int(n_active),
                                      int(max_active), int(n_plane), _stream()),
          "doda_point_recover_fp")


def point_recover_bp(d_out, d_feats, rules, n_active, max_active, n_plane):
    _pool_args(d_out, d_feats, rules)
    check(lib().doda_point_recover_bp(_p(d_out), _p(d_feats), _p(rules), int(n_active),
                                      int(max_active), int(n_plane), _stream()),
          "doda_point_recover_bp")


# ------------------------------------------------------------------------------------------
# rulebooks
# ------------------------------------------------------------------------------------------
def _shape3(spatial_shape):
    s = [int(v) for v in np.asarray(spatial_shape).reshape(-1)]
    if len(s) != 3:
        raise RuntimeError("spatial_shape must have 3 entries")
    return (C.c_int32 * 3)(*s), s


def _check_indices(indices):
    _need_cuda(indices)
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != 4:
        raise RuntimeError("indices must be int32 [M,4] (batch,x,y,z)")
    return indices.contiguous()


def _rulebook_ws(m, batch_size, shape3, device):
    """Workspace of a rulebook build over the cell map batch_size x shape3, sized by the library's own rule
    (doda_rulebook_workspace_bytes_grid, include/doda_hip.h): with room for the direct-address grid where the build would use
    one, the minimum (hash) workspace otherwise."""
    return _ws(lib().doda_rulebook_workspace_bytes_grid(m, int(batch_size), _shape3(shape3)[0]), device)


def rulebook_subm(indices, spatial_shape, batch_size, ksize=3):
    """Gather table int32 [ksize^3, M] of a SubMConv3d (nbr[o][t] = input row or -1)."""
    indices = _check_indices(indices)
    m = indices.shape[0]
    shape_c, _ = _shape3(spatial_shape)
    K = ksize ** 3
    nbr = torch.empty((K, m), dtype=torch.int32, device=indices.device)
    ws = _rulebook_ws(m, batch_size, _shape3(spatial_shape)[1], indices.device)
    check(lib().doda_rulebook_subm(_p(indices), m, shape_c, int(batch_size), int(ksize), _p(nbr), m,
                                   _p(ws), ws.numel(), _stream()), "doda_rulebook_subm")
    return nbr


def rulebook_down2(indices, spatial_shape, batch_size):
    """SparseConv3d(k=2,s=2) rulebook.  Returns (out_indices int32 [M_out,4], child int32
    [8,M_out], par_off int32 [8,M], out_shape list[3]).  One D2H sync (M_out)."""
    indices = _check_indices(indices)
    m = indices.shape[0]
    dev = indices.device
    shape_c, s = _shape3(spatial_shape)
    out_shape = [(v - 2) // 2 + 1 for v in s]
    parent = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    off = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    out_idx_full = torch.empty((max(m, 1), 4), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)   # always written by the scan
    ws = _rulebook_ws(m, batch_size, out_shape, dev)
    check(lib().doda_rulebook_down2_assign(_p(indices), m, shape_c, int(batch_size), _p(parent),
                                           _p(off), _p(out_idx_full), _p(count), _p(ws), ws.numel(),
                                           _stream()), "doda_rulebook_down2_assign")
    m_out = int(count.item())
    child = torch.empty((8, m_out), dtype=torch.int32, device=dev)
    par_off = torch.empty((8, m), dtype=torch.int32, device=dev)
    check(lib().doda_rulebook_down2_tables(_p(parent), _p(off), m, m_out, _p(child), m_out,
                                           _p(par_off), m, _stream()), "doda_rulebook_down2_tables")
    return out_idx_full[:m_out], child, par_off, out_shape   # a view: no copy launch


def _i3(v):
    v = [v] * 3 if isinstance(v, int) else list(v)
    arr = (C.c_int32 * 3)(*[int(x) for x in v])
    return arr


def rulebook_conv(indices, spatial_shape, batch_size, ksize, stride, padding, dilation):
    """Generic SparseConv3d rulebook (K <= 27).  Returns (out_indices int32 [M_out,4], tbl int32
    [K,M_out], tbl_rev int32 [K,M], out_shape list[3]).  One D2H sync (M_out)."""
    indices = _check_indices(indices)
    m = indices.shape[0]
    dev = indices.device
    shape_c, _ = _shape3(spatial_shape)
    k, s, p, d = _i3(ksize), _i3(stride), _i3(padding), _i3(dilation)
    K = k[0] * k[1] * k[2]
    out_shape_c = (C.c_int32 * 3)()
    count = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib().doda_rulebook_conv_workspace_bytes(m, K)
    if nbytes == 0:
        raise DodaNativeError("doda_rulebook_conv: kernel volume %d or size not supported" % K)
    ws = _ws(nbytes, dev)
    check(lib().doda_rulebook_conv_assign(_p(indices), m, shape_c, int(batch_size), k, s, p, d, out_shape_c,
                                          _p(count), _p(ws), ws.numel(), _stream()), "doda_rulebook_conv_assign")
    m_out = int(count.item())
    out_idx = torch.empty((m_out, 4), dtype=torch.int32, device=dev)
    tbl = torch.empty((K, m_out), dtype=torch.int32, device=dev)
    tbl_rev = torch.empty((K, m), dtype=torch.int32, device=dev)
    check(lib().doda_rulebook_conv_tables(_p(indices), m, shape_c, int(batch_size), k, s, p, d, m_out,
                                          _p(out_idx), _p(tbl), m_out, _p(tbl_rev), m, _p(ws), ws.numel(),
                                          _stream()), "doda_rulebook_conv_tables")
    return out_idx, tbl, tbl_rev, [int(v) for v in out_shape_c]


def rulebook_subm_generic(indices, spatial_shape, batch_size, ksize):
    """SubM neighbour table for per-axis odd kernel sizes (K <= 27): int32 [K, M]."""
    indices = _check_indices(indices)
    m = indices.shape[0]
    shape_c, _ = _shape3(spatial_shape)
    k = _i3(ksize)
    K = k[0] * k[1] * k[2]
    nbr = torch.empty((K, m), dtype=torch.int32, device=indices.device)
    ws = _ws(lib().doda_rulebook_workspace_bytes(m), indices.device)
    check(lib().doda_rulebook_subm_generic(_p(indices), m, shape_c, int(batch_size), k, _p(nbr), m, _p(ws),
                                           ws.numel(), _stream()), "doda_rulebook_subm_generic")
    return nbr


def rulebook_pairs(tbl, n_rows, flip, pad=True, with_seg=False):
    """spconv-v1.2-format (pairs int32 [2,K,n_rows] -1 padded, pairNum int32 [K]) from a table.
    pad=False leaves the entries past pairNum[o] unwritten (lists for the pair-list weight gradient).
    with_seg: also return the lists' segment prefix int32 [K, ceil(n_rows / 256)] (see doda_hip.h)."""
    _need_cuda(tbl)
    K, ld = tbl.shape
    dev = tbl.device
    pairs = torch.empty((2, K, max(n_rows, 1)), dtype=torch.int32, device=dev)
    pair_num = torch.zeros(K, dtype=torch.int32, device=dev)
    nbytes = lib().doda_rulebook_pairs_workspace_bytes(n_rows, K)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev) if with_seg else _ws(nbytes, dev)
    if n_rows == 0:
        if with_seg:
            return pairs[:, :, :0], pair_num, torch.zeros((K, 1), dtype=torch.int32, device=dev)
        return pairs[:, :, :0], pair_num
    check(lib().doda_rulebook_pairs(_p(tbl), ld, K, n_rows, int(bool(flip)) | (0 if pad else 2), _p(pairs), n_rows,
                                    _p(pair_num), _p(ws), ws.numel(), _stream()),
          "doda_rulebook_pairs")
    if with_seg:
        nt = -(-n_rows // lib().doda_rulebook_pairs_tile())
        return pairs, pair_num, ws[:K * nt * 4].view(torch.int32).view(K, nt)
    return pairs, pair_num


# ------------------------------------------------------------------------------------------
# convolution arithmetic
# ------------------------------------------------------------------------------------------
def _feat_ok(x, name):
    _need_cuda(x)
    if x.dim() != 2 or not x.is_contiguous():
        raise RuntimeError("%s must be a contiguous [rows, channels] tensor" % name)


def totals_zeros(nc, device):
    """Zeroed fp64 totals for nc channels in the library's layout (doda_conv_epilogue.stats_totals): [8 slots, 2 sums, nc / 4
    groups, 16] — a 128-byte line per four channels, the first four doubles of a group used."""
    return torch.zeros((STATS_SLOTS, 2, nc // 4, 16), dtype=torch.float64, device=device)


def totals_sums(totals):
    """[2, nc] float64: the totals summed over their slots."""
    return totals[..., :4].sum(0).reshape(2, -1)


def totals_from_rows(rows):
    """The totals that epilogue rows [n, 2, nc] (fp32) add up to, row k in slot k mod 8 (tests)."""
    n, _, nc = rows.shape
    t = totals_zeros(nc, rows.device)
    for k in range(n):
        t[k % STATS_SLOTS, :, :, :4] += rows[k].double().view(2, nc // 4, 4)
    return t


def tilebook_build(tbl, n_rows=None):
    """Tile-local form of a K = 27 gather table (doda_tilebook_build) as a byte tensor, or None when the
    library has no tilebook for this K.  Pass it to spconv_gather(tilebook=...)."""
    _need_cuda(tbl)
    K, ld = tbl.shape
    n_rows = ld if n_rows is None else int(n_rows)
    nbytes = lib().doda_tilebook_bytes(n_rows, K)
    if nbytes == 0:
        return None
    tb = torch.empty(nbytes, dtype=torch.uint8, device=tbl.device)
    check(lib().doda_tilebook_build(_p(tbl), ld, K, n_rows, _p(tb), nbytes, _stream()), "doda_tilebook_build")
    tb._doda_rows = n_rows
    return tb


class GatherCall:
    """A doda_spconv_gather_ex call prepared once (same arguments as spconv_gather; `out` and, with want_stats, the statistics
    buffer are created once and overwritten by every run) and launched by `run()` with ONE native call: the host cost of the
    extension's call sites.  For timing loops over kernels shorter than the Python wrapper (one 150k-voxel scene: 9 us).
    The call is bound to the stream that was current when the object was made and to the tensors it was made with."""

    def __init__(self, *args, **kwargs):
        self.result = spconv_gather(*args, _call=self, **kwargs)

    def run(self):
        check(lib().doda_spconv_gather_ex(*self._args), "doda_spconv_gather_ex")
        return self.result


def spconv_gather(x, w, tbl, n_out, w_layout, nc, out_f32=False, packed=None, residual=None, tilebook=None,
                  want_stats=False, bn=None, out=None, residual_bcast=False, _call=None):
    """y[t] = sum_o x[tbl[o][t]] @ B_o (doda_spconv_gather_ex, the one gather entry point of ABI 7).  x: [n_in,kc]
    f32|bf16; w: fp32 weights viewed [K,kc,nc] (layout 0) or [K,nc,kc] (layouts 1,2), or `packed`: the
    fragment-packed buffer produced by PackPlan for this (weight, layout, dtype).  Returns y [n_out, nc] in x.dtype (or
    float32 when out_f32); with `residual` ([n_out, nc], dtype of y) returns conv + residual.
    want_stats: returns (y, stats [rows, 2, nc] fp32): the BatchNorm partial sums of the epilogue
    (doda_conv_epilogue.stats) — (sum y, sum y^2), or with bn = (bn_x, mean, invstd, gamma, beta, relu) the
    BatchNorm-backward sums of a data-grad call.  want_stats = "totals" (or a totals tensor to accumulate into): the
    sums as fp64 totals instead (ABI 9, doda_conv_epilogue.stats_totals; totals_zeros / totals_sums), returns (y, totals).
    out: write into this tensor instead of allocating."""
    _feat_ok(x, "x")
    _need_cuda(tbl)
    K, ld = tbl.shape
    kc = x.shape[1]
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("spconv_gather: unsupported feature dtype %s" % x.dtype)
    esz = 4 if x.dtype == torch.float32 else 2
    if packed is not None:
        need = lib().doda_spconv_gather_workspace_bytes(K, kc, nc, esz)
        if packed.numel() * packed.element_size() < need - 255:
            raise RuntimeError("packed weight buffer too small")
        w_ptr, ws_ptr, ws_n = _p(packed), None, 0
        layout = int(w_layout) | 0x100
    else:
        _need_cuda(w)
        w = w.contiguous()
        if w.dtype != torch.float32 or w.numel() != K * kc * nc:
            raise RuntimeError("weight must be float32 with K*kc*nc = %d elements" % (K * kc * nc))
        ws = _ws(lib().doda_spconv_gather_workspace_bytes(K, kc, nc, esz), x.device)
        w_ptr, ws_ptr, ws_n, layout = _p(w), _p(ws), ws.numel(), int(w_layout)
    ydt = torch.float32 if (x.dtype == torch.float32 or out_f32) else torch.bfloat16
    if residual is not None:
        _need_cuda(residual)
        want = (nc,) if residual_bcast else (n_out, nc)
        if residual.dtype != ydt or tuple(residual.shape) != want or not residual.is_contiguous():
            raise RuntimeError("residual must be a contiguous [n_out, nc] tensor (or [nc] with residual_bcast) in the output dtype")
    y = out if out is not None else torch.empty((n_out, nc), dtype=ydt, device=x.device)
    ep = _ConvEpilogue()
    ep.residual = _p(residual) if residual is not None else None
    ep.residual_bcast = int(bool(residual_bcast and residual is not None))
    if tilebook is not None:
        ep.tilebook = _p(tilebook)
        ep.tilebook_rows = int(getattr(tilebook, "_doda_rows", n_out))
    stats, rows = None, C.c_int32(0)
    totals = None
    if want_stats == "totals" or torch.is_tensor(want_stats):   # ABI 9: fp64 totals [8, 2, nc] (a tensor: accumulate into it)
        totals = want_stats if torch.is_tensor(want_stats) else totals_zeros(nc, x.device)
        if totals.dtype != torch.float64 or tuple(totals.shape) != (STATS_SLOTS, 2, nc // 4, 16) or not totals.is_contiguous():
            raise RuntimeError("spconv_gather: totals must be a contiguous float64 [8, 2, nc / 4, 16] tensor (totals_zeros)")
        ep.stats_totals = _p(totals)
    if want_stats is not False and want_stats is not None:
        stats = torch.empty((int(lib().doda_spconv_stats_capacity(n_out)) if totals is None else 1, 2, nc), dtype=torch.float32,
                            device=x.device)
        ep.stats, ep.stats_rows_h = _p(stats), C.pointer(rows)
        if bn is not None:
            bx, mean, invstd, gamma, beta, relu = bn
            ep.bn_x, ep.bn_mean, ep.bn_invstd, ep.bn_gamma, ep.bn_beta = _p(bx), _p(mean), _p(invstd), _p(gamma), _p(beta)
            ep.bn_relu = int(bool(relu))
    call_args = (_p(x), x.shape[0], kc, esz, w_ptr, nc, _p(tbl), ld, K, n_out, _p(y),
                 int(bool(out_f32)), layout, ws_ptr, ws_n, C.byref(ep), _stream())
    check(lib().doda_spconv_gather_ex(*call_args), "doda_spconv_gather_ex")
    if _call is not None:   # (GatherCall: everything the native call references stays alive with the object)
        _call._args = call_args
        _call._keep = (x, w, tbl, y, ep, rows, stats, residual, tilebook, bn, packed, ws if packed is None else None, totals)
    if totals is not None:
        return y, totals
    return (y, stats[:rows.value]) if want_stats else y


def bn_fwd_final(stats, m, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None):
    """The reduction half of a training-mode BatchNorm whose statistics rode in a conv epilogue (doda_bn_fwd_final):
    stats [rows, 2, c] fp32 -> (save_mean, save_invstd); running statistics updated in place when given."""
    _need_cuda(stats)
    rows, _, c = stats.shape
    mean = torch.empty(c, dtype=torch.float32, device=stats.device)
    invstd = torch.empty(c, dtype=torch.float32, device=stats.device)
    check(lib().doda_bn_fwd_final(_p(stats), rows, int(m), c, float(eps), float(momentum),
                                  _p(running_mean) if running_mean is not None else None,
                                  _p(running_var) if running_var is not None else None,
                                  _p(num_batches_tracked) if num_batches_tracked is not None else None,
                                  _p(mean), _p(invstd), _stream()), "doda_bn_fwd_final")
    return mean, invstd


class PackPlan:
    """One-launch pre-pack of many weight tensors (doda_spconv_pack_multi).

    entries: list of (w fp32 device tensor viewed [K,*,*], K, kc, nc, layout, elem_bytes).  Output
    buffers and the device descriptor table are created once; run() re-packs everything in a single
    kernel launch (call it whenever the weights changed)."""

    def __init__(self, entries, device):
        import numpy as np
        l = lib()
        n = len(entries)
        dsz = l.doda_spconv_pack_desc_bytes()
        assert dsz == 48
        desc = np.zeros(n, dtype=PACK_DESC)
        self.outputs = []
        for k, (w, K, kc, nc, layout, esz) in enumerate(entries):
            if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == K * kc * nc):
                raise RuntimeError("PackPlan: weights must be contiguous fp32 device tensors")
            out = torch.empty(l.doda_spconv_gather_workspace_bytes(K, kc, nc, esz), dtype=torch.uint8,
                              device=device)
            self.outputs.append(out)   # (the weights are NOT kept alive: the owner re-plans when they die)
            desc[k] = (w.data_ptr(), out.data_ptr(), K, kc, nc, layout, esz, 0, 0, 0)
        blk_end = np.zeros(n, dtype=np.int32)
        total = C.c_int32()
        check(l.doda_spconv_pack_plan_h(desc.ctypes.data, n, blk_end.ctypes.data, C.byref(total)),
              "doda_spconv_pack_plan_h")
        self.n, self.total = n, int(total.value)
        self.desc_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(device)
        self.blk_dev = torch.from_numpy(blk_end).to(device)

    def run(self):
        check(lib().doda_spconv_pack_multi(_p(self.desc_dev), _p(self.blk_dev), self.n, self.total,
                                           _stream()), "doda_spconv_pack_multi")


class WgradPlan:
    """A doda_spconv_wgrad_multi call prepared once (job descriptors, output tensors, workspace, descriptor buffer) and launched
    by `run()` with ONE native call — what the extension's deferred flush costs the host per call.  spconv_wgrad_multi() builds the
    same call in Python every time (~10 us per job): for timing loops over launches shorter than that (one 150k-voxel scene: 60 us
    for eight layers) the wrapper, not the GPU, paces the loop on a busy host.  `outputs` = the dw tensors (overwritten by every run).
    Launches on torch's current stream at run() time; workspace and descriptor buffer belong to the plan (runs must be stream-ordered)."""

    def __init__(self, jobs):
        self.outputs = spconv_wgrad_multi(jobs, _plan=self)

    def run(self):
        check(lib().doda_spconv_wgrad_multi(C.addressof(self._arr), self._n, _p(self._ws), self._ws.numel(), _p(self._desc),
                                            self._desc.numel(), _stream()), "doda_spconv_wgrad_multi")
        return self.outputs


def spconv_wgrad_multi(jobs, _plan=None):
    """Weight gradients of many layers in one native call (doda_spconv_wgrad_multi).
    jobs: list of (a [*,ca], b [n_rows,cb], tbl int32 [K,ld], n_rows[, pairs[, dw[, tilebook]]]); `tilebook` =
    tilebook_build(tbl) (bf16 16 -> 16, K = 27 jobs then take the LDS-staged kernel); `pairs` = None or
    (pair_in int32 [K,ld_p], pair_out int32 [K,ld_p], pair_num int32 [K] | None, seg int32 [K,nt] | None): bf16 jobs with
    16-multiple channel counts then take the pair-list kernel; `dw` = an existing float32 [K,ca,cb] tensor
    to ACCUMULATE into.  Returns the list of dw tensors (float32 [K, ca, cb]), equal to spconv_wgrad per
    job up to the summation order of the partials."""
    if not jobs:
        return []
    arr = (_WgradJob * len(jobs))()
    outs, keep = [], []
    for k, job in enumerate(jobs):
        a, b, tbl, n_rows = job[:4]
        pairs = job[4] if len(job) > 4 else None
        acc_into = job[5] if len(job) > 5 else None
        tilebook = job[6] if len(job) > 6 else None
        _feat_ok(a, "a")
        _feat_ok(b, "b")
        a, b = a.contiguous(), b.contiguous()
        if a.dtype != b.dtype:
            raise RuntimeError("wgrad_multi: a and b must share a dtype")
        if tbl is not None:
            _need_cuda(tbl)
            K, ld = tbl.shape
        else:
            K, ld = pairs[0].shape[0], int(n_rows)
        if acc_into is not None:
            dw = acc_into
            if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.numel() != K * a.shape[1] * b.shape[1]:
                raise RuntimeError("wgrad_multi: the tensor to accumulate into must be contiguous float32 [K,ca,cb]")
        else:
            dw = torch.empty((K, a.shape[1], b.shape[1]), dtype=torch.float32, device=a.device)
        arr[k] = _WgradJob(_p(a), _p(b), _p(tbl), _p(dw), a.shape[1], b.shape[1], ld, K, int(n_rows),
                           4 if a.dtype == torch.float32 else 2,
                           None, None, None, 0, a.shape[0], WGRAD_ACCUMULATE if acc_into is not None else 0, 0,
                           None, 0, 0, _p(tilebook) if tilebook is not None else None)
        if tilebook is not None:
            keep.append(tilebook)
        if pairs is not None:
            pin, pout, pnum = pairs[:3]
            seg = pairs[3] if len(pairs) > 3 else None
            if pin.dtype != torch.int32 or pout.dtype != torch.int32 or pin.stride(-1) != 1 or pout.stride(-1) != 1 \
                    or pin.shape != pout.shape or pin.dim() != 2 or pin.stride(0) != pout.stride(0):
                raise RuntimeError("wgrad_multi: pair lists must be int32 [K, ld] with a unit inner stride")
            arr[k].pair_in, arr[k].pair_out = _p(pin), _p(pout)
            arr[k].pair_num = _p(pnum)
            arr[k].pair_ld = pin.stride(0) if pin.shape[0] > 1 else pin.shape[1]
            if seg is not None:
                if not seg.is_cuda or seg.dtype != torch.int32 or seg.dim() != 2 or seg.shape[0] != K \
                        or not seg.is_contiguous():
                    raise RuntimeError("wgrad_multi: the segment prefix must be a device int32 [K, nt] tensor")
                arr[k].pair_seg, arr[k].pair_seg_nt = _p(seg), seg.shape[1]
            keep.append((pin, pout, pnum, seg))
        outs.append(dw)
        keep.append((a, b))
    dev = outs[0].device
    l = lib()
    ws = _ws(l.doda_spconv_wgrad_multi_workspace_bytes(C.addressof(arr), len(jobs)), dev)
    desc = torch.empty(l.doda_spconv_wgrad_multi_desc_bytes(len(jobs)), dtype=torch.uint8, device=dev)
    check(l.doda_spconv_wgrad_multi(C.addressof(arr), len(jobs), _p(ws), ws.numel(), _p(desc), desc.numel(),
                                    _stream()), "doda_spconv_wgrad_multi")
    if _plan is not None:   # (WgradPlan: everything the native call references stays alive with the plan)
        _plan._arr, _plan._n, _plan._ws, _plan._desc, _plan._keep = arr, len(jobs), ws, desc, (keep, list(jobs))
    return outs


def spconv_wgrad(a, b, tbl, n_rows):
    """dw[o] = sum_t a[tbl[o][t]]^T b[t]  ->  float32 [K, ca, cb] (one job of doda_spconv_wgrad_multi)."""
    _feat_ok(a, "a")
    _feat_ok(b, "b")
    _need_cuda(tbl)
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("spconv_wgrad: a and b must share a dtype (float32 or bfloat16)")
    if n_rows == 0:
        return torch.zeros((tbl.shape[0], a.shape[1], b.shape[1]), dtype=torch.float32, device=a.device)
    return spconv_wgrad_multi([(a, b, tbl, n_rows)])[0]


def spconv_wgrad_pairs(a, b, pair_in, pair_out, pair_num, pair_seg=None, accumulate_into=None):
    """dw[o] (+)= sum_{p < pair_num[o]} a[pair_in[o,p]]^T b[pair_out[o,p]] -> float32 [K, ca, cb]: one pair-list job
    of doda_spconv_wgrad_multi (bf16 operands, channel counts multiples of 16).  pair_num None: every list is full
    (the identity list of a 1x1 convolution).  pair_seg: the lists' segment prefix int32 [K, nt] (third result of
    rulebook_pairs; required whenever pair_num is given)."""
    _feat_ok(a, "a")
    _feat_ok(b, "b")
    _need_cuda(pair_in, pair_out)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.shape[1] % 16 or b.shape[1] % 16:
        raise RuntimeError("spconv_wgrad_pairs: bf16 operands with channel counts that are multiples of 16")
    return spconv_wgrad_multi([(a, b, None, b.shape[0], (pair_in, pair_out, pair_num, pair_seg), accumulate_into)])[0]


def maxpool_fwd(x, tbl, n_out):
    _feat_ok(x, "x")
    K, ld = tbl.shape
    y = torch.empty((n_out, x.shape[1]), dtype=torch.float32, device=x.device)
    check(lib().doda_maxpool_fwd_f32(_p(x), x.shape[1], _p(tbl), ld, K, n_out, _p(y), _stream()),
          "doda_maxpool_fwd_f32")
    return y


def maxpool_bwd(x, y, dy, tbl, n_out):
    K, ld = tbl.shape
    dx = torch.zeros_like(x)
    check(lib().doda_maxpool_bwd_f32(_p(x), _p(y), _p(dy), x.shape[1], _p(tbl), ld, K, n_out,
                                     _p(dx), _stream()), "doda_maxpool_bwd_f32")
    return dx


# ------------------------------------------------------------------------------------------
# fused BatchNorm(+ReLU)
# ------------------------------------------------------------------------------------------
def _esz(t):
    if t.dtype == torch.float32:
        return 4
    if t.dtype == torch.bfloat16:
        return 2
    raise RuntimeError("unsupported feature dtype %s" % t.dtype)


def _bn_bwd_out(x):
    """An [m, c] tensor like x and two fp32 [c] vectors: (dx, dgamma, dbeta) of a backward, (y, save_mean, save_invstd) of a
    training-mode forward."""
    c = x.shape[1]
    return (torch.empty_like(x), torch.empty(c, dtype=torch.float32, device=x.device),
            torch.empty(c, dtype=torch.float32, device=x.device))


def _add_ld(add, m, c, what):
    """(pointer, row stride in elements) of the second-gradient operand: dense, or a column slice of a wider matrix."""
    _need_cuda(add)
    if add.dim() != 2 or tuple(add.shape) != (m, c) or add.stride(1) != 1 or add.stride(0) < c:
        raise RuntimeError("%s: add must be [m, c] with unit column stride" % what)
    return _p(add), int(add.stride(0))


def _bn_bwd_args(what, x, dy, add=None, also=()):
    """Operand checks of a BatchNorm backward -> (m, c, add's pointer or None, add's row stride in elements)."""
    _feat_ok(x, "x")
    _feat_ok(dy, "dy")
    _need_cuda(*also)
    m, c = x.shape
    ap, ld = _add_ld(add, m, c, what) if add is not None else (None, c)
    return m, c, ap, ld


def bn_relu_fwd(x, gamma, beta, running_mean, running_var, training, momentum, eps, relu,
                num_batches_tracked=None):
    """-> (y, save_mean, save_invstd).  x: contiguous [m, c] fp32|bf16 on device, c % 4 == 0."""
    _feat_ok(x, "x")
    m, c = x.shape
    if training:
        y, save_mean, save_invstd = _bn_bwd_out(x)
    else:
        y = torch.empty_like(x)
        save_mean = running_mean.float().contiguous()
        save_invstd = torch.rsqrt(running_var.float() + eps).contiguous()
    ws = _ws(lib().doda_bn_workspace_bytes(m, c), x.device)
    rm, rv, nbt = (running_mean, running_var, num_batches_tracked) if training else (None, None, None)
    check(lib().doda_bn_relu_fwd(_p(x), m, c, _esz(x), float(eps), float(momentum), _p(gamma), _p(beta),
                                 _p(rm), _p(rv), _p(nbt), int(bool(training)), int(bool(relu)), _p(y), _p(save_mean),
                                 _p(save_invstd), _p(ws), ws.numel(), _stream()), "doda_bn_relu_fwd")
    return y, save_mean, save_invstd


def bn_relu_bwd(x, dy, save_mean, save_invstd, gamma, beta, relu):
    """-> (dx, dgamma, dbeta) for the training-mode forward above."""
    m, c, _, _ = _bn_bwd_args("bn_relu_bwd", x, dy)
    dx, dgamma, dbeta = _bn_bwd_out(x)
    ws = _ws(lib().doda_bn_workspace_bytes(m, c), x.device)
    check(lib().doda_bn_relu_bwd(_p(x), _p(dy), m, c, _esz(x), _p(save_mean), _p(save_invstd),
                                 _p(gamma), _p(beta), int(bool(relu)), _p(dx), _p(dgamma), _p(dbeta),
                                 _p(ws), ws.numel(), _stream()), "doda_bn_relu_bwd")
    return dx, dgamma, dbeta


def bn_relu_bwd_add(x, dy, save_mean, save_invstd, gamma, beta, relu, add):
    """bn_relu_bwd with a second gradient of x summed into dx inside the apply pass (doda_bn_relu_bwd_add); `add`
    may be a column slice of a wider matrix (e.g. g[:, :c] of torch.cat's gradient): no copy is made."""
    m, c, _, _ = _bn_bwd_args("bn_relu_bwd_add", x, dy)
    ap, ld = _add_ld(add, m, c, "bn_relu_bwd_add")      # (not optional here)
    dx, dgamma, dbeta = _bn_bwd_out(x)
    ws = _ws(lib().doda_bn_workspace_bytes(m, c), x.device)
    check(lib().doda_bn_relu_bwd_add(_p(x), _p(dy), m, c, _esz(x), _p(save_mean), _p(save_invstd), _p(gamma), _p(beta),
                                        int(bool(relu)), ap, ld, _p(dx), _p(dgamma), _p(dbeta), _p(ws), ws.numel(),
                                        _stream()), "doda_bn_relu_bwd_add")
    return dx, dgamma, dbeta


def bn_relu_bwd_stats(x, dy, stats, save_mean, save_invstd, gamma, beta, relu, add=None):
    """BatchNorm(+ReLU) backward over the (sum dz, sum dz * xhat) rows of a data-grad conv epilogue
    (doda_bn_relu_bwd_stats); add as in bn_relu_bwd_add.  -> (dx [+ add], dgamma, dbeta)."""
    m, c, ap, ld = _bn_bwd_args("bn_relu_bwd_stats", x, dy, add, also=(stats,))
    dx, dgamma, dbeta = _bn_bwd_out(x)
    coef = torch.empty(3 * c, dtype=torch.float32, device=x.device)
    check(lib().doda_bn_relu_bwd_stats(_p(x), _p(dy), m, c, _esz(x), _p(stats), stats.shape[0], _p(save_mean),
                                          _p(save_invstd), _p(gamma), _p(beta), int(bool(relu)), ap, ld, _p(dx), _p(dgamma),
                                          _p(dbeta), _p(coef), _stream()), "doda_bn_relu_bwd_stats")
    return dx, dgamma, dbeta


def bn_relu_fwd_totals(x, totals, gamma, beta, running_mean, running_var, momentum, eps, relu, num_batches_tracked=None,
                       totals_b=None):
    """Training-mode BatchNorm(+ReLU) over the fp64 totals of conv epilogues (doda_bn_relu_fwd_totals, ONE launch);
    totals_b: totals of the producer of the trailing columns (a channel concatenation).  -> (y, save_mean, save_invstd)."""
    _feat_ok(x, "x")
    _need_cuda(totals)
    m, c = x.shape
    c_a = int(totals.shape[2]) * 4
    y, save_mean, save_invstd = _bn_bwd_out(x)
    check(lib().doda_bn_relu_fwd_totals(_p(x), m, c, _esz(x), _p(totals), _p(totals_b), c_a, float(eps), float(momentum),
                                        _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(num_batches_tracked),
                                        int(bool(relu)), _p(y), _p(save_mean), _p(save_invstd), _stream()),
          "doda_bn_relu_fwd_totals")
    return y, save_mean, save_invstd


def bn_relu_bwd_totals(x, dy, totals, save_mean, save_invstd, gamma, beta, relu, add=None):
    """BatchNorm(+ReLU) backward over the fp64 totals of a data-grad conv epilogue (doda_bn_relu_bwd_totals, ONE launch).
    -> (dx [+ add], dgamma, dbeta)."""
    m, c, ap, ld = _bn_bwd_args("bn_relu_bwd_totals", x, dy, add, also=(totals,))
    dx, dgamma, dbeta = _bn_bwd_out(x)
    check(lib().doda_bn_relu_bwd_totals(_p(x), _p(dy), m, c, _esz(x), _p(totals), _p(save_mean), _p(save_invstd), _p(gamma),
                                        _p(beta), int(bool(relu)), ap, ld, _p(dx), _p(dgamma), _p(dbeta), _stream()),
          "doda_bn_relu_bwd_totals")
    return dx, dgamma, dbeta


def cast_colsum(x):
    """(x.bfloat16(), x.sum(0)) of a device fp32 [n, c <= 64] matrix in one pass (doda_cast_colsum_f32_bf16)."""
    _feat_ok(x, "x")
    n, c = x.shape
    y = torch.empty((n, c), dtype=torch.bfloat16, device=x.device)
    nb = int(lib().doda_cast_colsum_blocks(n, c))
    if x.dtype != torch.float32 or nb == 0:
        raise RuntimeError("cast_colsum: fp32 [n, c <= 64]")
    partial = torch.empty((nb, c), dtype=torch.float32, device=x.device)
    check(lib().doda_cast_colsum_f32_bf16(_p(x), n, c, _p(y), _p(partial), nb, _stream()), "doda_cast_colsum_f32_bf16")
    return y, partial.sum(0)


def pad_channels(x, c_out):
    """x [n, c_in] (fp32 / bf16, contiguous) zero-padded to c_out channels in one kernel (doda_pad_channels)."""
    _feat_ok(x, "x")
    n, c_in = x.shape
    y = torch.empty((n, c_out), dtype=x.dtype, device=x.device)
    check(lib().doda_pad_channels(_p(x), n, c_in, c_out, _esz(x), _p(y), _stream()), "doda_pad_channels")
    return y


# ------------------------------------------------------------------------------------------
# neighbour queries
# ------------------------------------------------------------------------------------------
def knnquery(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    """pointops2_cuda.knnquery_cuda signature (offset/new_offset are END offsets, int32)."""
    _need_cuda(xyz, new_xyz, offset, new_offset, idx, dist2)
    check(lib().doda_knnquery(int(m), int(nsample), _p(xyz), _p(new_xyz), _p(offset),
                              _p(new_offset), int(offset.numel()), _p(idx), _p(dist2), _stream()),
          "doda_knnquery")


def knn_batch(xyz, query_xyz, batch_idxs, query_batch_offsets, idx, n, m, k):
    _need_cuda(xyz, query_xyz, batch_idxs, query_batch_offsets, idx)
    check(lib().doda_knn_batch(int(n), int(m), int(k), _p(xyz), _p(query_xyz), _p(batch_idxs),
                               _p(query_batch_offsets), _p(idx), _stream()), "doda_knn_batch")


def ballquery_batch_p(xyz, batch_idxs, batch_offsets, idx, start_len, n, mean_active, radius):
    _need_cuda(xyz, batch_idxs, batch_offsets, idx, start_len)
    ws = _ws(lib().doda_ballquery_workspace_bytes(int(n)), xyz.device)
    total = C.c_int32(0)
    check(lib().doda_ballquery_batch_p(int(n), int(mean_active), float(radius), _p(xyz),
                                       _p(batch_idxs), _p(batch_offsets), _p(idx), _p(start_len),
                                       C.byref(total), _p(ws), ws.numel(), _stream()),
          "doda_ballquery_batch_p")
    return int(total.value)


# ------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------
def seg_meters(hist, preds, labels, n_classes, ignore_index, p2v=None):
    """hist int64 [3, k] += (intersection, prediction area, target area) of the points (doda_seg_meters; reference
    util/common_utils.py:233-246).  preds: int32 / int64 class per point, or per VOXEL with p2v (int32 [N]) mapping points to voxels."""
    _need_cuda(preds)
    _need_cuda(labels)
    if (hist.dtype != torch.int64 or not hist.is_contiguous() or tuple(hist.shape) != (3, int(n_classes)) or labels.dtype != torch.int64
            or preds.dtype not in (torch.int32, torch.int64) or (p2v is not None and p2v.dtype != torch.int32)):
        raise RuntimeError("seg_meters: hist int64 [3,k], labels int64 [N], preds int32|int64, p2v int32")
    preds, labels = preds.contiguous(), labels.contiguous()
    if p2v is not None:
        _need_cuda(p2v)
        p2v = p2v.contiguous()
    n = labels.shape[0]
    if (p2v.shape[0] if p2v is not None else preds.shape[0]) != n:
        raise RuntimeError("seg_meters: one prediction (or one p2v entry) per label")
    check(lib().doda_seg_meters(_p(preds), 1 if preds.dtype == torch.int64 else 0, _p(p2v) if p2v is not None else None, _p(labels),
                                n, int(n_classes), int(ignore_index), _p(hist), _stream()), "doda_seg_meters")
    return hist


def cross_entropy_fwd(logits, labels, ignore_index):
    """-> (out float32 [2] = {mean loss over valid points, n_valid}, lse float32 [N])."""
    _need_cuda(logits)
    _need_cuda(labels)
    if logits.dtype != torch.float32 or labels.dtype != torch.int64 or logits.dim() != 2:
        raise RuntimeError("cross_entropy: logits float32 [N,C], labels int64 [N]")
    logits, labels = logits.contiguous(), labels.contiguous()
    n, c = logits.shape
    lse = torch.empty(n, dtype=torch.float32, device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    ws = _ws(lib().doda_cross_entropy_workspace_bytes(n), logits.device)
    check(lib().doda_cross_entropy_fwd(_p(logits), _p(labels), n, c, int(ignore_index), _p(lse), _p(out), _p(ws),
                                       ws.numel(), _stream()), "doda_cross_entropy_fwd")
    return out, lse


def cross_entropy_bwd(logits, labels, lse, out, grad, ignore_index):
    n, c = logits.shape
    d = torch.empty_like(logits)
    check(lib().doda_cross_entropy_bwd(_p(logits), _p(labels), _p(lse), _p(out), _p(grad), n, c, int(ignore_index),
                                       _p(d), _stream()), "doda_cross_entropy_bwd")
    return d


# ---- point head + loss at voxel level (ABI 11, csrc/head.hip) -----------------------------------------------------
def _head_args(what, feats, weight, bias, v2p=None, labels=None):
    """The operands of a voxel-level head call, checked and contiguous: (feats, weight, bias, v2p, labels); v2p and labels None for
    an entry point that takes no point lists (voxel_confidence)."""
    _feat_ok(feats, "feats")
    lists = v2p is not None
    _need_cuda(weight, *((v2p, labels) if lists else ()))
    if weight.dtype != torch.float32 or (lists and (v2p.dtype != torch.int32 or labels.dtype != torch.int64 or v2p.dim() != 2)):
        raise RuntimeError("%s: weight float32 [n_cls, c]%s" % (what, ", v2p int32 [m, 1 + max_active], labels int64 [points]" if lists else ""))
    cont = lambda t: t.contiguous() if t is not None else None
    return feats.contiguous(), weight.contiguous(), cont(bias), cont(v2p), cont(labels)


def _head_bwd(blocks, feats, weight, bias, want_lo, launch):
    """A backward sweep into outputs allocated here: launch(the native call's leading arguments (feats .. n_cls), d_feats, dz, dz_lo,
    db_partial, n_blocks).  -> (d_feats, dz, dz_lo or None, d_bias float32 [n_cls] = the workgroups' rows summed)."""
    feats, weight = feats.contiguous(), weight.contiguous()
    (m, c), n_cls = feats.shape, weight.shape[0]
    nb = int(blocks(m))
    d_feats = torch.empty_like(feats)
    dz = torch.empty((m, n_cls), dtype=feats.dtype, device=feats.device)
    dz_lo = torch.empty_like(dz) if want_lo else None
    dbp = torch.empty((nb, n_cls), dtype=torch.float32, device=feats.device)
    launch((_p(feats), m, c, feats.element_size(), _p(weight), _p(bias.contiguous() if bias is not None else None), n_cls),
           d_feats, dz, dz_lo, dbp, nb)
    return d_feats, dz, dz_lo, dbp.sum(0)


def head_ce_fwd(feats, weight, bias, v2p, labels, ignore_index, want_pred=True):
    """Linear head + cross-entropy over the voxel -> point lists without the [points, classes] matrix (doda_head_ce_fwd).
    -> (out float32 [2] = {mean loss over the valid points, n_valid}, pred int32 [m] = argmax class per voxel or None)."""
    feats, weight, bias, v2p, labels = _head_args("head_ce", feats, weight, bias, v2p, labels)
    m, c = feats.shape
    nb = int(lib().doda_head_ce_blocks(m))
    out = torch.empty(2, dtype=torch.float32, device=feats.device)
    pred = torch.empty(m, dtype=torch.int32, device=feats.device) if want_pred else None
    ws = torch.empty(2 * nb, dtype=torch.float32, device=feats.device)
    check(lib().doda_head_ce_fwd(_p(feats), m, c, feats.element_size(), _p(weight), _p(bias), weight.shape[0], _p(v2p), v2p.shape[1],
                                 _p(labels), int(ignore_index), _p(out), _p(pred), _p(ws), nb, _stream()), "doda_head_ce_fwd")
    return out, pred


def head_ce_bwd(feats, weight, bias, v2p, labels, ignore_index, out, grad):
    """-> (d_feats [m, c], dz [m, n_cls] — both in the features' dtype —, d_bias float32 [n_cls])."""
    v2p, labels = v2p.contiguous(), labels.contiguous()
    d_feats, dz, _, d_b = _head_bwd(lib().doda_head_ce_blocks, feats, weight, bias, False, lambda head, d_feats, dz, dz_lo, dbp, nb: check(
        lib().doda_head_ce_bwd(*head, _p(v2p), v2p.shape[1], _p(labels), int(ignore_index), _p(out), _p(grad.contiguous()), _p(d_feats),
                               _p(dz), _p(dbp), nb, _stream()), "doda_head_ce_bwd"))
    return d_feats, dz, d_b


def head_dw(feats, dz):
    """d weight [n_cls, c] of the voxel-level head from feats [m, c] and dz [m, n_cls]: the bf16 MFMA kernel (doda_head_dw_bf16) or,
    fp32, the library's weight gradient over an identity table."""
    m, c = feats.shape
    n_cls = dz.shape[1]
    if feats.dtype == torch.bfloat16 and c == 16 and n_cls <= 32:
        nb = int(lib().doda_head_dw_blocks(m))
        part = torch.empty((nb, 32, 16), dtype=torch.float32, device=feats.device)
        check(lib().doda_head_dw_bf16(_p(feats.contiguous()), _p(dz.contiguous()), m, c, n_cls, _p(part), nb, _stream()), "doda_head_dw_bf16")
        return part.sum(0)[:n_cls]
    ident = torch.arange(m, dtype=torch.int32, device=feats.device).view(1, m)
    return spconv_wgrad(feats.contiguous(), dz, ident, m)[0].t()


def head_grads(needs, feats, weight, bias, d_feats, dz, dz_lo, d_b):
    """The gradients a voxel-level head function (model._VoxelHeadCE, lovasz._VoxelHeadLovasz: feats, weight, bias, v2p, labels,
    ignore_index) returns, from its backward sweep's outputs and needs = ctx.needs_input_grad: dW = dz^T feats through head_dw, plus
    the same on dz_lo where the sweep wrote one (bf16: what rounding dz dropped)."""
    d_w = None
    if needs[1]:
        d_w = head_dw(feats, dz)
        if dz_lo is not None:
            d_w = d_w + head_dw(feats, dz_lo)
        d_w = d_w.to(weight.dtype)
    return (d_feats if needs[0] else None), d_w, (d_b if bias is not None and needs[2] else None), None, None, None


# ---- Lovasz-softmax head at voxel level (include/doda_loss.h, csrc/lovasz.hip) -------------------------------------
def lovasz_fwd(feats, weight, bias, v2p, labels, ignore_index, want_grad=True):
    """Linear head + Lovasz-softmax (classes present) over the voxel -> point lists without the [points, classes] matrix
    (doda_lovasz_fwd).  -> (out float32 [2] = {loss, present classes}, pred int32 [m], gitem float32 [m, n_cls, 2] or None: the
    per-item Lovasz gradients doda_lovasz_bwd reads)."""
    feats, weight, bias, v2p, labels = _head_args("lovasz", feats, weight, bias, v2p, labels)
    m, c = feats.shape
    n_cls = weight.shape[0]
    out = torch.empty(2, dtype=torch.float32, device=feats.device)
    pred = torch.empty(m, dtype=torch.int32, device=feats.device)
    gitem = torch.empty((m, n_cls, 2), dtype=torch.float32, device=feats.device) if want_grad else None
    nbytes = int(lib().doda_lovasz_workspace_bytes(m, n_cls))
    if nbytes == 0:
        raise DodaNativeError("doda_lovasz_fwd: %d voxels x %d classes is outside the compiled range" % (m, n_cls))
    ws = _ws(nbytes, feats.device)
    check(lib().doda_lovasz_fwd(_p(feats), m, c, feats.element_size(), _p(weight), _p(bias), n_cls, _p(v2p), v2p.shape[1], _p(labels),
                                int(ignore_index), _p(out), _p(pred), _p(gitem), _p(ws), ws.numel(), _stream()), "doda_lovasz_fwd")
    return out, pred, gitem


def lovasz_bwd(feats, weight, bias, gitem, out, grad):
    """-> (d_feats [m, c], dz [m, n_cls] — both in the features' dtype —, dz_lo [m, n_cls] bf16 = what rounding dz to bf16 dropped
    (None for fp32 features), d_bias float32 [n_cls])."""
    return _head_bwd(lib().doda_lovasz_blocks, feats, weight, bias, feats.dtype == torch.bfloat16, lambda head, d_feats, dz, dz_lo, dbp, nb: check(
        lib().doda_lovasz_bwd(*head, _p(gitem), _p(out), _p(grad.contiguous()), _p(d_feats), _p(dz), _p(dz_lo), _p(dbp), nb, _stream()),
        "doda_lovasz_bwd"))


# ---- self-training pseudo labels (include/doda_selftrain.h) --------------------------------------------
def voxel_confidence(feats, weight, bias):
    """(pred int32 [m], conf float32 [m]) of the Linear head on the voxel rows: the argmax class (bit-identical to head_ce_fwd's
    pred) and its softmax probability 1 / sum_k exp(z_k - z_max) (doda_st_voxel_confidence).  feats bf16 / fp32 [m, 16 | 32]."""
    feats, weight, bias, _, _ = _head_args("voxel_confidence", feats, weight, bias)
    if weight.dim() != 2 or weight.shape[1] != feats.shape[1]:
        raise RuntimeError("voxel_confidence: weight float32 [n_cls, c]")
    if bias is not None:
        _need_cuda(bias)
        if bias.dtype != torch.float32 or bias.numel() != weight.shape[0]:
            raise RuntimeError("voxel_confidence: bias float32 [n_cls]")
    m, c = feats.shape
    pred = torch.empty(m, dtype=torch.int32, device=feats.device)
    conf = torch.empty(m, dtype=torch.float32, device=feats.device)
    check(lib().doda_st_voxel_confidence(_p(feats), m, c, feats.element_size(), _p(weight), _p(bias), weight.shape[0], _p(pred),
                                         _p(conf), _stream()), "doda_st_voxel_confidence")
    return pred, conf


def st_point_store(pred, conf, p2v, store_cls, store_conf, offset, n_cls, hist=None):
    """store_cls / store_conf[offset + i] = pred / conf[p2v[i]] for every point i (doda_st_point_store); hist: int64 [n_cls, 256]
    to ADD the level-0 radix histogram of those points to, or None."""
    for t in (pred, conf, p2v, store_cls, store_conf):
        _need_cuda(t)
    if (pred.dtype != torch.int32 or conf.dtype != torch.float32 or p2v.dtype != torch.int32 or store_cls.dtype != torch.uint8
            or store_conf.dtype != torch.float32 or store_cls.shape != store_conf.shape or pred.shape != conf.shape):
        raise RuntimeError("st_point_store: pred int32 / conf float32 [m], p2v int32 [n], store uint8 / float32 [len]")
    for t in (pred, conf, p2v, store_cls, store_conf):
        if not t.is_contiguous():
            raise RuntimeError("st_point_store: contiguous tensors only")
    if hist is not None:
        _need_cuda(hist)
        if hist.dtype != torch.int64 or hist.shape != (n_cls, 256) or not hist.is_contiguous():
            raise RuntimeError("st_point_store: hist int64 [n_cls, 256]")
    check(lib().doda_st_point_store(_p(pred), _p(conf), pred.numel(), _p(p2v), p2v.numel(), int(n_cls), _p(store_cls), _p(store_conf),
                                    store_cls.numel(), int(offset), _p(hist), _stream()), "doda_st_point_store")


def st_radix_hist(store_cls, store_conf, n_cls, level, prefix=None):
    """int64 [n_cls, 256]: radix level `level` of the stored confidences per class, restricted to the keys whose higher bits equal
    prefix[c] (int32 device tensor [n_cls]; -1 = class done; unused at level 0) (doda_st_radix_hist)."""
    _need_cuda(store_cls, store_conf)
    if store_cls.dtype != torch.uint8 or store_conf.dtype != torch.float32 or store_cls.shape != store_conf.shape:
        raise RuntimeError("st_radix_hist: store uint8 / float32 [len]")
    if prefix is not None:
        _need_cuda(prefix)
        if prefix.dtype != torch.int32 or prefix.numel() != n_cls:
            raise RuntimeError("st_radix_hist: prefix int32 [n_cls]")
    hist = torch.zeros((n_cls, 256), dtype=torch.int64, device=store_cls.device)
    check(lib().doda_st_radix_hist(_p(store_cls.contiguous()), _p(store_conf.contiguous()), store_cls.numel(), int(n_cls), int(level),
                                   _p(prefix.contiguous()) if prefix is not None else None, _p(hist), _stream()), "doda_st_radix_hist")
    return hist


def st_label(store_cls, store_conf, thres32, ignore):
    """(labels uint8 [len], kept int64 [n_cls]): labels = conf > thres32[cls] ? cls : ignore, kept = points kept per class
    (doda_st_label).  thres32: float32 device tensor [n_cls] of strict lower bounds."""
    _need_cuda(store_cls, store_conf, thres32)
    if store_cls.dtype != torch.uint8 or store_conf.dtype != torch.float32 or thres32.dtype != torch.float32:
        raise RuntimeError("st_label: store uint8 / float32 [len], thres float32 [n_cls]")
    n_cls = thres32.numel()
    labels = torch.empty(store_cls.shape, dtype=torch.uint8, device=store_cls.device)
    kept = torch.zeros(n_cls, dtype=torch.int64, device=store_cls.device)
    check(lib().doda_st_label(_p(store_cls.contiguous()), _p(store_conf.contiguous()), store_cls.numel(), n_cls,
                              _p(thres32.contiguous()), int(ignore), _p(labels), _p(kept), _stream()), "doda_st_label")
    return labels, kept


# ---- training subsample (include/doda_subsample.h, csrc/subsample.hip) ----------------------------------------------
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _mulhilo32(a, b):
    """(high, low) 32-bit halves of the constant a times the int64 tensor b (values below 2^32), in int64 arithmetic."""
    p0, p1 = a * (b & 0xFFFF), a * (b >> 16)
    t = p1 + (p0 >> 16)
    return t >> 16, ((t & 0xFFFF) << 16) | (p0 & 0xFFFF)


def subsample_keys(seed, n, device, key_mask=0xffffffff):
    """int64 [n]: the keys of points 0 .. n - 1 under `seed` — csrc/subsample_key.hpp (Philox-4x32-10, counter (j, 0, 0, 0), key =
    the seed's two halves, output word 0) restated with torch integer ops on any device."""
    c0 = torch.arange(n, dtype=torch.int64, device=device)
    c1, c2, c3 = torch.zeros_like(c0), torch.zeros_like(c0), torch.zeros_like(c0)
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & 0xffffffff, (k1 + _PHILOX_W1) & 0xffffffff
    return c0 & int(key_mask)


def _subsample_args(xyz, labels, offsets, ks, seeds):
    offsets, ks, seeds = [int(v) for v in offsets], [int(v) for v in ks], [int(v) & 0xffffffffffffffff for v in seeds]
    n_seg = len(offsets) - 1
    if n_seg < 1 or len(ks) != n_seg or len(seeds) != n_seg:
        raise RuntimeError("subsample: n_seg + 1 offsets, n_seg counts, n_seg seeds")
    if (xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or labels.dtype != torch.int32
            or labels.shape != (xyz.shape[0],) or offsets[-1] != xyz.shape[0] or labels.device != xyz.device):
        raise RuntimeError("subsample: xyz float32 [N, 3], labels int32 [N], offsets[-1] = N")
    offsets_s = [0]
    for k in ks:
        offsets_s.append(offsets_s[-1] + k)
    return offsets, ks, seeds, n_seg, offsets_s


def subsample_torch(xyz, labels, offsets, ks, seeds, key_mask=0xffffffff):
    """subsample() with torch ops on the tensors' device (any device): the same outputs bit for bit.  Per segment one sort of
    key * 2^31 + index, the first k indices sorted again."""
    offsets, ks, seeds, n_seg, offsets_s = _subsample_args(xyz, labels, offsets, ks, seeds)
    picks = []
    for b in range(n_seg):
        n = offsets[b + 1] - offsets[b]
        if not 0 <= ks[b] <= n:
            raise RuntimeError("subsample: 0 <= k <= points of the segment")
        order = (subsample_keys(seeds[b], n, xyz.device, key_mask) << 31) | torch.arange(n, dtype=torch.int64, device=xyz.device)
        picks.append(torch.sort(torch.sort(order)[0][:ks[b]] & 0x7fffffff)[0])
    sub = torch.cat(picks)
    rows = sub + torch.cat([torch.full((k,), offsets[b], dtype=torch.int64, device=xyz.device) for b, k in enumerate(ks)])
    return xyz.index_select(0, rows), labels.index_select(0, rows), sub.to(torch.int32), offsets_s


def subsample(xyz, labels, offsets, ks, seeds, key_mask=0xffffffff):
    """The random subsample of every scene of a batch (reference dataset/dataset.py:73-77), one native call on the current stream
    (doda_subsample_draw).  xyz float32 [N, 3], labels int32 [N]; offsets: the n_seg + 1 scene offsets, ks: points to keep per
    scene, seeds: one 64-bit seed per scene (host lists).  Scene b keeps the ks[b] points smallest in (key(seed_b, j) & key_mask, j),
    in ascending j.  -> (xyz_s [K, 3], labels_s [K], sub_idx int32 [K] (index inside the scene), offsets_s (host list)).  The
    workspace is the cached per-stream buffer.  CPU tensors: subsample_torch, the same outputs bit for bit."""
    if not xyz.is_cuda:
        return subsample_torch(xyz, labels, offsets, ks, seeds, key_mask)
    offsets, ks, seeds, n_seg, offsets_s = _subsample_args(xyz, labels, offsets, ks, seeds)
    xyz, labels = xyz.contiguous(), labels.contiguous()
    off_h, k_h, seeds_h = (C.c_int64 * (n_seg + 1))(*offsets), (C.c_int32 * n_seg)(*ks), (C.c_uint64 * n_seg)(*seeds)
    total = offsets_s[-1]
    out_xyz = torch.empty((total, 3), dtype=torch.float32, device=xyz.device)
    out_labels = torch.empty(total, dtype=torch.int32, device=xyz.device)
    out_idx = torch.empty(total, dtype=torch.int32, device=xyz.device)
    nbytes = lib().doda_subsample_workspace_bytes(off_h, n_seg)
    ws = _ws(nbytes, xyz.device)
    check(lib().doda_subsample_draw(_p(xyz), _p(labels), None, None, off_h, n_seg, k_h, seeds_h, int(key_mask) & 0xffffffff, _p(out_xyz),
                                    _p(out_labels), _p(out_idx), None, None, _p(ws), ws.numel(), _stream()), "doda_subsample_draw")
    return out_xyz, out_labels, out_idx, offsets_s


# ---- optimizer step -------------------------------------------------------------------------------
# ---- full-cloud evaluation (include/doda_eval.h, csrc/eval.hip) ---------------------------------------------------
class EvalTable:
    """The cell table of a batch's processed points (include/doda_eval.h): `scenes` (ctypes array of doda_eval_scene, m_end still
    unset), the device tensors order / xyz_sorted / cell_start and the per-scene grid tensors the keys were made from."""

    def __init__(self, scenes, ends, order, xyz_sorted, cell_start, grid):
        self.scenes, self.ends, self.order, self.xyz_sorted, self.cell_start, self.grid = scenes, ends, order, xyz_sorted, cell_start, grid


def _eval_ends(offset, total, what):
    ends = [int(v) for v in offset.cpu().tolist()]
    if not ends or any(b < a for a, b in zip([0] + ends[:-1], ends)) or ends[-1] != total:
        raise RuntimeError("%s: END offsets, non-decreasing, the last one the row count" % what)
    return ends


def _eval_batch_index(ends, device):
    sizes = [e - s for s, e in zip([0] + ends[:-1], ends)]
    return torch.repeat_interleave(torch.arange(len(sizes), device=device), torch.tensor(sizes, device=device), output_size=ends[-1])


def _eval_keys(xyz, bidx, grid):
    """int64 [rows]: the cell id of every point — per axis clamp(floor((x - origin) * inv_side), 0, dims - 1) in fp32, the
    expression eval.hip's eval_cell restates (one rounded subtraction, one rounded multiplication), then cell_base + (cx ny + cy) nz + cz."""
    origin, inv, dims, base = grid
    c = ((xyz - origin[bidx]) * inv[bidx][:, None]).floor()
    c = torch.nan_to_num(c, nan=0.0, posinf=3.0e38, neginf=-3.0e38).clamp(min=0.0)
    d = dims[bidx]
    c = torch.minimum(c, (d - 1).to(torch.float32)).to(torch.int64)
    return base[bidx] + (c[:, 0] * d[:, 1] + c[:, 1]) * d[:, 2] + c[:, 2]


def eval_table(xyz, offset, cell_side, max_cells=None):
    """The cell table of the processed points xyz float32 [n, 3] with END offsets int32 [B] (device tensors), built with torch on the
    device: per scene a grid from its bounding box with cells of `cell_side` metres — doubled on the host until the scene's grid has
    at most max_cells (DODA_EVAL_MAX_CELLS) cells —, a stable sort of the cell ids, bincount and cumsum.  One read-back (the offsets
    and the per-scene bounds)."""
    from ._lib import EVAL_MAX_CELLS, EVAL_MAX_SCENES, EvalScene
    _need_cuda(xyz, offset)
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or offset.dtype != torch.int32 or not float(cell_side) > 0.0:
        raise RuntimeError("eval_table: xyz float32 [n, 3], offset int32 [B], cell_side > 0")
    max_cells = EVAL_MAX_CELLS if max_cells is None else min(int(max_cells), EVAL_MAX_CELLS)
    xyz = xyz.contiguous()
    n, dev = xyz.shape[0], xyz.device
    ends = _eval_ends(offset, n, "eval_table")
    nb = len(ends)
    if nb > EVAL_MAX_SCENES:
        raise DodaNativeError("eval_table: %d scenes in one batch (at most %d)" % (nb, EVAL_MAX_SCENES))
    starts = [0] + ends[:-1]
    bounds = torch.stack([torch.cat((xyz[s:e].amin(0), xyz[s:e].amax(0))) if e > s else xyz.new_zeros(6)
                          for s, e in zip(starts, ends)]).cpu().numpy()
    if not np.isfinite(bounds).all():
        raise RuntimeError("eval_table: non-finite coordinates")
    scenes = (EvalScene * nb)()
    base = 0
    for b in range(nb):
        lo, hi = bounds[b, :3].astype(np.float64), bounds[b, 3:].astype(np.float64)
        side = np.float32(cell_side)
        while True:
            dims = np.floor((hi - lo) / float(side)).astype(np.int64) + 1
            if int(dims.prod()) <= max_cells:
                break
            side = np.float32(side * np.float32(2.0))
        sc = scenes[b]
        sc.n_end, sc.m_end, sc.cell_base = ends[b], 0, base
        for k in range(3):
            sc.dims[k], sc.origin[k] = int(dims[k]), float(bounds[b, k])
        sc.side, sc.inv_side = float(side), float(np.float32(1.0) / side)
        base += int(dims.prod())
    grid = (torch.tensor([[s.origin[k] for k in range(3)] for s in scenes], dtype=torch.float32, device=dev),
            torch.tensor([s.inv_side for s in scenes], dtype=torch.float32, device=dev),
            torch.tensor([[s.dims[k] for k in range(3)] for s in scenes], dtype=torch.int64, device=dev),
            torch.tensor([s.cell_base for s in scenes], dtype=torch.int64, device=dev))
    key = _eval_keys(xyz, _eval_batch_index(ends, dev), grid)
    order = torch.sort(key, stable=True)[1]
    cell_start = torch.zeros(base + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = torch.cumsum(torch.bincount(key, minlength=base), 0)
    return EvalTable(scenes, ends, order.to(torch.int32), xyz[order].contiguous(), cell_start, grid)


def eval_nn(xyz, new_xyz, offset, new_offset, cell_side=0.08, table=None, sort_queries=True):
    """(idx int32 [m], dist2 float32 [m]): for every row of new_xyz the nearest row of xyz of its scene, bit-identical to
    knnquery(nsample = 1) on the same tensors (doda_eval_nn over eval_table's grid).  offset / new_offset: END offsets int32 [B].
    sort_queries: hand the queries out in cell order (a wave then walks the same cells); the result does not depend on it."""
    _need_cuda(xyz, new_xyz, offset, new_offset)
    if new_xyz.dtype != torch.float32 or new_xyz.dim() != 2 or new_xyz.shape[1] != 3 or new_offset.dtype != torch.int32:
        raise RuntimeError("eval_nn: new_xyz float32 [m, 3], new_offset int32 [B]")
    if table is None:
        table = eval_table(xyz, offset, cell_side)
    new_xyz = new_xyz.contiguous()
    m, dev = new_xyz.shape[0], new_xyz.device
    new_ends = _eval_ends(new_offset, m, "eval_nn")
    if len(new_ends) != len(table.ends):
        raise RuntimeError("eval_nn: offset and new_offset name the same scenes")
    scenes = type(table.scenes)()
    C.memmove(scenes, table.scenes, C.sizeof(scenes))
    for b, e in enumerate(new_ends):
        scenes[b].m_end = e
    qorder = None
    if sort_queries and m > 0:
        qorder = torch.argsort(_eval_keys(new_xyz, _eval_batch_index(new_ends, dev), table.grid)).to(torch.int32)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    dist2 = torch.empty(m, dtype=torch.float32, device=dev)
    check(lib().doda_eval_nn(_p(table.xyz_sorted), _p(table.order), table.order.numel(), _p(table.cell_start), scenes, len(new_ends),
                             _p(new_xyz), _p(qorder), m, _p(idx), _p(dist2), _stream()), "doda_eval_nn")
    return idx, dist2


def eval_score(feats, weight, bias, p2v, idx, labels_all, ignore_index, hist, want_pred=True):
    """Full-cloud scoring without the score matrix (doda_eval_score): for full point i the voxel v = p2v[idx[i]] (idx None: the
    identity).  hist int64 [3, n_cls] += (intersection, prediction area, target area) over the valid points.
    -> (out float64 [2] = {sum of the valid points' cross-entropy, their number}, pred_all uint8 [m] = the voxels' argmax, or None)."""
    feats, weight, bias, _, _ = _head_args("eval_score", feats, weight, bias)
    _need_cuda(p2v, labels_all, hist)
    n_cls = weight.shape[0]
    if (weight.dim() != 2 or weight.shape[1] != feats.shape[1] or p2v.dtype != torch.int32 or labels_all.dtype != torch.int64
            or hist.dtype != torch.int64 or tuple(hist.shape) != (3, n_cls) or not hist.is_contiguous()
            or (bias is not None and (bias.dtype != torch.float32 or bias.numel() != n_cls or not bias.is_cuda))):
        raise RuntimeError("eval_score: weight float32 [n_cls, c], bias float32 [n_cls], p2v int32 [n], labels int64 [m], hist int64 [3, n_cls]")
    p2v, labels_all = p2v.contiguous(), labels_all.contiguous()
    m = labels_all.shape[0]
    if idx is not None:
        _need_cuda(idx)
        if idx.dtype != torch.int32 or idx.shape[0] != m:
            raise RuntimeError("eval_score: idx int32 [m], one per label")
        idx = idx.contiguous()
    elif p2v.shape[0] != m:
        raise RuntimeError("eval_score: without idx, one p2v entry per label")
    nb = int(lib().doda_eval_score_blocks(m))
    out = torch.empty(2, dtype=torch.float64, device=feats.device)
    ws = torch.empty(2 * nb, dtype=torch.float64, device=feats.device)
    pred = torch.empty(m, dtype=torch.uint8, device=feats.device) if want_pred else None
    check(lib().doda_eval_score(_p(feats), feats.shape[0], feats.shape[1], feats.element_size(), _p(weight), _p(bias), n_cls, _p(p2v),
                                p2v.shape[0], _p(idx), _p(labels_all), m, int(ignore_index), _p(pred), _p(hist), _p(out), _p(ws), nb,
                                _stream()), "doda_eval_score")
    return out, pred


def sgd_multi(params, grads, bufs, first, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
              maximize=False):
    """torch.optim.SGD's update of all (param, grad, momentum buffer) triples in one launch (doda_sgd_multi).
    fp32 contiguous device tensors; bufs[k] may be None when momentum == 0; first[k]: buffer not initialised."""
    n = len(params)
    if n == 0:
        return
    dev = params[0].device
    arr = (_SgdTensor * n)()
    for k, (p, g, b) in enumerate(zip(params, grads, bufs)):
        for t in (p, g) + ((b,) if b is not None else ()):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or not t.is_cuda:
                raise ValueError("sgd_multi needs contiguous fp32 tensors on one HIP device")
        if g.shape != p.shape or (b is not None and b.shape != p.shape):
            raise ValueError("sgd_multi: shape mismatch")
        arr[k].p, arr[k].g, arr[k].buf = p.data_ptr(), g.data_ptr(), (b.data_ptr() if b is not None else None)
        arr[k].n, arr[k].first_step = p.numel(), int(bool(first[k]))
    nbytes = lib().doda_sgd_multi_desc_bytes(n)
    desc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().doda_sgd_multi(C.cast(arr, C.c_void_p), n, float(lr), float(momentum), float(dampening),
                               float(weight_decay), int(bool(nesterov)), int(bool(maximize)), _p(desc), nbytes,
                               _stream()), "doda_sgd_multi")


def optim_step(kind, params, grads, state1, state2, bc1, bc2s, first, lr, beta1, beta2, eps, weight_decay, nesterov=False,
               maximize=False, max_norm=0.0, norm_out=None):
    """One optimizer step over all tensors (doda_optim_step, include/doda_optim.h): kind _lib.OPTIM_SGD / OPTIM_ADAM / OPTIM_ADAMW;
    state1 / state2: the momentum buffers (entries may be None when the momentum, passed as beta1, is 0) or exp_avg / exp_avg_sq;
    bc1 / bc2s: Adam's per-tensor bias corrections; first: SGD's buffer-not-initialised flags.  max_norm > 0 clips the global
    gradient norm first, stores the scaled gradients back and writes the norm to norm_out (fp32 device scalar).  fp32 contiguous
    device tensors; one launch, two with the clip."""
    from ._lib import OPTIM_SGD, OptimHyper, OptimTensor
    n = len(params)
    if n == 0:
        return
    adam = kind != OPTIM_SGD
    dev = params[0].device
    arr = (OptimTensor * n)()
    for k in range(n):
        p, g = params[k], grads[k]
        a = state1[k] if state1 else None
        b = state2[k] if adam else None
        for t in (p, g, a, b):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or not t.is_cuda or t.shape != p.shape):
                raise ValueError("optim_step needs contiguous fp32 tensors of the parameter's shape on one HIP device")
        arr[k].p, arr[k].g = p.data_ptr(), g.data_ptr()
        arr[k].state1 = a.data_ptr() if a is not None else None
        arr[k].state2 = b.data_ptr() if b is not None else None
        arr[k].n = p.numel()
        if adam:
            arr[k].bias_correction1, arr[k].bias_correction2_sqrt = bc1[k], bc2s[k]
        else:
            arr[k].first_step = int(bool(first[k]))
    clip = max_norm is not None and max_norm > 0
    if clip and (norm_out is None or norm_out.dtype != torch.float32 or norm_out.device != dev or norm_out.numel() != 1):
        raise ValueError("optim_step: the clip needs an fp32 device scalar for the norm")
    hyper = OptimHyper(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(nesterov)), int(bool(maximize)))
    nbytes = lib().doda_optim_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().doda_optim_step(arr, n, int(kind), C.byref(hyper), float(max_norm) if clip else 0.0, _p(norm_out) if clip else None,
                                _p(ws), nbytes, _stream()), "doda_optim_step")


# ---- coarse-level op lists (ABI 11, csrc/layers.hip: doda_layers_run) --------------------------------------
# the CX_* kinds and flags are _lib's (doda_hip.h).  Widest BatchNorm op the list takes (csrc/bn_totals.hpp BN_TOT_MAX_C = PRE_MAX_C:
# the LDS channel vectors of lay_bn / bn_apply and of the folded gather prologue); a list with a wider one is refused with
# DODA_ERR_UNSUPPORTED before anything launches
CX_BN_MAX_C = 256


def _cx_array(ops, n_part):
    n = len(ops)
    arr = (_CxOp * n)()
    ptr_fields = {"x", "w", "tbl", "y", "y2", "res", "aux", "stats", "stats_b", "gamma", "beta", "mean", "invstd",
                  "running_mean", "running_var", "nbt", "dgamma", "dbeta"}
    for k, o in enumerate(ops):
        for name, v in o.items():
            if name in ptr_fields:
                if v is not None:
                    _need_cuda(v)
                setattr(arr[k], name, v.data_ptr() if v is not None else None)
            else:
                setattr(arr[k], name, v)
        arr[k].n_part = n_part
    return arr


def stats_totals(c, device):
    """Zeroed fp64 totals for the statistics of a c-channel tensor (the `stats` of an op of layers_run) = totals_zeros."""
    return totals_zeros(c, device)


def layers_run(ops, device, elem_bytes=2):
    """Run a list of ops (dicts keyed by the doda_cx_op field names; tensors for the pointer fields) through the per-layer backend (doda_layers_run, ABI 11): one whole-chip launch
    per op, BatchNorm ops folded into the next convolution's gather where their rows are few (set_pre_rows).  `stats` /
    `stats_b` are fp64 totals (stats_totals).  Returns the number of launches issued."""
    n = len(ops)
    arr = _cx_array(ops, 0)
    launches = C.c_int32(0)
    check(lib().doda_layers_run(C.cast(arr, C.c_void_p), n, int(elem_bytes), C.byref(launches), _stream()), "doda_layers_run")
    return int(launches.value)


def set_pre_rows(fwd=None, bwd=None):
    """Row thresholds of layers_run's BatchNorm folding (doda_set_option DODA_OPT_PRE_FWD_ROWS / _BWD_ROWS; 0: never fold).
    Returns the previous pair."""
    from ._lib import OPT_PRE_BWD_ROWS, OPT_PRE_FWD_ROWS
    old = (int(lib().doda_get_option(OPT_PRE_FWD_ROWS)), int(lib().doda_get_option(OPT_PRE_BWD_ROWS)))
    if fwd is not None:
        check(lib().doda_set_option(OPT_PRE_FWD_ROWS, int(fwd)), "doda_set_option")
    if bwd is not None:
        check(lib().doda_set_option(OPT_PRE_BWD_ROWS, int(bwd)), "doda_set_option")
    return old


# ---- the rest of PG_OP: clustering, segment pools, proposal IoU (include/doda_pgops.h, csrc/pgops.hip) -------------------
def _pg_graph_args(what, semantic_label, ball_query_idxs, start_len, cuda):
    for t in (semantic_label, ball_query_idxs, start_len):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.is_cuda != cuda:
            raise RuntimeError("%s: contiguous int32 %s tensors expected" % (what, "device" if cuda else "CPU"))
    n = semantic_label.numel()
    if start_len.numel() != 2 * n:
        raise RuntimeError("%s: start_len must be [N, 2] for N labels" % what)
    return n, ball_query_idxs.numel()


def pg_components(semantic_label, ball_query_idxs, start_len):
    """(root int32 [N], size int32 [N]): connected components of the ball-query graph restricted to equal semantic labels, edges
    taken as undirected (doda_pg_components).  root[i] is the smallest point index of i's component, size is the component's point
    count at roots and 0 elsewhere.  No read-back."""
    _need_cuda(semantic_label, ball_query_idxs, start_len)
    n, n_active = _pg_graph_args("pg_components", semantic_label, ball_query_idxs, start_len, True)
    root = torch.empty(n, dtype=torch.int32, device=semantic_label.device)     # (both written in full by the init launch)
    size = torch.empty(n, dtype=torch.int32, device=semantic_label.device)
    check(lib().doda_pg_components(_p(semantic_label), _p(ball_query_idxs), _p(start_len), n, n_active, _p(root), _p(size),
                                   _stream()), "doda_pg_components")
    return root, size


def pg_cluster(semantic_label, ball_query_idxs, start_len, threshold):
    """(cluster_idxs int32 [sumNPoint, 2], cluster_offsets int32 [nCluster + 1]) on the device: the components of pg_components
    with at least `threshold` points, numbered by ascending root — the reference's order, whose seeds ascend and are their
    component's smallest index —, rows (cluster id, point index).  Inside a cluster the points ascend (the reference lists them in
    BFS visiting order; no consumer depends on it).  Grouping is torch on the device: a stable sort by root, cumulative sums.  One
    read-back gives the two output sizes."""
    root, size = pg_components(semantic_label, ball_query_idxs, start_len)
    n, dev = root.numel(), root.device
    if n == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ar = torch.arange(n, dtype=torch.int32, device=dev)
    rl = root.long()
    keep = size[rl] >= int(threshold)
    kept_root = (root == ar) & keep
    sum_n, n_cluster = torch.stack((keep.sum(), kept_root.sum())).tolist()          # the one read-back
    order = torch.sort(torch.where(keep, root, n), stable=True)[1][:sum_n]           # kept points by (root, index)
    rank = torch.cumsum(kept_root, 0) - 1                                            # cluster number at a kept root
    cluster_idxs = torch.stack((rank[rl[order]], order), 1).to(torch.int32)
    roots = torch.sort(torch.where(kept_root, ar, n))[0][:n_cluster].long()          # kept roots ascending
    cluster_offsets = torch.zeros(n_cluster + 1, dtype=torch.int32, device=dev)
    cluster_offsets[1:] = torch.cumsum(size[roots], 0)
    return cluster_idxs.contiguous(), cluster_offsets


def pg_bfs_cluster_host(semantic_label, ball_query_idxs, start_len, threshold):
    """The reference's sequential BFS on CPU tensors (doda_pg_bfs_cluster_h; no GPU touched): the same pair as pg_cluster, clusters
    and the points inside each in the reference's order."""
    n, n_active = _pg_graph_args("pg_bfs_cluster_host", semantic_label, ball_query_idxs, start_len, False)
    idxs = torch.zeros((n, 2), dtype=torch.int32)
    offsets = torch.zeros(n + 1, dtype=torch.int32)
    sum_n, n_cluster = C.c_int32(0), C.c_int32(0)
    check(lib().doda_pg_bfs_cluster_h(_p(semantic_label), _p(ball_query_idxs), _p(start_len), n, n_active, int(threshold), _p(idxs),
                                      _p(offsets), C.byref(sum_n), C.byref(n_cluster)), "doda_pg_bfs_cluster_h")
    return idxs[:sum_n.value].clone(), offsets[:n_cluster.value + 1].clone()


def _pg_seg_args(what, rows, offsets, seg, n_seg, c, extra=None):
    """rows: float32 [n_rows, c]; seg: float32 [n_seg, c] (extra: int32 of the same shape); offsets int32 [n_seg + 1]."""
    ts = (rows, offsets, seg) + (() if extra is None else (extra,))
    _need_cuda(*ts)
    n_seg, c = int(n_seg), int(c)
    ok = (rows.dtype == torch.float32 and seg.dtype == torch.float32 and offsets.dtype == torch.int32
          and all(t.is_contiguous() for t in ts) and rows.dim() == 2 and rows.shape[1] == c and seg.numel() == n_seg * c
          and offsets.numel() == n_seg + 1 and (extra is None or (extra.dtype == torch.int32 and extra.numel() == n_seg * c)))
    if not ok:
        raise RuntimeError("%s: contiguous float32 [rows, C] / [nProposal, C] and int32 offsets [nProposal + 1] expected" % what)
    return rows.shape[0], n_seg, c


def _pg_pool(name, inp, offsets, out, n_seg, c):
    n_rows, n_seg, c = _pg_seg_args(name, inp, offsets, out, n_seg, c)
    check(getattr(lib(), "doda_pg_" + name)(_p(inp), _p(offsets), _p(out), n_rows, n_seg, c, _stream()), "doda_pg_" + name)


def sec_mean(inp, offsets, out, n_seg, c):
    """out[s] = sum over the rows of segment s of inp[row] / float(len) (fp32; 0 for an empty segment)."""
    _pg_pool("sec_mean", inp, offsets, out, n_seg, c)


def sec_min(inp, offsets, out, n_seg, c):
    """out[s] = column-wise minimum over segment s (+inf for an empty one), bit-exact."""
    _pg_pool("sec_min", inp, offsets, out, n_seg, c)


def sec_max(inp, offsets, out, n_seg, c):
    """out[s] = column-wise maximum over segment s (-inf for an empty one), bit-exact."""
    _pg_pool("sec_max", inp, offsets, out, n_seg, c)


def sec_mean_bp(d_inp, offsets, d_out, n_seg, c):
    """d_inp[row] = d_out[s] / float(len) for the rows of every segment; other rows are left as they are."""
    n_rows, n_seg, c = _pg_seg_args("sec_mean_bp", d_inp, offsets, d_out, n_seg, c)
    check(lib().doda_pg_sec_mean_bp(_p(d_inp), _p(offsets), _p(d_out), n_rows, n_seg, c, _stream()), "doda_pg_sec_mean_bp")


def roipool_fp(feats, offsets, out, maxidx, n_seg, c):
    """out[s] = column-wise maximum over segment s, maxidx[s] the smallest row that holds it (-inf / -1 where nothing wins)."""
    n_rows, n_seg, c = _pg_seg_args("roipool_fp", feats, offsets, out, n_seg, c, extra=maxidx)
    check(lib().doda_pg_roipool_fp(_p(feats), _p(offsets), _p(out), _p(maxidx), n_rows, n_seg, c, _stream()), "doda_pg_roipool_fp")


def roipool_bp(d_feats, offsets, maxidx, d_out, n_seg, c):
    """d_feats[maxidx[s][ch]][ch] += d_out[s][ch]; an argmax outside the rows (-1) is skipped."""
    n_rows, n_seg, c = _pg_seg_args("roipool_bp", d_feats, offsets, d_out, n_seg, c, extra=maxidx)
    check(lib().doda_pg_roipool_bp(_p(d_feats), _p(maxidx), _p(d_out), n_rows, n_seg, c, _stream()), "doda_pg_roipool_bp")


def get_iou(proposals_idx, proposals_offset, instance_labels, instance_pointnum, proposals_iou, n_instance, n_proposal):
    """proposals_iou float32 [nProposal, nInstance] = intersection / (proposal + instance - intersection + 1e-5), the reference's
    expression bit for bit, from one integer histogram per proposal (doda_pg_get_iou)."""
    ts = (proposals_idx, proposals_offset, instance_labels, instance_pointnum, proposals_iou)
    _need_cuda(*ts)
    n_instance, n_proposal = int(n_instance), int(n_proposal)
    ok = (proposals_idx.dtype == torch.int32 and proposals_offset.dtype == torch.int32 and instance_labels.dtype == torch.int64
          and instance_pointnum.dtype == torch.int32 and proposals_iou.dtype == torch.float32 and all(t.is_contiguous() for t in ts)
          and proposals_offset.numel() == n_proposal + 1 and instance_pointnum.numel() == n_instance
          and proposals_iou.numel() == n_proposal * n_instance)
    if not ok:
        raise RuntimeError("get_iou: int32 proposals_idx / proposals_offset [nProposal + 1] / instance_pointnum [nInstance], int64 "
                           "instance_labels, float32 proposals_iou [nProposal, nInstance], all contiguous")
    ws = _ws(lib().doda_pg_get_iou_workspace_bytes(n_proposal, n_instance), proposals_idx.device)
    check(lib().doda_pg_get_iou(_p(proposals_idx), _p(proposals_offset), _p(instance_labels), _p(instance_pointnum),
                                _p(proposals_iou), instance_labels.numel(), proposals_idx.numel(), n_instance, n_proposal, _p(ws),
                                ws.numel(), _stream()), "doda_pg_get_iou")


# ---- the rest of pointops2_cuda: sampling, grouping, interpolation, subtraction, aggregation (include/doda_pointops.h) --------
def _po_check(what, floats=(), ints=()):
    """float32 / int32, contiguous, on the device."""
    _need_cuda(*floats, *ints)
    for t in floats:
        if t.dtype != torch.float32:
            raise TypeError("%s: float32 tensors expected, got %s" % (what, t.dtype))
    for t in ints:
        if t.dtype != torch.int32:
            raise TypeError("%s: int32 index / offset tensors expected, got %s" % (what, t.dtype))
    for t in (*floats, *ints):
        if not t.is_contiguous():
            raise RuntimeError("%s: contiguous tensors expected" % what)


def _po_shape(what, ok):
    if not ok:
        raise RuntimeError("%s: tensor shapes do not match the sizes" % what)


po_transpose_calls = 0   # how many times the index by destination was built (tests count it)


def po_transpose(idx, n):
    """(start int32 [n + 1], pos int32 [m * nsample]) of idx int32 [m, nsample]: for every destination j in [0, n) the flat positions
    p with idx.view(-1)[p] == j, ascending, at pos[start[j] : start[j + 1]]; entries outside [0, n) are dropped."""
    global po_transpose_calls
    _po_check("po_transpose", ints=(idx,))
    _po_shape("po_transpose", idx.dim() == 2)
    n = int(n)
    m, nsample = idx.shape
    start = torch.zeros(n + 1, dtype=torch.int32, device=idx.device)
    pos = torch.empty(m * nsample, dtype=torch.int32, device=idx.device)
    nbytes = lib().doda_po_transpose_workspace_bytes(n)
    ws = _ws(nbytes, idx.device)
    check(lib().doda_po_transpose(_p(idx), m, nsample, n, _p(start), _p(pos), _p(ws), ws.numel(), _stream()), "doda_po_transpose")
    po_transpose_calls += 1
    return start, pos


def _po_transposed_ok(what, start, pos, n, total):
    _po_check(what, ints=(start, pos))
    _po_shape(what, start.numel() == n + 1 and pos.numel() >= total)


def po_grouping_fwd(inp, idx, out):
    """out [m, nsample, c] = inp [n, c] rows at idx [m, nsample]; an index outside [0, n) reads as 0."""
    _po_check("po_grouping_fwd", (inp, out), (idx,))
    _po_shape("po_grouping_fwd", inp.dim() == 2 and idx.dim() == 2 and out.numel() == idx.numel() * inp.shape[1])
    n, c = inp.shape
    check(lib().doda_po_grouping_fwd(_p(inp), _p(idx), _p(out), n, idx.shape[0], idx.shape[1], c, _stream()), "doda_po_grouping_fwd")


def po_grouping_bwd(d_out, start, pos, d_inp):
    """d_inp [n, c] = per destination the sum, in ascending position, of the rows of d_out [m * nsample, c]."""
    _po_check("po_grouping_bwd", (d_out, d_inp))
    n, c = d_inp.shape
    total = d_out.numel() // max(c, 1)
    _po_shape("po_grouping_bwd", d_inp.dim() == 2 and d_out.numel() == total * c)
    _po_transposed_ok("po_grouping_bwd", start, pos, n, total)
    check(lib().doda_po_grouping_bwd(_p(d_out), _p(start), _p(pos), _p(d_inp), n, total, c, _stream()), "doda_po_grouping_bwd")


def po_interpolation_fwd(inp, idx, w, out):
    """out [m, c] = sum_i inp[idx[r, i]] * w[r, i], i ascending (inp [n, c], idx / w [m, k])."""
    _po_check("po_interpolation_fwd", (inp, w, out), (idx,))
    _po_shape("po_interpolation_fwd", inp.dim() == 2 and idx.dim() == 2 and w.shape == idx.shape
              and out.shape == (idx.shape[0], inp.shape[1]))
    n, c = inp.shape
    check(lib().doda_po_interpolation_fwd(_p(inp), _p(idx), _p(w), _p(out), n, idx.shape[0], idx.shape[1], c, _stream()),
          "doda_po_interpolation_fwd")


def po_interpolation_bwd(d_out, w, start, pos, d_inp):
    """d_inp [n, c] = per destination the sum, in ascending position p, of d_out[p // k] * w.view(-1)[p]."""
    _po_check("po_interpolation_bwd", (d_out, w, d_inp))
    _po_shape("po_interpolation_bwd", d_out.dim() == 2 and w.dim() == 2 and d_inp.dim() == 2 and w.shape[0] == d_out.shape[0]
              and d_inp.shape[1] == d_out.shape[1])
    (m, k), (n, c) = w.shape, d_inp.shape
    _po_transposed_ok("po_interpolation_bwd", start, pos, n, m * k)
    check(lib().doda_po_interpolation_bwd(_p(d_out), _p(w), _p(start), _p(pos), _p(d_inp), n, m, k, c, _stream()),
          "doda_po_interpolation_bwd")


def po_subtraction_fwd(a, b, idx, out):
    """out [m, nsample, c] = a[r] - b[idx[r, i]] (a [m, c], b [n, c])."""
    _po_check("po_subtraction_fwd", (a, b, out), (idx,))
    _po_shape("po_subtraction_fwd", a.dim() == 2 and b.dim() == 2 and idx.dim() == 2 and a.shape[1] == b.shape[1]
              and idx.shape[0] == a.shape[0] and out.numel() == idx.numel() * a.shape[1])
    check(lib().doda_po_subtraction_fwd(_p(a), _p(b), _p(idx), _p(out), b.shape[0], a.shape[0], idx.shape[1], a.shape[1], _stream()),
          "doda_po_subtraction_fwd")


def po_subtraction_bwd(d_out, start, pos, d_a, d_b):
    """d_a [m, c] = sum_i d_out[r, i], i ascending; d_b [n, c] = per destination the sum of -d_out[p] in ascending position."""
    _po_check("po_subtraction_bwd", (d_out, d_a, d_b))
    _po_shape("po_subtraction_bwd", d_out.dim() == 3 and d_a.shape == (d_out.shape[0], d_out.shape[2]) and d_b.dim() == 2
              and d_b.shape[1] == d_out.shape[2])
    m, nsample, c = d_out.shape
    _po_transposed_ok("po_subtraction_bwd", start, pos, d_b.shape[0], m * nsample)
    check(lib().doda_po_subtraction_bwd(_p(d_out), _p(start), _p(pos), _p(d_a), _p(d_b), d_b.shape[0], m, nsample, c, _stream()),
          "doda_po_subtraction_bwd")


def _po_aggregation_sizes(what, inp, position, w, idx):
    _po_shape(what, inp.dim() == 2 and position.dim() == 3 and w.dim() == 3 and idx.shape == position.shape[:2]
              and w.shape[:2] == position.shape[:2] and position.shape[2] == inp.shape[1] and w.shape[2] >= 1)
    m, nsample, c = position.shape
    return inp.shape[0], m, nsample, c, w.shape[2]


def po_aggregation_fwd(inp, position, w, idx, out):
    """out [m, c] = sum_i (inp[idx[r, i]] + position[r, i]) * w[r, i, ch % w_c], i ascending."""
    _po_check("po_aggregation_fwd", (inp, position, w, out), (idx,))
    n, m, nsample, c, w_c = _po_aggregation_sizes("po_aggregation_fwd", inp, position, w, idx)
    _po_shape("po_aggregation_fwd", out.shape == (m, c))
    check(lib().doda_po_aggregation_fwd(_p(inp), _p(position), _p(w), _p(idx), _p(out), n, m, nsample, c, w_c, _stream()),
          "doda_po_aggregation_fwd")


def po_aggregation_bwd(inp, position, w, idx, start, pos, d_out, d_inp, d_position, d_w):
    """The three gradients of po_aggregation_fwd (include/doda_pointops.h states each sum's order)."""
    _po_check("po_aggregation_bwd", (inp, position, w, d_out, d_inp, d_position, d_w), (idx,))
    n, m, nsample, c, w_c = _po_aggregation_sizes("po_aggregation_bwd", inp, position, w, idx)
    _po_shape("po_aggregation_bwd", d_out.shape == (m, c) and d_inp.shape == inp.shape and d_position.shape == position.shape
              and d_w.shape == w.shape)
    _po_transposed_ok("po_aggregation_bwd", start, pos, n, m * nsample)
    check(lib().doda_po_aggregation_bwd(_p(inp), _p(position), _p(w), _p(idx), _p(start), _p(pos), _p(d_out), _p(d_inp),
                                        _p(d_position), _p(d_w), n, m, nsample, c, w_c, _stream()), "doda_po_aggregation_bwd")


def po_furthestsampling(xyz, offset, new_offset, tmp, idx):
    """idx int32 [m]: furthest point sampling of xyz [n, dim] per batch segment; offset / new_offset int32 [B] are END offsets.  tmp:
    float32 [n] workspace, initialised by the kernel.  Ties go to the lowest point index (include/doda_pointops.h)."""
    _po_check("po_furthestsampling", (xyz, tmp), (offset, new_offset, idx))
    _po_shape("po_furthestsampling", xyz.dim() == 2 and tmp.numel() >= xyz.shape[0] and offset.numel() == new_offset.numel())
    check(lib().doda_po_furthestsampling(_p(xyz), _p(offset), _p(new_offset), _p(tmp), _p(idx), xyz.shape[0], idx.numel(),
                                         offset.numel(), xyz.shape[1], _stream()), "doda_po_furthestsampling")


# ------------------------------------------------------------------------------------------
# the rest of the spconv surface (include/doda_spconv.h): transposed rulebook, max pooling by element size, dense volumes
# ------------------------------------------------------------------------------------------
def rulebook_deconv(indices, spatial_shape, batch_size, ksize, stride, padding, dilation, output_padding):
    """Rulebook of a transposed sparse convolution (K <= 27).  Returns (out_indices int32 [M_out,4], tbl int32 [K,M_out],
    tbl_rev int32 [K,M], out_shape list[3]) in the layout of rulebook_conv.  One D2H sync (M_out)."""
    indices = _check_indices(indices)
    m = indices.shape[0]
    dev = indices.device
    shape_c, _ = _shape3(spatial_shape)
    k, s, p, d, op = _i3(ksize), _i3(stride), _i3(padding), _i3(dilation), _i3(output_padding)
    K = k[0] * k[1] * k[2]
    out_shape_c = (C.c_int32 * 3)()
    count = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib().doda_rulebook_deconv_workspace_bytes(m, K)
    if nbytes == 0:
        raise DodaNativeError("doda_rulebook_deconv: kernel volume %d or size not supported" % K)
    ws = _ws(nbytes, dev)
    check(lib().doda_rulebook_deconv_assign(_p(indices), m, shape_c, int(batch_size), k, s, p, d, op, out_shape_c,
                                            _p(count), _p(ws), ws.numel(), _stream()), "doda_rulebook_deconv_assign")
    m_out = int(count.item())
    out_idx = torch.empty((m_out, 4), dtype=torch.int32, device=dev)
    tbl = torch.empty((K, m_out), dtype=torch.int32, device=dev)
    tbl_rev = torch.empty((K, m), dtype=torch.int32, device=dev)
    check(lib().doda_rulebook_deconv_tables(_p(indices), m, shape_c, int(batch_size), k, s, p, d, op, m_out,
                                            _p(out_idx), _p(tbl), m_out, _p(tbl_rev), m, _p(ws), ws.numel(),
                                            _stream()), "doda_rulebook_deconv_tables")
    return out_idx, tbl, tbl_rev, [int(v) for v in out_shape_c]


def _pool_tbl(tbl, rows, what):
    _need_cuda(tbl)
    if tbl.dtype != torch.int32 or tbl.dim() != 2 or not tbl.is_contiguous() or tbl.shape[1] < rows:
        raise RuntimeError("%s: the table must be a contiguous int32 [K, >= %d] tensor" % (what, rows))


def maxpool_fwd_rows(x, tbl, n_out):
    """Indice max pooling of fp32 or bf16 rows over the outputs' table [K, n_out] (doda_maxpool_fwd): y [n_out, c] in x's dtype."""
    _feat_ok(x, "x")
    _pool_tbl(tbl, n_out, "maxpool_fwd_rows")
    y = torch.empty((n_out, x.shape[1]), dtype=x.dtype, device=x.device)
    check(lib().doda_maxpool_fwd(_p(x), x.shape[1], _esz(x), _p(tbl), tbl.shape[1], tbl.shape[0], x.shape[0], n_out, _p(y),
                                 _stream()), "doda_maxpool_fwd")
    return y


def maxpool_bwd_rows(x, y, dy, tbl_rev, dx=None):
    """Gradient of maxpool_fwd_rows over the inputs' table [K, n_in] (doda_maxpool_bwd): every row of dx is written once, so a dx
    handed in needs no fill."""
    for t, name in ((x, "x"), (y, "y"), (dy, "dy")):
        _feat_ok(t, name)
    _pool_tbl(tbl_rev, x.shape[0], "maxpool_bwd_rows")
    if dx is None:
        dx = torch.empty_like(x)
    if not (y.dtype == dy.dtype == dx.dtype == x.dtype and y.shape == dy.shape and y.shape[1] == x.shape[1]
            and dx.shape == x.shape and dx.is_contiguous() and dx.is_cuda):
        raise RuntimeError("maxpool_bwd_rows: x / dx [n_in, c] and y / dy [n_out, c] of one dtype")
    check(lib().doda_maxpool_bwd(_p(x), _p(y), _p(dy), x.shape[1], _esz(x), _p(tbl_rev), tbl_rev.shape[1], tbl_rev.shape[0],
                                 x.shape[0], y.shape[0], _p(dx), _stream()), "doda_maxpool_bwd")
    return dx


def _dense_args(what, rows, indices, batch_size, spatial_shape):
    _feat_ok(rows, what + ": rows")
    indices = _check_indices(indices)
    if indices.shape[0] != rows.shape[0]:
        raise RuntimeError("%s: one index row per feature row" % what)
    shape_c, s = _shape3(spatial_shape)
    return indices, shape_c, s


def dense_scatter(rows, indices, batch_size, spatial_shape, channels_first):
    """The dense volume of unique rows (doda_dense_scatter): [B, C, X, Y, Z] or [B, X, Y, Z, C], zero where no row lies."""
    indices, shape_c, s = _dense_args("dense_scatter", rows, indices, batch_size, spatial_shape)
    c = rows.shape[1]
    out = torch.empty([int(batch_size), c] + s if channels_first else [int(batch_size)] + s + [c], dtype=rows.dtype, device=rows.device)
    check(lib().doda_dense_scatter(_p(rows), _p(indices), rows.shape[0], c, _esz(rows), int(batch_size), shape_c,
                                   int(bool(channels_first)), _p(out), _stream()), "doda_dense_scatter")
    return out


def dense_gather(volume, indices, channels_first):
    """Rows [M, C] of a contiguous dense volume at `indices` (doda_dense_gather)."""
    _need_cuda(volume)
    indices = _check_indices(indices)
    if volume.dim() != 5 or not volume.is_contiguous():
        raise RuntimeError("dense_gather: a contiguous 5-D volume")
    b = volume.shape[0]
    c, s = (volume.shape[1], list(volume.shape[2:])) if channels_first else (volume.shape[4], list(volume.shape[1:4]))
    shape_c, _ = _shape3(s)
    rows = torch.empty((indices.shape[0], c), dtype=volume.dtype, device=volume.device)
    check(lib().doda_dense_gather(_p(volume), _p(indices), indices.shape[0], c, _esz(volume), b, shape_c,
                                  int(bool(channels_first)), _p(rows), _stream()), "doda_dense_gather")
    return rows


def from_dense(volume):
    """(indices int32 [M, 4], rows [M, C]) of the active cells of a contiguous channels-last volume [B, X, Y, Z, C], in row-major
    cell order (doda_from_dense_count / _emit).  One D2H sync (M)."""
    _need_cuda(volume)
    if volume.dim() != 5 or not volume.is_contiguous():
        raise RuntimeError("from_dense: a contiguous [B, X, Y, Z, C] volume")
    b, c = volume.shape[0], volume.shape[4]
    shape_c, s = _shape3(list(volume.shape[1:4]))
    dev = volume.device
    nbytes = lib().doda_from_dense_workspace_bytes(b * s[0] * s[1] * s[2])
    if nbytes == 0:
        raise DodaNativeError("doda_from_dense: a volume of %d cells is not supported" % (b * s[0] * s[1] * s[2]))
    ws = _ws(nbytes, dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().doda_from_dense_count(_p(volume), c, _esz(volume), b, shape_c, _p(count), _p(ws), ws.numel(), _stream()),
          "doda_from_dense_count")
    m = int(count.item())
    indices = torch.empty((m, 4), dtype=torch.int32, device=dev)
    rows = torch.empty((m, c), dtype=volume.dtype, device=dev)
    check(lib().doda_from_dense_emit(_p(volume), c, _esz(volume), b, shape_c, m, _p(indices), _p(rows), _p(ws), ws.numel(),
                                     _stream()), "doda_from_dense_emit")
    return indices, rows

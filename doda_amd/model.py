"""SparseConv U-Net of DODA, as a caller of doda_amd.spconv.

The reference's own model files (model/unet.py:15-69, model/unet_block.py:9-100) run unchanged on
top of doda_amd.spconv; they cannot travel to the GPU box, so bench.py and
smoke() drive this counterpart.  It has the same layer graph (7 levels, channels
16*i, block_reps residual blocks per stage, BN(eps=1e-4, momentum=0.1) -> ReLU -> conv
pre-activation order, k2s2 down / inverse up sharing `spconv{i}`, concatenation skip, BN weight 1 /
bias 0 init) and the same module names, so state dicts are interchangeable with the reference's
checkpoints (`input_conv.0.weight`, `unet.blocks.block0.conv_branch.2.weight`, `unet.conv.2.weight`,
`unet.u...`, `unet.deconv.2.weight`, `unet.blocks_tail.block0.i_branch.0.weight`, `linear.weight`).
tests/test_oracle_unet.py and tests/test_gpu_unet.py check that equivalence through
tests/golden/unet_golden.npz / unet_state_keys.json, which the reference's own model files produced.
"""
import functools
import os as _os
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import torch
from torch import nn
from torch.autograd import Function
from torch.nn.modules.module import register_module_module_registration_hook

from . import nn as _dnn
from . import ops as _ops
from . import pointgroup_ops, spconv
from .lovasz import _VoxelHeadLovasz, lovasz_softmax
from .spconv import conv as _cv
from .spconv import functional as Fsp
from .spconv.modules import SparseModule, _run, any_hooks
from .streams import independent_stream


def default_cfg(n_classes=20, in_channel=3, mid_channel=16, block_reps=2, block_residual=True,
                use_xyz=False, voxel_mode=4):
    """The keys SparseConvNet reads, with cfgs/scannet/spconv.yaml's values (:16-21)."""
    backbone = SimpleNamespace(in_channel=in_channel, mid_channel=mid_channel, block_reps=block_reps,
                               block_residual=block_residual, use_xyz=use_xyz)
    return SimpleNamespace(MODEL=SimpleNamespace(BACKBONE=backbone),
                           COMMON_CLASSES=SimpleNamespace(n_classes=n_classes),
                           DATA_CONFIG=SimpleNamespace(
                               DATA_PROCESSOR=SimpleNamespace(voxel_mode=voxel_mode),
                               DATA_CLASS=SimpleNamespace(n_classes=n_classes, ignore_label=255)))


def unwrap(model):
    """The network itself behind a DistributedDataParallel-style wrapper."""
    return model.module if hasattr(model, "module") else model


# One extension call per residual block instead of one per BatchNorm / convolution (DODA_FAST_BLOCKS=0: module by module)
FAST_BLOCKS = _os.environ.get("DODA_FAST_BLOCKS", "1") == "1"
# Skip connections through the BatchNorm's pass-through output (round 3): a tensor that feeds a fused BatchNorm AND a skip
# (the U-Net level's concatenation, reference model/unet_block.py:89-93; the 1x1 skip of a channel-changing block) hands
# the skip the BatchNorm op's alias of it, so the skip's gradient — for the concatenation a column slice of the wider
# gradient, taken with its row stride, no copy — is summed inside the BatchNorm's backward kernel: 12 accumulation
# kernels per step less.  DODA_SKIP_FUSION=0: off.
SKIP_IN_BLOCK = SKIP_VIA_BN = _os.environ.get("DODA_SKIP_FUSION", "1") == "1"
# The concatenation's BatchNorm takes the statistics rows of its two halves (conv epilogues) instead of sweeping the new tensor
CAT_STATS = _os.environ.get("DODA_CAT_STATS", "1") == "1"


# ---- one description per block, cached until the module tree changes ----
# The generation counts submodule registrations anywhere in the process: setattr / add_module of a submodule (so also
# SyncBatchNorm.convert_sync_batchnorm and DSNorm.convert_dsnorm); train(), eval() and .float() register nothing.  A direct write
# into `_modules[...]` bypasses the hook.  What no registration reports — a replaced Parameter, its dtype, requires_grad, training —
# is looked at per call, where the operands are gathered.
_STRUCTURE = [0]


def _structure_changed(module, name, submodule):
    _STRUCTURE[0] += 1


register_module_module_registration_hook(_structure_changed)


def _described(module, describe):
    """describe(module), kept on the module (its one cache entry) until the next registration of a submodule."""
    entry = module.__dict__.get("_doda_desc")
    if entry is None or entry[0] != _STRUCTURE[0]:
        entry = module.__dict__["_doda_desc"] = (_STRUCTURE[0], describe(module))
    return entry[1]


def _plain_bn(m):
    return type(m) is nn.BatchNorm1d and m.affine and m.track_running_stats and m.momentum is not None


def _plain_conv(m, cls, ksize):
    return type(m) is cls and m.bias is None and m.kernel_size == ksize


def _op_list_bn(m):   # (the kernels' widest BatchNorm; width 32 carries 320 / 384 / 448 channels at levels 5-7)
    return m._parameters["weight"].dtype == torch.float32 and m.num_features <= _ops.CX_BN_MAX_C


def _op_list_conv(m):
    return (m._parameters["weight"].dtype == torch.float32 and m.in_channels % 16 == 0 and m.out_channels % 16 == 0
            and m.in_channels >= 16)


class _Block:
    """The plain residual block of the reference (model/unet_block.py:9-37): [BN, ReLU, SubM3, BN, ReLU, SubM3] + skip.
    skip: the bias-free 1x1 SubM convolution that can run inside an extension call, or None (`identity`, or any other i_branch,
    which then runs as a module); modules: what the hook sweep of a route looks at; per_block / op_list: does the block meet what
    ext.residual_block (channels in fours) / the op list (channels in sixteens, fp32 weights, BatchNorm width) asks of it."""
    __slots__ = ("bn1", "bn2", "conv1", "conv2", "skip", "identity", "modules", "per_block", "op_list")


def _describe_block(block):
    mods = tuple(block.conv_branch._modules.values())
    if not (len(mods) == 6 and _plain_bn(mods[0]) and type(mods[1]) is nn.ReLU and _plain_conv(mods[2], spconv.SubMConv3d, [3, 3, 3])
            and _plain_bn(mods[3]) and type(mods[4]) is nn.ReLU and _plain_conv(mods[5], spconv.SubMConv3d, [3, 3, 3])
            and mods[2].indice_key is not None and mods[2].indice_key == mods[5].indice_key):
        return None
    d = _Block()
    d.bn1, d.conv1, d.bn2, d.conv2 = mods[0], mods[2], mods[3], mods[5]
    sk = tuple(block.i_branch._modules.values())
    d.identity = len(sk) == 1 and type(sk[0]) is nn.Identity
    d.skip = sk[0] if (len(sk) == 1 and _plain_conv(sk[0], spconv.SubMConv3d, [1, 1, 1]) and sk[0].in_channels % 4 == 0
                       and sk[0].out_channels % 4 == 0) else None
    d.modules = (block.conv_branch, block.i_branch) + mods + sk
    convs = (d.conv1, d.conv2) if d.skip is None else (d.conv1, d.conv2, d.skip)
    d.per_block = all(c.in_channels % 4 == 0 and c.out_channels % 4 == 0 for c in convs)
    d.op_list = ((d.identity or d.skip is not None) and all(_op_list_conv(c) for c in convs)
                 and _op_list_bn(d.bn1) and _op_list_bn(d.bn2))
    return d


class _Triple:
    """[norm, ReLU, sparse convolution]: a level's `conv` (down) and `deconv` (up) sequences (model/unet_block.py:62-85).
    op_list: "down" / "up" when the op list takes it as that step (plain BatchNorm, bias-free k2 convolution, strided for down,
    inverse for up, channels in sixteens, fp32), else None."""
    __slots__ = ("bn", "conv", "modules", "op_list")


def _describe_triple(seq):
    mods = tuple(seq._modules.values())
    if not (len(mods) == 3 and type(mods[1]) is nn.ReLU and isinstance(mods[2], spconv.SparseConvolution)):
        return None
    d = _Triple()
    d.bn, d.conv, d.modules = mods[0], mods[2], (seq,) + mods
    kind = ("down" if type(d.conv) is spconv.SparseConv3d and d.conv.stride == [2, 2, 2] else
            "up" if type(d.conv) is spconv.SparseInverseConv3d else None)
    d.op_list = kind if (kind and _plain_bn(d.bn) and _op_list_bn(d.bn) and d.conv.bias is None and d.conv.kernel_size == [2, 2, 2]
                         and _op_list_conv(d.conv)) else None
    return d


def _bn_operands(bn):
    """bn x5 of both extension calls: gamma, beta, running_mean, running_var, num_batches_tracked — the objects of THIS call."""
    par, buf = bn._parameters, bn._buffers
    return [par["weight"], par["bias"], buf["running_mean"], buf["running_var"], buf["num_batches_tracked"]]


def _block_operands(d, feats, idict, rows, training, skip_in_call, pairs):
    """What either route hands the extension for one block — (rulebook, bn1 x5, conv1 x3, bn2 x5, conv2 x3, skip conv x5 | None) —
    or None where a precondition fails.  conv x3 = weight, packed forward, packed data-grad.  skip conv x5 (when skip_in_call) =
    conv x3, the identity table of `rows` rows, and that table again as both pair lists of the skip's weight gradient where
    `pairs` and the level is large enough for lists, else None."""
    bn1, bn2, c1, c2 = d.bn1, d.bn2, d.conv1, d.conv2
    data = idict.get(c1.indice_key)
    if (data is None or data.kind != "subm" or data.tbl.shape[1] != rows or bn1.training != training or bn2.training != training
            or c1.training != training or c2.training != training):
        return None
    b1, b2 = _bn_operands(bn1), _bn_operands(bn2)
    pk1, pk2 = c1._packed(feats, idict), c2._packed(feats, idict)
    if pk1 is None or pk2 is None or b1[0].dtype != torch.float32 or b2[0].dtype != torch.float32:
        return None
    sc = None
    if skip_in_call:
        w = d.skip._parameters["weight"]
        pks = d.skip._packed(feats, idict)
        if pks is None:
            return None
        ident = _cv._identity_table(rows, feats.device)
        sc = [w, pks[0], pks[1], ident, ident if (pairs and Fsp._want_pairs(feats, w, rows)) else None]
    return (data, b1, [c1._parameters["weight"], pk1[0], pk1[1]], b2, [c2._parameters["weight"], pk2[0], pk2[1]], sc)


def _triple_operands(d, feats, idict, rows, training):
    """(strided rulebook, bn x5, conv x3) of a down or up step at the level with `rows` rows, or None where a precondition fails."""
    data = idict.get(d.conv.indice_key)
    if data is None or data.kind != "down2" or d.bn.training != training or data.tbl_rev.shape[1] != rows:
        return None
    pk = d.conv._packed(feats, idict)
    bn = _bn_operands(d.bn)
    if pk is None or bn[0].dtype != torch.float32:
        return None
    return data, bn, [d.conv._parameters["weight"], pk[0], pk[1]]


def _residual_block_args(d, feats, stats, operands, rb, skip, want_stats):
    """ext.residual_block's positional arguments (csrc_ext/doda_torch.cpp, the comment above residual_block and its signature:
    x, stats_in, bn1, bn2, training, momentum1, eps1, momentum2, eps2, cv1, cv2, rb, n_out, skip, want_stats, sc, stats_in_b)."""
    data, bn1, cv1, bn2, cv2, sc = operands
    stats_b = None
    if isinstance(stats, tuple):   # the input is a channel concatenation: statistics rows of its two halves
        stats, stats_b = stats
    return (feats, stats, bn1, bn2, d.bn1.training, d.bn1.momentum, d.bn1.eps, d.bn2.momentum, d.bn2.eps, cv1, cv2, rb,
            data.outids.shape[0], skip, want_stats, sc or [], stats_b)


def _block_step(d, operands):
    """(tensors, scalars) of an op-list RB step (csrc_ext/doda_torch.cpp, `step RB (kind 0)` above namespace coarse): t[0] subm
    table, t[1:6] bn1, t[6:9] conv1, t[9:14] bn2, t[14:17] conv2, t[17:20] skip conv or None x3, t[20] identity table or None,
    t[21] that table as the skip's pair lists or None; scalars eps1, momentum1, eps2, momentum2."""
    data, bn1, cv1, bn2, cv2, sc = operands
    return ([data.tbl] + bn1 + cv1 + bn2 + cv2 + (sc or [None, None, None, None, None]),
            [d.bn1.eps, d.bn1.momentum, d.bn2.eps, d.bn2.momentum])


def _updown_step(d, operands, down, rows_out):
    """(tensors, scalars) of an op-list DOWN / UP step (csrc_ext/doda_torch.cpp, `step DOWN (kind 1)` / `step UP (kind 2)`):
    child and par_off tables (UP: swapped), bn x5, conv x3; scalars eps, momentum, rows of the step's output."""
    data, bn, cv = operands
    return (([data.tbl, data.tbl_rev] if down else [data.tbl_rev, data.tbl]) + bn + cv, [d.bn.eps, d.bn.momentum, rows_out])


def _subm3(cin, cout, key):
    return spconv.SubMConv3d(cin, cout, kernel_size=3, padding=1, bias=False, indice_key=key)


class ResidualBlock(SparseModule):
    """y = conv_branch(x) + i_branch(x); i_branch is Identity or a 1x1 SubM when Cin != Cout."""

    def __init__(self, in_channels, out_channels, norm_fn, indice_key=None):
        super().__init__()
        skip = nn.Identity() if in_channels == out_channels else \
            spconv.SubMConv3d(in_channels, out_channels, kernel_size=1, bias=False)
        self.i_branch = spconv.SparseSequential(skip)
        self.conv_branch = spconv.SparseSequential(
            norm_fn(in_channels), nn.ReLU(), _subm3(in_channels, out_channels, indice_key),
            norm_fn(out_channels), nn.ReLU(), _subm3(out_channels, out_channels, indice_key))

    def _description(self):
        """The block's _Block, or None when it is not the plain block of the reference."""
        return _described(self, _describe_block)

    def forward(self, input):
        # reference: output = conv_branch(input); output.features += i_branch(identity).features
        # (model/unet_block.py:33-37).  Here the add rides in the last convolution's store and, for an
        # identity skip, the skip's gradient in the first BatchNorm's backward kernel.
        if FAST_BLOCKS:
            out = self._forward_one_call(input)
            if out is not None:
                return out
        if type(self.i_branch[0]) is nn.Identity and len(self.i_branch) == 1:
            return self.conv_branch(input, residual="input")
        skip = self.i_branch(input.header(input.features))
        return self.conv_branch(input, residual=skip.features)

    def _forward_one_call(self, input):
        """The whole block as ONE extension call (csrc_ext residual_block: the same native ops and autograd nodes the
        module-by-module path issues, without the interpreter between them), or None when any precondition of that
        path does not hold — then the modules run one by one as before."""
        ext, d, feats = Fsp._ext, self._description(), input.features
        # (hooks — feature taps, profilers — must fire: module by module then)
        if (ext is None or not Fsp._SERIAL or d is None or not d.per_block or any_hooks(d.modules) or not feats.is_cuda or feats.dim() != 2 or feats.shape[0] < 2 or feats.dtype not in (torch.float32, torch.bfloat16)):
            return None
        training = d.bn1.training
        # the 1x1 skip convolution (reference model/unet_block.py:18-21) runs inside the extension call, on the first
        # BatchNorm's pass-through alias of the input: its data gradient is then summed inside that BatchNorm's
        # backward kernel instead of by an autograd accumulation kernel (SKIP_IN_BLOCK; the input has two consumers)
        in_call = SKIP_IN_BLOCK and training and d.skip is not None and d.skip.training
        operands = _block_operands(d, feats, input.indice_dict, feats.shape[0], training, in_call, True)
        if operands is None:
            return None
        data, skip = operands[0], None
        if not (d.identity or in_call):
            skip = self.i_branch(input.header(feats)).features
            if skip.dtype != feats.dtype:
                return None
        p1, p2 = Fsp._lists(data, feats, operands[2][0]), Fsp._lists(data, feats, operands[4][0])
        if (p1 is None) != (p2 is None):
            return None
        rb = [data.tbl, None, None, None, None] if p1 is None else [data.tbl, p1[0], p1[1], p1[2], p1[3] if len(p1) > 3 else None]
        want_stats = training and Fsp.BN_FUSION and data.outids.shape[0] > Fsp.STATS_MIN_ROWS
        y, stats = ext.residual_block(*_residual_block_args(d, feats, input.stats(), operands, rb, skip, want_stats))
        out = input.header(y, data.outids, data.out_spatial_shape)
        if stats is not None:
            out.set_stats(stats)
        return out


class VGGBlock(SparseModule):
    def __init__(self, in_channels, out_channels, norm_fn, indice_key=None):
        super().__init__()
        self.conv_layers = spconv.SparseSequential(
            norm_fn(in_channels), nn.ReLU(), _subm3(in_channels, out_channels, indice_key))

    def forward(self, input):
        return self.conv_layers(input)


# Coarse levels as ONE extension call per direction (csrc_ext coarse_ublock: a UBlock subtree compiled into an op list, one autograd
# node, gradients of every layer incl. the deferred weight-gradient jobs), issued by the library as whole-chip per-layer launches
# (doda_layers_run, csrc/layers.hip) with every BatchNorm whose rows are few folded into the gather of the convolution behind it
# and the level concatenations written in place by their two producers: ~60 launches, ~100 autograd nodes and the interpreter
# between them less per step; bf16 and fp32.  Bench step 5.05 -> 4.81 ms, host floor 5.0 -> 4.1 ms (tools/layers_ab.py).
# DODA_COARSE_MODE: "layers" (default) | "off" (module by module).  Round 5's persistent single-XCD executor ("exec") is gone:
# with the per-layer launches issued from inside the library it lost at every batch size (4.30 against 4.05-4.28 ms at the host
# floor, 7.35 against 4.81 at the bench size).
# ABI 12: the op list takes ANY level (a GEMM op carries its table's tilebook, the LDS-staged kernels write column slices), so the
# default subtree is the whole U-Net: one extension call forward, one autograd node backward, no interpreter between the 99 + 134
# launches of a step's convolutions and BatchNorms, the three remaining torch.cat and their gradient slices gone (4.61 -> 4.53 ms,
# host floor 4.1 -> 2.1 ms per step).
COARSE_MODE = _os.environ.get("DODA_COARSE_MODE", "layers")
COARSE_EXEC_LEVEL = int(_os.environ.get("DODA_COARSE_LEVEL", "1"))
COARSE_LAYERS_MAX_ROWS = int(_os.environ.get("DODA_COARSE_LAYERS_MAX_ROWS", str(1 << 23)))


def set_coarse_mode(mode, level=None):
    """mode: "layers" | "off"; level: the U-Net level whose UBlock subtree becomes one extension call."""
    global COARSE_MODE, COARSE_EXEC_LEVEL
    assert mode in ("layers", "off"), mode
    COARSE_MODE = mode
    if level is not None:
        COARSE_EXEC_LEVEL = int(level)
    return mode


def choose_coarse_backend(rows, dtype):
    """"layers" when a subtree whose input has `rows` rows runs as one extension call, None for module by module."""
    if COARSE_MODE == "off" or dtype not in (torch.bfloat16, torch.float32):
        return None
    return "layers" if 2 <= rows <= COARSE_LAYERS_MAX_ROWS else None


def _coarse_entry_level():
    """The level whose UBlock becomes one call: COARSE_EXEC_LEVEL, or below the tensor hook at EARLY_LEVEL's input when the exchange is armed."""
    return COARSE_EXEC_LEVEL if _early_exchange[0] is None else max(COARSE_EXEC_LEVEL, EARLY_LEVEL + 1)


# Early gradient exchange (doda_amd.dist.GradAllReduce.arm): a callback fired from a tensor hook when the backward pass has
# produced the gradient of level EARLY_LEVEL's input — every deeper layer and the whole decoder are done by then.
EARLY_LEVEL = 3
_early_exchange = [None]


def set_early_exchange(fn):
    _early_exchange[0] = fn


# Level at which the forward pass turns launch-floor bound (a few thousand rows and fewer): PyramidPrefetcher starts the
# NEXT batch's rulebook kernels there instead of next to the level-1 convolutions (see PyramidPrefetcher.submit).
COARSE_LEVEL = 4
_coarse_hooks = []
_STEP_KINDS = {"rb": 0, "down": 1, "up": 2}


def _walk(ub):
    steps = [("rb", blk, ub.level) for blk in ub.blocks._modules.values()]
    if len(ub.nPlanes) > 1:
        steps += [("down", ub.conv, ub.level)] + _walk(ub.u) + [("up", ub.deconv, ub.level)]
        steps += [("rb", blk, ub.level) for blk in ub.blocks_tail._modules.values()]
    return steps


def _describe_subtree(ub):
    """The UBlock subtree as op-list steps — ([("rb", block, level) | ("down", seq, level) | ("up", seq, level)] in execution order,
    their descriptions, every module and every parameter of the subtree for the per-call sweeps) — or False when a module of it is
    not the plain reference form (model/unet_block.py:9-37,55-100) or does not meet what the op list asks (_Block, _Triple)."""
    steps, descs = _walk(ub), []
    for kind, m, _ in steps:
        if kind == "rb":
            d = m._description() if type(m) is ResidualBlock else None
            good = d is not None and d.op_list
        else:
            d = _described(m, _describe_triple)
            good = d is not None and d.op_list == kind
        if not good:
            return False
        descs.append(d)
    return steps, descs, list(ub.modules()), list(ub.parameters())


class UBlock(nn.Module):
    """One U-Net level: blocks -> [down -> UBlock(level+1) -> up -> cat -> blocks_tail]."""

    def __init__(self, nPlanes, norm_fn, block_reps, block, indice_key_id=1):
        super().__init__()
        self.nPlanes = nPlanes
        self.level = indice_key_id
        c = nPlanes[0]
        subm_key, down_key = "subm%d" % indice_key_id, "spconv%d" % indice_key_id
        self.blocks = spconv.SparseSequential(OrderedDict(
            ("block%d" % r, block(c, c, norm_fn, indice_key=subm_key)) for r in range(block_reps)))
        if len(nPlanes) > 1:
            c_next = nPlanes[1]
            self.conv = spconv.SparseSequential(
                norm_fn(c), nn.ReLU(),
                spconv.SparseConv3d(c, c_next, kernel_size=2, stride=2, bias=False, indice_key=down_key))
            self.u = UBlock(nPlanes[1:], norm_fn, block_reps, block, indice_key_id=indice_key_id + 1)
            self.deconv = spconv.SparseSequential(
                norm_fn(c_next), nn.ReLU(),
                spconv.SparseInverseConv3d(c_next, c, kernel_size=2, bias=False, indice_key=down_key))
            self.blocks_tail = spconv.SparseSequential(OrderedDict(
                ("block%d" % r, block(c * (2 - r) if r < 2 else c, c, norm_fn, indice_key=subm_key))
                for r in range(block_reps)))

    # ---- the subtree as executor steps (csrc_ext coarse_ublock) ----
    def _coarse_modules(self):
        """The steps of _describe_subtree, or False."""
        plan = _described(self, _describe_subtree)
        return plan and plan[0]

    def _forward_coarse(self, input):
        """The whole subtree in one executor call, or None when a precondition fails (then the modules run one by one)."""
        ext = Fsp._ext
        feats = input.features
        if (ext is None or not Fsp._SERIAL or not feats.is_cuda or feats.dim() != 2
                or choose_coarse_backend(feats.shape[0], feats.dtype) is None):
            return None
        plan = _described(self, _describe_subtree)
        if plan is False:
            return None
        steps, descs, modules, params = plan
        training = self.training
        grad = torch.is_grad_enabled() and feats.requires_grad
        # per call (the plan is cached): a hook on ANY module of the subtree (feature taps, profilers) must fire, and a frozen
        # parameter must not receive a gradient — both mean module by module
        if any_hooks(modules):
            return None
        if grad:
            for q in params:
                if not q.requires_grad:
                    return None
            if not (training and ext.get_defer_wgrad() and ext.get_direct_grads()):
                return None
        idict = input.indice_dict
        kinds, tensors, scalars = [], [], []
        gate_step = -1          # first step of level COARSE_LEVEL: where the rulebook prefetcher's gate opens (see forward)
        rows = {self.level: feats.shape[0]}
        for (kind, _, lvl), d in zip(steps, descs):
            if kind == "rb":
                operands = _block_operands(d, feats, idict, rows.get(lvl), training, not d.identity, grad)
                if operands is None:
                    return None
                if lvl == COARSE_LEVEL and gate_step < 0:
                    gate_step = len(kinds)
                step = _block_step(d, operands)
            else:
                operands = _triple_operands(d, feats, idict, rows.get(lvl), training)
                if operands is None:
                    return None
                if kind == "down":
                    rows[lvl + 1] = operands[0].outids.shape[0]
                    if rows[lvl + 1] < 2:
                        return None
                step = _updown_step(d, operands, kind == "down", rows[lvl + 1] if kind == "down" else rows[lvl])
            kinds.append(_STEP_KINDS[kind])
            tensors.append(step[0])
            scalars.append(step[1])
        stats_in = input.stats()
        if not torch.is_tensor(stats_in):   # (the op list's first BatchNorm takes one statistics tensor, not a concatenation's pair)
            stats_in = None
        gate = None
        if self.level < COARSE_LEVEL and gate_step >= 0 and _coarse_hooks and training and torch.is_grad_enabled():
            hooks = list(_coarse_hooks)

            def gate():
                for hook in hooks:
                    hook()
        y, stats = ext.coarse_ublock(feats, stats_in, kinds, tensors, scalars, training, gate_step if gate is not None else -1, gate)
        out = input.header(y)
        if stats is not None:
            out.set_stats(stats)
        return out

    def forward(self, input):
        if self.level == COARSE_LEVEL and _coarse_hooks and self.training and torch.is_grad_enabled():   # (training steps only)
            for hook in list(_coarse_hooks):   # the step enters its coarse levels: few rows, most CUs idle from here on
                hook()
        if (self.level == EARLY_LEVEL and _early_exchange[0] is not None and self.training and torch.is_grad_enabled()
                and input.features.requires_grad):
            def _fire(g, fn=_early_exchange[0]):
                fn()
                return g
            input.features.register_hook(_fire)
        if COARSE_MODE != "off" and self.level == _coarse_entry_level():
            out = self._forward_coarse(input)
            if out is not None:
                return out
        out = self.blocks(input)
        if len(self.nPlanes) > 1:
            skip_feats, st_a = out.features, out.stats()
            down = self._down_with_skip(out) if SKIP_VIA_BN else None
            if down is not None:
                skip_feats, down = down
            else:
                down = self.conv(out)                 # (re-binds out.features)
            dec = self.deconv(self.u(down))
            st_b = dec.stats()
            out.features = torch.cat((skip_feats, dec.features), dim=1)
            # BatchNorm statistics are per channel: the concatenation's are its halves' — the rows the two producing convs
            # accumulated in their epilogues — so the first BatchNorm of blocks_tail needs no sweep over the new tensor
            out.clear_stats()
            if CAT_STATS and torch.is_tensor(st_a) and torch.is_tensor(st_b):   # (a half that is itself a concatenation: no pair of pairs)
                out.set_stats((st_a, st_b))
            out = self.blocks_tail(out)
        return out

    def _down_with_skip(self, out):
        """self.conv = [BatchNorm, ReLU, strided conv] with the BatchNorm's pass-through output: returns (alias of
        out.features for the skip connection, the strided conv's output), or None when the sequence is not that plain
        triple in training mode on the fused path.  The concatenation's gradient for the skip — a column slice of a
        twice as wide matrix — then reaches the BatchNorm's backward kernel as its strided `add` operand."""
        d = _described(self.conv, _describe_triple)
        feats = out.features
        if (d is None or not d.bn.training or not torch.is_grad_enabled() or not feats.requires_grad or out.indices.shape[0] < 2
                or _dnn._ext is None or not _dnn.fusable(d.bn, feats) or any_hooks(d.modules)):
            return None
        y, alias = _dnn.batch_norm_relu(feats, d.bn, True, True, out.stats())
        return alias, _run(d.conv, out.header(y))


class _PointLinear(Function):
    """scores[n] = feats[p2v[n]] @ W^T + b: the voxel->point gather and the Linear head of reference
    model/unet.py:62-64 as ONE gather-GEMM (K = 1 table = p2v).  Backward re-uses the same native
    kernels: d_feats[v] = sum over the voxel's points (table = transposed v2p map) of d_scores @ W,
    dW = wgrad over the p2v table."""

    @staticmethod
    def forward(ctx, feats, weight, bias, p2v, v2p_t):
        n = p2v.shape[0]
        fused_bias = (bias is not None and bias.dtype == torch.float32 and bias.is_cuda and feats.shape[1] % 4 == 0
                      and weight.shape[0] % 4 == 0)
        # (the bias rides in the gather kernel's store as a broadcast residual row: no separate pass over the scores)
        scores = None
        if fused_bias:
            try:
                scores = _ops.spconv_gather(feats.contiguous(), weight.view(1, *weight.shape), p2v.view(1, n), n, 1,
                                            weight.shape[0], out_f32=True, residual=bias.detach().contiguous(),
                                            residual_bcast=True)
            except _ops.DodaNativeError:   # (a shape the dense-table fast kernel does not take)
                fused_bias = False
        if scores is None:
            scores = _ops.spconv_gather(feats.contiguous(), weight.view(1, *weight.shape), p2v.view(1, n),
                                        n, 1, weight.shape[0], out_f32=True)
        if bias is not None and not fused_bias:
            scores += bias
        ctx.save_for_backward(feats, weight, p2v, v2p_t)
        ctx.has_bias = bias is not None
        return scores

    @staticmethod
    def backward(ctx, d_scores):
        feats, weight, p2v, v2p_t = ctx.saved_tensors
        n = p2v.shape[0]
        d_feats = d_w = d_b = None
        if (d_scores.is_cuda and d_scores.dtype == torch.float32 and feats.dtype == torch.bfloat16 and d_scores.dim() == 2
                and d_scores.shape[1] <= 64 and d_scores.shape[0] > 0):
            # bf16 operand of the two gather-GEMMs below and the column sums (d_bias) in ONE pass over the fp32 gradient
            dy, colsum = _ops.cast_colsum(d_scores.contiguous())
            if ctx.has_bias and ctx.needs_input_grad[2]:
                d_b = colsum
        else:
            dy = d_scores.contiguous().to(feats.dtype)
        if ctx.needs_input_grad[0]:
            k = v2p_t.shape[0]
            w_rep = weight.unsqueeze(0).expand(k, *weight.shape).contiguous()
            d_feats = _ops.spconv_gather(dy, w_rep, v2p_t, feats.shape[0], 0, weight.shape[1])
        if ctx.needs_input_grad[1]:
            d_w = _ops.spconv_wgrad(feats.contiguous(), dy, p2v.view(1, n), n)[0].t().to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2] and d_b is None:
            d_b = d_scores.sum(0)
        return d_feats, d_w, d_b, None, None


class _FusedCE(Function):
    @staticmethod
    def forward(ctx, scores, labels, ignore_index):
        scores = scores.contiguous()
        out, lse = _ops.cross_entropy_fwd(scores, labels, ignore_index)
        ctx.save_for_backward(scores, labels, lse, out)
        ctx.ignore_index = ignore_index
        return out[0]

    @staticmethod
    def backward(ctx, grad):
        scores, labels, lse, out = ctx.saved_tensors
        g = grad.reshape(1).to(torch.float32).contiguous()
        return _ops.cross_entropy_bwd(scores, labels, lse, out, g, ctx.ignore_index), None, None


class _VoxelHeadCE(Function):
    """loss = CrossEntropyLoss(ignore_index)(Linear(feats[p2v]), labels) (reference model/unet.py:62-64,107-108,196) computed at
    VOXEL level: every point of a voxel reads the same feature row, so the [points, classes] score matrix — written and re-read
    five times by the matrix path, ~210 us of the bench step — never exists (csrc/head.hip).  Second output: the per-voxel
    argmax class (the meters' prediction: pred_point = pred_voxel[p2v])."""

    @staticmethod
    def forward(ctx, feats, weight, bias, v2p, labels, ignore_index):
        out, pred = _ops.head_ce_fwd(feats, weight, bias, v2p, labels, ignore_index)
        ctx.save_for_backward(feats, weight, bias, v2p, labels, out)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(pred)
        return out[0], pred

    @staticmethod
    def backward(ctx, grad, _grad_pred):
        feats, weight, bias, v2p, labels, out = ctx.saved_tensors
        d_feats, dz, d_b = _ops.head_ce_bwd(feats, weight, bias, v2p, labels, ctx.ignore_index, out, grad.reshape(1).to(torch.float32))
        return _ops.head_grads(ctx.needs_input_grad, feats, weight, bias, d_feats, dz, None, d_b)


FUSED_HEAD_LOSS = _os.environ.get("DODA_FUSED_HEAD_LOSS", "1") == "1"


def cross_entropy(scores, labels, ignore_index=255):
    """nn.CrossEntropyLoss(ignore_index) (reference model/unet.py:108,196).  Device fp32 logits with at
    most 64 classes go through the fused native pair (doda_cross_entropy_fwd/_bwd: 3 launches instead
    of ~15 torch kernels that each stream the [N, C] matrix); anything else through log_softmax + gather
    (torch's own nll_loss reduction kernels take ~1.6 ms per step at 800k points x 20 classes)."""
    if (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.shape[1] <= 64
            and labels.dtype == torch.int64 and scores.shape[0] > 0):
        return _FusedCE.apply(scores, labels.contiguous(), int(ignore_index))
    valid = labels != ignore_index
    logp = torch.log_softmax(scores.float(), dim=1)
    picked = logp.gather(1, labels.clamp(0, scores.shape[1] - 1).unsqueeze(1)).squeeze(1)
    return -(picked * valid).sum() / valid.sum().clamp(min=1)


LOSS_KINDS = ("cross_entropy", "lovasz")


def loss_kind_of(cfg):
    """OPTIMIZATION.loss of an experiment config (reference model/unet.py:107-113): cross_entropy (also when the key or the whole
    section is absent, as in default_cfg) or lovasz; anything else is NotImplementedError, as in the reference."""
    opt = getattr(cfg, "OPTIMIZATION", None)
    kind = "cross_entropy" if opt is None else (opt.get("loss", "cross_entropy") if hasattr(opt, "get")
                                                else getattr(opt, "loss", "cross_entropy"))
    if kind not in LOSS_KINDS:
        raise NotImplementedError("OPTIMIZATION.loss: %r (cross_entropy | lovasz)" % (kind,))
    return kind


def criterion_of(model):
    """The point-level criterion(scores, labels, ignore_index) of a (possibly wrapped) network; cross_entropy for one without a choice."""
    return getattr(unwrap(model), "criterion", cross_entropy)


def matrix_loss(net, scores, labels, ignore_index):
    """The tail of the matrix path: the network's criterion on the point-level scores, which stay behind for point_predictions."""
    net.voxel_pred = None                 # (point_predictions: this batch's scores, not an earlier call's voxel argmax)
    net.point_scores = scores.detach()    # (no reference to the score matrix's graph)
    return criterion_of(net)(scores, labels, ignore_index)


class SparseConvNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        # the configured loss: the point-level criterion of the matrix path and the voxel-level autograd function of head_loss
        self.loss_kind = loss_kind_of(cfg)
        if self.loss_kind == "lovasz":
            self.criterion, self.voxel_head = lovasz_softmax, _VoxelHeadLovasz
        else:
            self.criterion, self.voxel_head = cross_entropy, _VoxelHeadCE
        bb = cfg.MODEL.BACKBONE
        try:
            n_classes = cfg.COMMON_CLASSES.n_classes
        except AttributeError:
            n_classes = cfg.DATA_CONFIG.DATA_CLASS.n_classes
        m = bb.mid_channel
        norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
        block = ResidualBlock if bb.block_residual else VGGBlock
        self.input_conv = spconv.SparseSequential(_subm3(bb.in_channel, m, "subm1"))
        self.unet = UBlock([m * i for i in range(1, 8)], norm_fn, bb.block_reps, block, indice_key_id=1)
        self.output_layer = spconv.SparseSequential(norm_fn(m), nn.ReLU())
        self.linear = nn.Linear(m, n_classes)
        for mod in self.modules():  # reference set_bn_init (unet.py:51-56)
            if "BatchNorm" in mod.__class__.__name__:
                mod.weight.data.fill_(1.0)
                mod.bias.data.fill_(0.0)

    def head_loss(self, feats, v2p_map, labels, ignore_index=255):
        """Linear head + the configured loss on the voxel features without the point-level score matrix (_VoxelHeadCE, or
        lovasz._VoxelHeadLovasz under OPTIMIZATION.loss: lovasz), or None when that form does not apply (then: scores =
        forward(...), self.criterion(scores, labels)).  Sets self.voxel_pred."""
        if not (FUSED_HEAD_LOSS and feats.is_cuda and feats.dim() == 2 and feats.shape[1] == 16 and feats.shape[0] > 0
                and feats.dtype in (torch.float32, torch.bfloat16) and self.linear.out_features <= 32
                and self.linear.weight.dtype == torch.float32 and v2p_map is not None and v2p_map.is_cuda
                and v2p_map.dtype == torch.int32 and v2p_map.dim() == 2 and v2p_map.shape[0] == feats.shape[0]
                and labels.is_cuda and labels.dtype == torch.int64 and not any_hooks((self.linear,))):
            return None
        if self.loss_kind == "lovasz" and not (self.linear.out_features >= 2 and v2p_map.shape[1] - 1 <= _ops.LOVASZ_MAX_POINTS_PER_VOXEL
                                                and 2 * feats.shape[0] * self.linear.out_features < 2 ** 31):
            return None
        loss, pred = self.voxel_head.apply(feats, self.linear.weight, self.linear.bias, v2p_map, labels, int(ignore_index))
        self.voxel_pred = pred
        return loss

    def _trunk(self, input):
        if input.features.is_cuda and input.indices.shape[0] > 0:
            # all 13 rulebooks up front (+ their pair lists when a bf16 backward pass will follow)
            spconv.ops.build_pyramid(input, len(self.unet.nPlanes), with_pairs=_with_pairs(self, input.features.dtype),
                                     with_tiles=tile_levels_for(input.features.dtype))   # tilebooks serve inference as well
        return self.output_layer(self.unet(self.input_conv(input)))

    @torch.no_grad()
    def voxel_confidence(self, input):
        """Pseudo-label inputs of the self-training stage (reference model/unet.py:115-132: softmax(Linear(feats[p2v])).max(1)) at
        VOXEL level, without the point-score matrix: trunk, output layer, then doda_st_voxel_confidence.  -> (pred int32 [m],
        conf float32 [m]); every point of voxel v has pred[v] / conf[v].  No fallback: a head outside the kernel's range (16 / 32
        channels, 2-32 classes, device tensors) raises."""
        feats = self._trunk(input).features
        return _ops.voxel_confidence(feats.contiguous(), self.linear.weight.detach(),
                                     self.linear.bias.detach() if self.linear.bias is not None else None)

    def forward(self, input, input_map, return_mid_feat=False, v2p_map=None, v2p_map_t=None, labels=None, ignore_index=255):
        out = self._trunk(input)
        feats = out.features
        if labels is not None and not return_mid_feat:      # the caller wants the loss: head + loss at voxel level
            loss = self.head_loss(feats, v2p_map, labels, ignore_index)
            if loss is not None:
                return loss
        fused = (v2p_map is not None and not return_mid_feat and feats.is_cuda
                 and input_map.dtype == torch.int32 and 0 < v2p_map.shape[1] - 1 <= 27
                 and feats.shape[1] % 4 == 0 and self.linear.out_features % 4 == 0)
        if fused:  # voxel->point gather + Linear as one gather-GEMM over the p2v table
            v2p_t = v2p_map_t if (v2p_map_t is not None and v2p_map_t.shape == (v2p_map.shape[1] - 1, v2p_map.shape[0])
                                  and v2p_map_t.is_contiguous()) else v2p_map[:, 1:].t().contiguous()
            scores = _PointLinear.apply(feats, self.linear.weight, self.linear.bias, input_map, v2p_t)
        else:
            point_feats = feats[input_map.long()]  # voxel -> point
            scores = self.linear(point_feats.to(self.linear.weight.dtype))
        if labels is not None and not return_mid_feat:
            return matrix_loss(self, scores, labels, ignore_index)
        return (point_feats, scores) if return_mid_feat else scores


F32_TILES = _os.environ.get("DODA_F32_TILES", "0") == "1"


# bf16 levels with a tilebook (DODA_TILE_LEVELS).  Levels 1-2 use it for the gathers AND the weight gradient; a level-3 tilebook
# (48 channels: no tile gather kernel) would serve the weight gradient only.
BF16_TILE_LEVELS = int(_os.environ.get("DODA_TILE_LEVELS", "2"))


def tile_levels_for(dtype):
    """Levels whose SubM rulebook gets a tilebook: the two finest for bf16 (rows of 32 / 64 bytes).  The tile kernel also
    takes fp32 16-channel rows (DODA_F32_TILES=1: level 1), but fp32 layers are bound by the fp32 matrix rate, 1/16 of
    bf16: measured in round 4 the fp32 step takes 12.2 ms with the tilebook against 11.9 ms on the dense-table kernels
    (conv_tile MODE 2 96 us against conv_fast 97 us per level-1 layer, and the tilebook build on top): off by default."""
    if dtype == torch.bfloat16:
        return BF16_TILE_LEVELS
    return 1 if (dtype == torch.float32 and F32_TILES) else 0


def _with_pairs(net, dtype):
    """Do this pass's rulebooks get their pair lists: only when a bf16 backward pass will follow."""
    return Fsp.WGRAD_PAIRS and torch.is_grad_enabled() and net.training and dtype == torch.bfloat16


def _build_pyramid_on(stream, coords, shape, batch_size, n_levels, with_pairs, with_tiles, after=()):
    """int32 indices and all rulebooks of one batch on `stream`, behind the events `after`.  -> (indices, indice_dict, event that
    the build has finished); _hand_over gives them to the consuming stream."""
    with torch.cuda.stream(stream):
        for event in after:
            stream.wait_event(event)
        idx32 = coords.int()
        probe = spconv.SparseConvTensor(None, idx32, shape, batch_size)
        spconv.ops.build_pyramid(probe, n_levels, with_pairs=with_pairs, with_tiles=with_tiles)
        done = torch.cuda.Event()
        done.record(stream)
    return idx32, probe.indice_dict, done


def _hand_over(idx32, book, done, device):
    """A pyramid built on a side stream, handed to the current stream: -> (indices int32, indice_dict)."""
    main = torch.cuda.current_stream(device)
    main.wait_event(done)
    idx32.record_stream(main)
    for data in book.values():
        for t in vars(data).values():
            for u in (t if isinstance(t, tuple) else (t,)):
                if torch.is_tensor(u) and u.is_cuda:
                    u.record_stream(main)
    return idx32, book


_PYR_STREAMS = {}


def _prebuild_pyramid(voxel_coords, spatial_shape, batch_size, n_levels, device, with_pairs=False, with_tiles=None):
    """Build the int32 indices and all rulebooks on a side stream that does NOT wait for the main
    stream.  Rulebooks depend only on the voxel coordinates; built at the head of the forward pass on
    the main stream, each of their six size read-backs blocks the host until the previous step's
    whole backward has drained, and the GPU then idles while the host catches up (measured: 1.1 ms of
    wall time per step for 0.55 ms of kernels).  Only valid when `voxel_coords` has no producer work
    pending on any stream (a resident batch) — the caller opts in.
    Returns (indices int32, indice_dict); every tensor is handed over to the main stream."""
    side = _PYR_STREAMS.get(device)
    if side is None:
        side = _PYR_STREAMS[device] = independent_stream(device, tag="rulebooks")
    return _hand_over(*_build_pyramid_on(side, voxel_coords, spatial_shape, batch_size, n_levels, with_pairs, with_tiles), device)


class PyramidPrefetcher:
    """Rulebooks as part of the data pipeline: the 13 rulebooks of batch k+1 are built on a helper thread
    and a side stream while the main thread issues step k.

    Rulebooks depend only on voxel coordinates — in the reference they are built inside spconv's forward,
    while its voxelisation already runs ahead of the step in DataLoader workers (dataset/dataset.py:121-187).
    Built in line, the six size read-backs of a pyramid (one per strided level) block the issuing thread
    for ~1.2 ms per step (tools/hostprof.py), and the step is paced by host issue time as much as by the
    GPU.  Here they block the helper thread instead (the extension call releases the GIL); the consumer
    picks the finished pyramid up with one stream-wait.  Every batch still gets its own rulebooks: nothing
    is cached across batches."""

    def __init__(self, device, n_levels, gated=False):
        """gated: the side stream does not start a build before the main stream's forward pass has reached the coarse
        levels (COARSE_LEVEL).  Measured: the same step with a re-used pyramid runs at 5.7 ms, with the next pyramid
        built from the start of the step at 6.5 ms — 0.9 ms of rulebook kernels next to the level-1 convolutions cost
        0.8 ms; next to the coarse levels' launch-floor-bound kernels they are nearly free."""
        self.device, self.n_levels = device, n_levels
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="doda-rulebooks")
        self.stream = independent_stream(device, tag="rulebooks")   # (not on the main stream's hardware queue)
        self.gated = bool(gated)
        self._gate = None            # (threading.Event, torch.cuda.Event) of the build waiting for this step's coarse phase
        self._lock = threading.Lock()
        self.gate_timeouts = 0       # builds that started WITHOUT the coarse-phase event (steps longer than the wait)
        if self.gated:
            _coarse_hooks.append(self._open_gate)

    def _open_gate(self):
        """Called from UBlock.forward at COARSE_LEVEL (main thread, main stream)."""
        with self._lock:
            gate, self._gate = self._gate, None
        if gate is not None:
            gate[1].record(torch.cuda.current_stream(self.device))
            gate[0].set()

    def submit(self, batch, with_pairs=False, with_tiles=None, resident=False, now=False):
        """now: build at once (the first batch: no step in flight whose coarse phase could open the gate).
        batch: collated dictionary whose `voxel_locs` is on the device.  Work still queued on the CALLER's
        current stream that produces it (collate_device returns with doda_voxelize_idx_fill pending) is ordered
        before the build through an event recorded here; resident=True (a batch that was complete before the
        call, e.g. bench.py's reused one) skips that event, so the build does not queue behind the step in flight."""
        coords, shape = batch["voxel_locs"], batch["spatial_shape"]
        bs = batch["offsets"].numel() - 1
        ready = None
        if coords.is_cuda and not resident:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
        gate = None
        if self.gated and not now:
            gate = (threading.Event(), torch.cuda.Event())
            with self._lock:
                stale, self._gate = self._gate, gate
            if stale is not None:      # a build whose step never reached the coarse levels: let it go
                stale[0].set()
        return self.pool.submit(self._build, coords, shape, bs, with_pairs, with_tiles, ready, gate)

    def _build(self, coords, shape, bs, with_pairs, with_tiles=None, ready=None, gate=None):
        torch.cuda.set_device(self.device)
        after = []
        if gate is not None:
            # wait (host side) until the main thread has recorded the coarse-phase event of the step in flight; a step
            # that never gets there (evaluation of a shallow model, an exception) must not hold the pipeline: time out
            if gate[0].wait(timeout=0.05):
                after.append(gate[1])
            else:
                # the step in flight did not reach its coarse levels in time (first iterations, evaluation, a profiler
                # run): this build goes ungated; the stale gate is withdrawn so that nobody records an event for it, and
                # the count tells an A/B reader how many of its steps were NOT gated
                with self._lock:
                    if self._gate is gate:
                        self._gate = None
                    self.gate_timeouts += 1
        if ready is not None:
            after.append(ready)
            coords.record_stream(self.stream)   # read there; the allocator must not recycle it under the build
        return _build_pyramid_on(self.stream, coords, shape, bs, self.n_levels, with_pairs, with_tiles, after)

    @staticmethod
    def take(future, device):
        """(indices int32, indice_dict) of a submitted batch, handed over to the current stream."""
        return _hand_over(*future.result(), device)

    def shutdown(self):
        with self._lock:
            gate, self._gate = self._gate, None
        if gate is not None:
            gate[0].set()
        self.pool.shutdown(wait=True)
        if self.gated and self._open_gate in _coarse_hooks:
            _coarse_hooks.remove(self._open_gate)


INPUT_ROWS = _os.environ.get("DODA_INPUT_ROWS", "1") == "1"


def _input_rows(net, feats, xyz, v2p, mode, feature_dtype):
    """The input layer's rows in one launch (ops.voxelize_fp_rows: cat + voxel pooling + cast + the layer's channel padding,
    reference model/unet.py:89-94), or None when that form does not apply (CPU, features with a gradient, another input layer)."""
    if not (INPUT_ROWS and feats.is_cuda and v2p.is_cuda and not feats.requires_grad and (xyz is None or not xyz.requires_grad)
            and feats.dtype == torch.float32 and (xyz is None or xyz.dtype == torch.float32) and v2p.dtype == torch.int32
            and v2p.dim() == 2 and v2p.shape[0] > 0 and feature_dtype in (torch.float32, torch.bfloat16) and mode in (3, 4)):
        return None
    conv = getattr(net, "input_conv", None)
    conv = conv[0] if conv is not None and len(conv) == 1 else None
    if not isinstance(conv, spconv.SubMConv3d):
        return None
    c_in = feats.shape[1] + (0 if xyz is None else xyz.shape[1])
    c_out = _cv.padded_in_channels(conv, feature_dtype)
    if conv.in_channels != c_in:
        return None
    rows = _ops.voxelize_fp_rows(feats.contiguous(), None if xyz is None else xyz.contiguous(), v2p.contiguous(), mode,
                                  c_out or c_in, feature_dtype)
    if c_out:
        rows._doda_padded_from = c_in
    return rows


def point_predictions(model, p2v):
    """argmax class per POINT after a `labels=` call of voxelize_and_run: the per-voxel argmax of the fused head gathered through
    p2v, or the argmax of the score matrix when the matrix path ran."""
    net = unwrap(model)
    vp = getattr(net, "voxel_pred", None)
    if vp is not None:
        return vp[p2v.long()].long()
    return net.point_scores.detach().argmax(1)


def voxelize_and_run(cfg, model, batch, device, feature_dtype=torch.float32, fused_head=True,
                     inputs_ready=False, pyramid=None, labels=None, ignore_index=255):
    """reference model/unet.py:72-99 (test_model_feat): H2D, voxel mean-pooling, network.
    labels: return the training LOSS instead of the per-point scores (reference model/unet.py:107-108,196: CrossEntropyLoss on the
    head's scores) — computed at voxel level without the score matrix when the head allows it; point_predictions() afterwards
    gives the argmax per point for the meters.
    inputs_ready: the batch is resident on `device` with no copy or kernel still producing it, so the
    rulebooks may be built on a side stream ahead of the main stream's queue (_prebuild_pyramid).
    pyramid: (indices int32, indice_dict) of this batch from PyramidPrefetcher.take."""
    inp, p2v, v2p = sparse_input(cfg, model, batch, device, feature_dtype, inputs_ready, pyramid)
    kwargs = {}
    if fused_head:
        v2p_t = batch.get("v2p_map_t")
        kwargs = dict(v2p_map=v2p, v2p_map_t=v2p_t.to(device, non_blocking=True) if v2p_t is not None else None)
        if labels is not None:   # -> the LOSS (head + CrossEntropyLoss at voxel level when the fused form applies)
            kwargs.update(labels=labels, ignore_index=ignore_index)
    out = model(inp, p2v, **kwargs)
    if labels is not None and not fused_head:
        return matrix_loss(unwrap(model), out, labels, ignore_index)
    return out


def sparse_input(cfg, model, batch, device, feature_dtype=torch.float32, inputs_ready=False, pyramid=None):
    """(network input SparseConvTensor, p2v, v2p) of a collated batch: H2D, voxel mean-pooling and the rulebooks (the first half
    of voxelize_and_run; reference model/unet.py:72-99)."""
    voxel_coords = batch["voxel_locs"].to(device, non_blocking=True)
    p2v = batch["p2v_map"].to(device, non_blocking=True)
    v2p = batch["v2p_map"].to(device, non_blocking=True)
    feats = batch["feats"].to(device, non_blocking=True)
    xyz = batch["locs_float"].to(device, non_blocking=True) if cfg.MODEL.BACKBONE.use_xyz else None
    batch_size = batch["offsets"].numel() - 1
    net = unwrap(model)
    voxel_feats = _input_rows(net, feats, xyz, v2p, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_mode, feature_dtype)
    if voxel_feats is None:
        if xyz is not None:
            feats = torch.cat((feats, xyz), 1)
        voxel_feats = pointgroup_ops.voxelization(feats, v2p, cfg.DATA_CONFIG.DATA_PROCESSOR.voxel_mode)
    if pyramid is None and (inputs_ready and batch["voxel_locs"].is_cuda and voxel_coords.shape[0] > 0
                            and hasattr(net, "unet") and device.type == "cuda"):
        pyramid = _prebuild_pyramid(voxel_coords, batch["spatial_shape"], batch_size, len(net.unet.nPlanes), device,
                                    with_pairs=_with_pairs(net, feature_dtype), with_tiles=tile_levels_for(feature_dtype))
    idx32, book = pyramid if pyramid is not None else (voxel_coords.int(), None)
    inp = spconv.SparseConvTensor(voxel_feats.to(feature_dtype), idx32, batch["spatial_shape"], batch_size)
    if book is not None:
        inp.indice_dict.update(book)
    return inp, p2v, v2p

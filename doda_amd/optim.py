"""torch's SGD, Adam and AdamW with the whole parameter update in one native launch, and the gradient-norm clip folded in.

`FusedSGD` IS `torch.optim.SGD` (same constructor, param groups, `state[p]["momentum_buffer"]`,
`state_dict()` / `load_state_dict()` — the reference's checkpoints store `optimizer.state_dict()`,
util/model_utils.py:87-94, tool/train.py:255-262) with `step()` re-routed: all (parameter, gradient,
momentum buffer) triples of a group go to `doda_sgd_multi` together instead of through torch's
multi-tensor kernels (five launches for the U-Net's 281 tensors).  The arithmetic follows torch's fused
functor term by term; parameters and buffers come out bit-identical (tests/test_gpu_round2.py).

`FusedAdam` / `FusedAdamW` are `torch.optim.Adam` / `torch.optim.AdamW` in the same way (`doda_optim_step`,
include/doda_optim.h): constructor, param groups and the state keys `step`, `exp_avg`, `exp_avg_sq` are torch's, `step` kept as
torch's default (non-fused) layout keeps it — an fp32 scalar on the CPU — so a state dict moves between these classes and plain
torch.optim.Adam / AdamW in both directions.  The bias corrections are computed on the host from `step`; the arithmetic is that of
torch's fused kernel (ATen/native/hip/fused_adam_utils.cuh) term by term (tests/test_gpu_optim.py).

All three take the keyword `max_grad_norm` (None: no clip).  When it is set, `step()` first clips the global gradient norm to it as
`torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)` would — the sum of squares in one launch more, fp64 and bitwise
reproducible, `coef = min(1, max_norm / (norm + 1e-6))` applied inside the update launch — and AFTER `step()` `p.grad` holds the
clipped gradient, as after `clip_grad_norm_`.  `clips_in_step` is then true (the trainer skips its own clip) and `last_grad_norm` is
the norm before the clip as an fp32 device scalar, never read back here.

`FusedAdam` / `FusedAdamW` fall back to the parent's `step()` (after torch's `clip_grad_norm_` when `max_grad_norm` is set) for what
the kernel does not cover: `amsgrad`, `capturable`, `differentiable`, `fused=True` or `foreach=True` asked for explicitly, a tensor
`lr` or beta, parameters that are not fp32 on a HIP device (the parent's own checks hold there), and a missing native library.  With
more than one param group the clip itself is torch's `clip_grad_norm_` over all groups (the norm spans them), then the unclipped
launch per group.

Parameters and gradients must be contiguous fp32 tensors on one HIP device (the native call checks every
tensor on every step and raises otherwise); sparse gradients are refused: use torch's optimizers for those."""
import math
import os

import torch

from . import _lib
from . import ops as _ops
from ._ext import ext as _ext


def _optim_step(*args):
    """doda_optim_step through the extension, or through ctypes when the extension is not loaded."""
    if _ext is not None:
        _ext.optim_step(*args)
    else:
        _ops.optim_step(*args)


class _Fused:
    """What the three optimizers share: the cached tensor lists, zero_grad in one call, and max_grad_norm."""

    def _init_clip(self, max_grad_norm):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive (None: no clip)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None

    @property
    def clips_in_step(self):
        return self.max_grad_norm is not None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._doda_lists = {}

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._doda_lists = {}

    def zero_grad(self, set_to_none=True):
        """torch's zero_grad(set_to_none=True) walks the parameters in Python (0.2 ms per step for the U-Net's 203); one
        extension call does the same stores.  set_to_none=False (in-place zeroing) is torch's."""
        if not set_to_none or _ext is None:
            return super().zero_grad(set_to_none=set_to_none)
        for group in self.param_groups:
            _ext.clear_grads(group["params"])

    def _torch_clip(self):
        """clip_grad_norm_ over every group: where the native clip does not apply (several groups, a fallback step)."""
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if params:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm).to(torch.float32)

    def _clip_args(self, device):
        """(max_norm, norm_out) of one native step: the clip runs inside it when there is one param group."""
        if self.max_grad_norm is None or len(self.param_groups) != 1:
            return 0.0, None
        norm = self.last_grad_norm
        if norm is None or norm.device != device or norm.dim() != 0:
            norm = self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=device)
        return self.max_grad_norm, norm


class FusedSGD(_Fused, torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *,
                 maximize=False, max_grad_norm=None):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, maximize=maximize)
        self._init_clip(max_grad_norm)

    def _slow_lists(self, group):
        """(params, grads, buffers, first flags) of the parameters that have a gradient; creates the missing
        momentum buffers (torch: clone of the first gradient — here the kernel writes it, first flag set)."""
        momentum = group["momentum"]
        ps, gs, bs, fs = [], [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("FusedSGD does not take sparse gradients; use torch.optim.SGD")
            first, buf = False, None
            if momentum != 0:
                state = self.state[p]
                buf = state.get("momentum_buffer")
                if buf is None:
                    buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    first = True
            ps.append(p); gs.append(p.grad); bs.append(buf); fs.append(int(first))
        return ps, gs, bs, fs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lists = self.__dict__.setdefault("_doda_lists", {})
        if self.clips_in_step and len(self.param_groups) != 1:
            self._torch_clip()
        for gi, group in enumerate(self.param_groups):
            lr = group["lr"]
            if torch.is_tensor(lr):
                lr = float(lr)
            momentum = group["momentum"]
            params = group["params"]
            # steady state: every parameter has a gradient and a buffer — the lists of the previous step stand
            # (the per-tensor dtype / layout / device checks are made by the native call on every step)
            cached = lists.get(gi)
            grads = [p.grad for p in params]
            if cached is not None and cached[0] is params and len(cached[1]) == len(params) and all(g is not None for g in grads):
                ps, bs, fs = params, cached[1], cached[2]
                gs = grads
            else:
                ps, gs, bs, fs = self._slow_lists(group)
                if len(ps) == len(params) and not any(fs):
                    lists[gi] = (params, bs, fs)
            if not ps:
                continue
            max_norm, norm = self._clip_args(ps[0].device)
            if max_norm > 0:    # the same arithmetic behind doda_optim_step, gradients scaled and stored back
                _optim_step(_lib.OPTIM_SGD, ps, gs, bs if momentum != 0 else [], [], [], [], fs, float(lr), float(momentum),
                            float(group["dampening"]), 0.0, float(group["weight_decay"]), bool(group["nesterov"]),
                            bool(group["maximize"]), max_norm, norm)
            elif _ext is not None:
                _ext.sgd_step(ps, gs, bs if momentum != 0 else [], fs, float(lr), float(momentum),
                              float(group["dampening"]), float(group["weight_decay"]), bool(group["nesterov"]),
                              bool(group["maximize"]))
            else:
                _ops.sgd_multi(ps, gs, bs, fs, lr, momentum, group["dampening"], group["weight_decay"],
                               group["nesterov"], group["maximize"])
        return loss


class FusedAdam(_Fused, torch.optim.Adam):
    def __init__(self, params, *args, max_grad_norm=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_clip(max_grad_norm)

    def _native(self):
        """Whether doda_optim_step covers every group as it stands (module docstring: the fallbacks)."""
        if _ext is None and not os.path.exists(_lib.LIB_PATH):
            return False
        for group in self.param_groups:
            if group["amsgrad"] or group["capturable"] or group["differentiable"] or group["fused"] or group["foreach"]:
                return False
            if torch.is_tensor(group["lr"]) or any(torch.is_tensor(b) for b in group["betas"]):
                return False
        lists = self.__dict__.setdefault("_doda_lists", {})
        if "fp32_hip" not in lists:     # (what a parameter is changes with the groups or a loaded state dict at the most)
            lists["fp32_hip"] = all(p.is_cuda and p.dtype == torch.float32 for group in self.param_groups for p in group["params"])
        return lists["fp32_hip"]

    def _slow_lists(self, group):
        """(params, grads, exp_avgs, exp_avg_sqs, step tensors, step values) of the parameters that have a gradient; creates the
        missing state as torch's non-fused route does (step: an fp32 scalar on the CPU)."""
        ps, gs, ms, vs, ts, tv = [], [], [], [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("%s does not take sparse gradients" % type(self).__name__)
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            ps.append(p); gs.append(p.grad); ms.append(state["exp_avg"]); vs.append(state["exp_avg_sq"])
            ts.append(state["step"]); tv.append(float(state["step"]))
        return ps, gs, ms, vs, ts, tv

    @torch.no_grad()
    def step(self, closure=None):
        if not self._native():
            if closure is not None:     # the parent evaluates it; the clip needs its gradients first
                with torch.enable_grad():
                    loss = closure()
                if self.clips_in_step:
                    self._torch_clip()
                super().step()
                return loss
            if self.clips_in_step:
                self._torch_clip()
            return super().step()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lists = self.__dict__.setdefault("_doda_lists", {})
        if self.clips_in_step and len(self.param_groups) != 1:
            self._torch_clip()
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            beta1, beta2 = (float(b) for b in group["betas"])
            # steady state: every parameter has a gradient and its state — the lists of the previous step stand, the step counts
            # are the previous ones plus one (the per-tensor dtype / layout / device checks are made by the native call on every step)
            cached = lists.get(gi)
            grads = [p.grad for p in params]
            if cached is not None and cached[0] is params and all(g is not None for g in grads):
                ps, gs, (ms, vs, ts, tv) = params, grads, cached[1:]
            else:
                ps, gs, ms, vs, ts, tv = self._slow_lists(group)
            if not ps:
                continue
            torch._foreach_add_(ts, 1)
            tv = [v + 1.0 for v in tv]
            lists.pop(gi, None)
            if len(ps) == len(params):
                lists[gi] = (params, ms, vs, ts, tv)
            corr = {v: (1.0 - beta1 ** v, math.sqrt(1.0 - beta2 ** v)) for v in set(tv)}
            kind = _lib.OPTIM_ADAMW if group.get("decoupled_weight_decay", False) else _lib.OPTIM_ADAM
            max_norm, norm = self._clip_args(ps[0].device)
            _optim_step(kind, ps, gs, ms, vs, [corr[v][0] for v in tv], [corr[v][1] for v in tv], [], float(group["lr"]), beta1,
                        beta2, float(group["eps"]), float(group["weight_decay"]), False, bool(group["maximize"]), max_norm, norm)
        return loss


class FusedAdamW(FusedAdam, torch.optim.AdamW):
    """torch.optim.AdamW (its defaults, decoupled_weight_decay set) with FusedAdam's step()."""

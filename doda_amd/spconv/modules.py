"""SparseModule marker base class and SparseSequential container (spconv v1.2 `spconv.modules`;
reference imports at model/unet_block.py:3-4, uses at model/unet.py:35,42 and
model/unet_block.py:10,41,62-85)."""
from collections import OrderedDict

import torch
from torch import nn
from torch.nn.modules import module as _mod

from .. import nn as _dnn
from .core import SparseConvTensor


class SparseModule(nn.Module):
    """Modules deriving from this are called with the SparseConvTensor itself; anything else in
    a SparseSequential is applied to `.features`."""
    pass


def is_spconv_module(module):
    return isinstance(module, SparseModule)


def any_hooks(modules):
    """Does a hook have to fire: one of the four kinds on any of `modules`, or any global module hook?  Everything that
    bypasses nn.Module.__call__ — _run below, the one-call routes of doda_amd.model — asks here, per call."""
    if (_mod._global_forward_hooks or _mod._global_forward_pre_hooks or _mod._global_backward_hooks
            or _mod._global_backward_pre_hooks):
        return True
    for m in modules:
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
            return True
    return False


def _run(module, *args, **kwargs):
    """module(*args) without nn.Module.__call__'s hook machinery when the module has no hooks: a
    U-Net step makes ~200 child calls and the step is issue-bound on the host."""
    if any_hooks((module,)):
        return module(*args, **kwargs)
    return module.forward(*args, **kwargs)


class SparseSequential(SparseModule):
    """nn.Sequential for mixed sparse / dense-feature modules.

    Accepts positional modules, a single OrderedDict, or keyword-named modules (upstream API).
    Non-sparse modules (BatchNorm1d, ReLU, Identity, DSNorm...) act on `.features`, which is
    re-bound on the same tensor object; they are skipped when the tensor has no active rows."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError("name exists.")
            self.add_module(name, module)

    def __getitem__(self, idx):
        if not (-len(self) <= idx < len(self)):
            raise IndexError("index {} is out of range".format(idx))
        if idx < 0:
            idx += len(self)
        it = iter(self._modules.values())
        for _ in range(idx):
            next(it)
        return next(it)

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError("name exists")
        self.add_module(name, module)

    def forward(self, input, residual=None):
        """residual (extension over spconv): feature matrix added to the output of the sequence; when
        the last module is a sparse convolution the add is fused into its kernel.  residual="input" adds
        the sequence's own input features (identity skip of a residual block): if the sequence starts
        with a fused BatchNorm the skip's gradient is summed inside that BatchNorm's backward kernel."""
        mods = list(self._modules.values())
        k = 0
        take_input = isinstance(residual, str)
        if take_input:
            assert residual == "input"
            residual = input.features
        while k < len(mods):
            module = mods[k]
            k += 1
            if is_spconv_module(module):
                if residual is not None and k == len(mods) and getattr(module, "supports_residual", False):
                    input = _run(module, input, residual=residual)
                    residual = None
                else:
                    input = _run(module, input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    if _dnn.fusable(module, input.features):
                        # BatchNorm1d [-> ReLU] on .features: one fused HIP path (doda_amd.nn); when the
                        # features came out of a conv that accumulated their statistics, those are used
                        relu = k < len(mods) and type(mods[k]) is nn.ReLU
                        stats = input.stats()
                        if take_input and k == 1 and module.training:
                            input.features, residual = _dnn.batch_norm_relu(input.features, module, relu, True, stats)
                        else:
                            input.features = _dnn.batch_norm_relu(input.features, module, relu, False, stats)
                        k += int(relu)
                    else:
                        input.features = _run(module, input.features)
            else:
                input = _run(module, input)
        if residual is not None:
            input.features = input.features + residual
        return input


# ---- the plain modules of spconv v1.2 (spconv.modules / spconv.tables / spconv.identity): Python only, CPU tensors included ------
class ToDense(SparseModule):
    """SparseConvTensor -> dense [B, C, X, Y, Z] tensor (the usual end of a network with a dense head)."""

    def forward(self, x):
        return x.dense()


class RemoveGrid(SparseModule):
    """Drops the tensor's grid buffer."""

    def forward(self, x):
        x.grid = None
        return x


class Identity(SparseModule):
    def forward(self, input):
        return input


class ConcatTable(SparseModule):
    """Applies every child to the same input; returns the list of their outputs."""

    def forward(self, input):
        return [module(input) for module in self._modules.values()]

    def add(self, module):
        self._modules[str(len(self._modules))] = module
        return self


class AddTable(SparseModule):
    """Sums the features of a list of tensors over the same voxels into a header of the first."""

    def forward(self, input):
        features = input[0].features
        for t in input[1:]:
            features = features + t.features
        return input[0].header(features)


class JoinTable(SparseModule):
    """Concatenates the features of a list of tensors over the same voxels along the channel dimension."""

    def forward(self, input):
        return input[0].header(torch.cat([t.features for t in input], 1))

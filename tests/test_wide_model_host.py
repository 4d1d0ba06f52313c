"""The coarse plan (UBlock._coarse_modules: the U-Net subtree as one op list, csrc/layers.hip doda_layers_run) at both
backbone widths, on the CPU: the plan takes no BatchNorm wider than the op list's kernels (ops.CX_BN_MAX_C), so the 32-wide
model runs module by module while the 16-wide model keeps its one-call subtree."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bn_widths(plan):
    out = []
    for kind, m, _ in plan:
        mods = list(m.conv_branch._modules.values()) if kind == "rb" else list(m._modules.values())
        out += [b.num_features for b in mods if isinstance(b, torch.nn.BatchNorm1d)]
    return out


def test_coarse_plan_bound_matches_the_kernels_limit():
    from doda_amd import ops
    src = open(os.path.join(ROOT, "doda_amd", "csrc", "bn_totals.hpp")).read()
    assert int(re.search(r"constexpr int BN_TOT_MAX_C = (\d+);", src).group(1)) == ops.CX_BN_MAX_C
    assert "PRE_MAX_C = BN_TOT_MAX_C" in open(os.path.join(ROOT, "doda_amd", "csrc", "spconv_common.hpp")).read()


def test_width16_keeps_the_coarse_plan():
    from doda_amd import ops
    from doda_amd.model import SparseConvNet, default_cfg
    for n_cls in (20, 13, 11, 8):
        net = SparseConvNet(default_cfg(n_classes=n_cls))
        plan = net.unet._coarse_modules()
        assert plan is not False and len(plan) > 0
        assert max(_bn_widths(plan)) == 192 <= ops.CX_BN_MAX_C      # (the level-6 tail: 2 x 96)
        assert net.unet.u.u.u._coarse_modules() is not False


def test_width32_runs_module_by_module():
    from doda_amd import ops
    from doda_amd.model import SparseConvNet, default_cfg
    net = SparseConvNet(default_cfg(mid_channel=32, n_classes=11))
    assert net.unet._coarse_modules() is False
    # every subtree above level 7 carries a BatchNorm over more than 256 channels (320 / 384 at the tails of levels 5 / 6);
    # level 7 alone (224 channels, no tail) stays within the limit
    ub, subtrees = net.unet, []
    while True:
        subtrees.append(ub)
        if len(ub.nPlanes) == 1:
            break
        ub = ub.u
    widths = {}
    for ub in subtrees:
        ub.__dict__.pop("_doda_coarse", None)
        plan = ub._coarse_modules()
        widths[ub.level] = plan
    for lvl in range(1, 7):
        assert widths[lvl] is False, lvl
    assert widths[7] is not False and max(_bn_widths(widths[7])) == 224 <= ops.CX_BN_MAX_C

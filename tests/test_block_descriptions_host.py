"""The cached descriptions behind the one-call routes (doda_amd.model: _Block per ResidualBlock, _Triple per down / up sequence, the
op-list plan per UBlock) follow the module tree: a submodule registered anywhere (setattr, add_module, the BatchNorm conversions)
starts a new structure generation, and every description is made again from the modules that are there now.  On the CPU."""
import torch
from torch import nn


def _net(**kw):
    from doda_amd.model import SparseConvNet, default_cfg
    return SparseConvNet(default_cfg(**kw))


def _plan(ub):
    from doda_amd import model as M
    return M._described(ub, M._describe_subtree)


def test_descriptions_name_a_batchnorm_replaced_by_setattr():
    net = _net()
    blk = net.unet.blocks.block0
    old = blk.conv_branch[0]
    d0, p0 = blk._description(), _plan(net.unet)
    assert d0.bn1 is old and d0.op_list and d0.per_block and p0 is not False and p0[1][0] is d0
    assert blk._description() is d0 and _plan(net.unet) is p0          # cached while nothing is registered
    new = nn.BatchNorm1d(16, eps=1e-4, momentum=0.1)
    setattr(blk.conv_branch, "0", new)
    d1, p1 = blk._description(), _plan(net.unet)
    assert d1.bn1 is new and new in d1.modules and not any(m is old for m in d1.modules)
    assert p1 is not False and p1[0][0][1] is blk and p1[1][0] is d1 and p1[1][0].bn1 is new
    assert any(m is new for m in p1[2]) and not any(m is old for m in p1[2])            # the hook sweep's modules
    assert any(q is new.weight for q in p1[3]) and not any(q is old.weight for q in p1[3])   # the requires_grad sweep's parameters
    # train() / eval() register nothing: the descriptions stay
    net.eval()
    net.train()
    assert blk._description() is d1 and _plan(net.unet) is p1


def test_descriptions_follow_a_conversion_of_the_whole_net():
    from doda_amd import model as M
    net = _net()
    blk, down = net.unet.blocks.block0, net.unet.conv
    assert blk._description() is not None and net.unet._coarse_modules() is not False
    t0 = M._described(down, M._describe_triple)
    assert t0.bn is down[0] and t0.op_list == "down"
    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
    assert type(blk.conv_branch[0]) is torch.nn.SyncBatchNorm
    # not the plain BatchNorm1d of either extension call any more: both routes yield to the modules that are there now
    assert blk._description() is None and net.unet._coarse_modules() is False
    t1 = M._described(down, M._describe_triple)
    assert t1 is not t0 and t1.bn is down[0] and type(t1.bn) is torch.nn.SyncBatchNorm and t1.op_list is None
    assert not any(m is t0.bn for m in t1.modules)


def test_a_false_plan_is_made_again_after_a_replacement(monkeypatch):
    from doda_amd import model as M
    net = _net(mid_channel=32, n_classes=11)
    made = []
    describe = M._describe_subtree
    monkeypatch.setattr(M, "_describe_subtree", lambda ub: made.append(ub.level) or describe(ub))
    assert net.unet._coarse_modules() is False and net.unet._coarse_modules() is False
    assert made == [1]                                                    # the second answer came from the cache
    blk = net.unet.blocks.block0
    blk.conv_branch.add_module("0", nn.BatchNorm1d(32, eps=1e-4, momentum=0.1))
    assert net.unet._coarse_modules() is False
    assert made == [1, 1]                                                 # recomputed, not reused

"""The positional contract between doda_amd.model and the two one-call entry points of the compiled extension
(csrc_ext/doda_torch.cpp: residual_block, coarse_ublock), stated from the module tree and the rulebooks alone: a recorder in the
extension's place sees, slot by slot, the very tensor objects the modules hold."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BN5 = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


class _Recorder:
    """Delegates to the real extension and keeps the positional arguments of the two one-call entry points."""

    def __init__(self, ext):
        self._ext, self.calls = ext, {"coarse_ublock": [], "residual_block": []}

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if name not in self.calls:
            return fn

        def recorded(*args):
            self.calls[name].append(args)
            return fn(*args)
        return recorded


def _walk(ub, steps):
    """The recursive walk of reference model/unet_block.py:87-99."""
    steps += [("rb", blk, ub.level) for blk in ub.blocks]
    if len(ub.nPlanes) > 1:
        steps.append(("down", ub.conv, ub.level))
        _walk(ub.u, steps)
        steps.append(("up", ub.deconv, ub.level))
        steps += [("rb", blk, ub.level) for blk in ub.blocks_tail]
    return steps


def _same(got, want):
    return len(got) == len(want) and all(g is w for g, w in zip(got, want))


def _five(bn):
    return [getattr(bn, k) for k in BN5]


@pytest.fixture(scope="module")
def recorded(native_lib):
    """One bf16 training step of the default network per route, the extension replaced by a recorder."""
    from doda_amd import model as M
    from doda_amd._ext import ext
    from doda_amd.scene import make_batch
    from doda_amd.spconv import functional as Fsp
    from tests.util import deterministic_init
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    d = torch.device("cuda:0")
    cfg = M.default_cfg()
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in make_batch(2, 30000, 9).items()}
    net = deterministic_init(M.SparseConvNet(cfg), seed=5).to(d).train()
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL, Fsp._ext)
    out = {"net": net}
    try:
        assert Fsp.set_deferred_wgrad(True)
        for mode in ("layers", "off"):
            M.set_coarse_mode(mode, 1)
            rec = Fsp._ext = _Recorder(ext)
            net.zero_grad(set_to_none=True)
            inp, p2v, v2p = M.sparse_input(cfg, net, bd, d, torch.bfloat16)
            M.cross_entropy(net(inp, p2v, v2p_map=v2p), bd["labels"]).backward()
            torch.cuda.synchronize()
            out[mode] = (rec.calls, inp.indice_dict)
    finally:
        Fsp._ext = old[2]
        Fsp.set_deferred_wgrad(False)
        M.set_coarse_mode(*old[:2])
    return out


def test_op_list_slots_are_the_modules_tensors(recorded):
    calls, book = recorded["layers"]
    steps = _walk(recorded["net"].unet, [])
    assert len(steps) == 38 and [s[0] for s in steps].count("rb") == 26
    assert len(calls["coarse_ublock"]) == 1 and not calls["residual_block"]          # the op list ran, and only it
    feats, stats_in, kinds, tensors, scalars, training = calls["coarse_ublock"][0][:6]
    assert training is True and kinds == [{"rb": 0, "down": 1, "up": 2}[s[0]] for s in steps]
    assert len(tensors) == len(scalars) == 38
    rows = {lvl: book["subm%d" % lvl].tbl.shape[1] for lvl in range(1, 8)}
    assert rows[1] == feats.shape[0] and min(rows.values()) >= 2
    for (kind, m, lvl), t, s in zip(steps, tensors, scalars):
        if kind == "rb":
            bn1, _, conv1, bn2, _, conv2 = m.conv_branch
            skip = m.i_branch[0]
            assert len(t) == 22 and t[0] is book["subm%d" % lvl].tbl
            assert _same(t[1:6], _five(bn1)) and t[6] is conv1.weight and _same(t[9:14], _five(bn2)) and t[14] is conv2.weight
            assert all(u is not None and u.is_cuda for u in (t[7], t[8], t[15], t[16]))  # packed forward / data-grad weights
            if type(skip) is torch.nn.Identity:
                assert all(u is None for u in t[17:22])
            else:
                assert t[17] is skip.weight and t[18] is not None and t[19] is not None
                assert t[20].dtype == torch.int32 and torch.equal(t[20], torch.arange(rows[lvl], dtype=torch.int32, device=t[20].device).view(1, -1))
                assert t[21] is None or t[21] is t[20]
            assert s == [bn1.eps, bn1.momentum, bn2.eps, bn2.momentum]
        else:
            bn, _, conv = m
            data = book["spconv%d" % lvl]
            assert len(t) == 10 and _same(t[2:7], _five(bn)) and t[7] is conv.weight and t[8] is not None and t[9] is not None
            if kind == "down":
                assert t[0] is data.tbl and t[1] is data.tbl_rev and s == [bn.eps, bn.momentum, rows[lvl + 1]]
            else:
                assert t[0] is data.tbl_rev and t[1] is data.tbl and s == [bn.eps, bn.momentum, rows[lvl]]


def test_residual_block_slots_are_the_modules_tensors(recorded):
    calls, book = recorded["off"]
    blocks = [s for s in _walk(recorded["net"].unet, []) if s[0] == "rb"]
    assert len(calls["residual_block"]) == 26 == len(blocks) and not calls["coarse_ublock"]   # one call per block, no op list
    for (_, m, lvl), a in zip(blocks, calls["residual_block"]):
        bn1, _, conv1, bn2, _, conv2 = m.conv_branch
        x, _, l1, l2, training, mom1, eps1, mom2, eps2, cv1, cv2, rb, n_out, skip, _, sc = a[:16]
        assert _same(l1, _five(bn1)) and _same(l2, _five(bn2)) and training is True
        assert (mom1, eps1, mom2, eps2) == (bn1.momentum, bn1.eps, bn2.momentum, bn2.eps)
        assert len(cv1) == len(cv2) == 3 and cv1[0] is conv1.weight and cv2[0] is conv2.weight
        assert len(rb) == 5 and rb[0] is book["subm%d" % lvl].tbl and n_out == rb[0].shape[1] == x.shape[0]
        assert not (skip is not None and len(sc) > 0)
        if type(m.i_branch[0]) is torch.nn.Identity:
            assert skip is None and len(sc) == 0
        else:                                     # (training mode, DODA_SKIP_FUSION on: the 1x1 skip runs inside the call)
            assert skip is None and len(sc) == 5 and sc[0] is m.i_branch[0].weight and sc[3].shape == (1, x.shape[0])

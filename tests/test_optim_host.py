"""The optimizer step with the clip folded in, host side (no GPU): the companion C ABI include/doda_optim.h and its argument errors,
build_optimizer's routing, FusedAdam / FusedAdamW on CPU parameters (the fallback to torch's own step), state-dict round trips with
plain torch optimizers, the fallback conditions, and the fp64 restatement of tests/optim_cases.py against torch's optimizers."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import optim_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optim_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses before anything is launched; nothing to update is nothing to do."""
    from doda_amd import _lib
    lib = native_lib
    assert lib.doda_optim_workspace_bytes(0) == 0 and lib.doda_optim_workspace_bytes(-3) == 0
    assert lib.doda_optim_workspace_bytes(1) == 64 + 8 * oc.NORM_BLOCKS            # one 56-byte descriptor, 16-byte aligned
    assert lib.doda_optim_workspace_bytes(281) == 281 * 56 + 8 + 8 * oc.NORM_BLOCKS

    def tensors(**kw):
        arr = (_lib.OptimTensor * 2)()
        for k in range(2):
            d = dict(p=16, g=32, state1=48, state2=64, n=5, bias_correction1=0.1, bias_correction2_sqrt=0.03, first_step=0)
            d.update(kw)
            for name, v in d.items():
                setattr(arr[k], name, v)
        return arr

    def step(**kw):
        d = dict(t=tensors(), n=2, kind=_lib.OPTIM_ADAM, hyper=C.pointer(_lib.OptimHyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)), max_norm=0.0,
                 norm=None, ws=64, wsb=1 << 20, stream=None)
        d.update(kw)
        return lib.doda_optim_step(*d.values())
    assert step(n=0, t=None, hyper=None, ws=None, wsb=0) == 0                      # no tensors: nothing to do, nothing looked at
    assert step(n=-1) == -1
    for name in ("t", "hyper", "ws"):
        assert step(**{name: None}) == -1, name
    assert step(kind=3) == -1 and step(kind=-1) == -1
    assert step(ws=72) == -1                                                        # misaligned workspace
    assert step(max_norm=10.0) == -1                                                # a clip without the norm's scalar
    for kind in (_lib.OPTIM_SGD, _lib.OPTIM_ADAM, _lib.OPTIM_ADAMW):
        assert step(kind=kind, t=tensors(p=None)) == -1 and step(kind=kind, t=tensors(g=None)) == -1
        assert step(kind=kind, t=tensors(n=-1)) == -1 and step(kind=kind, t=tensors(n=1 << 31)) == -1
    for kind in (_lib.OPTIM_ADAM, _lib.OPTIM_ADAMW):                                # a missing state buffer
        assert step(kind=kind, t=tensors(state1=None)) == -1 and step(kind=kind, t=tensors(state2=None)) == -1
    assert step(kind=_lib.OPTIM_SGD, t=tensors(state1=None)) == -1                  # (beta1 carries the momentum: 0.9 here)
    assert step(wsb=lib.doda_optim_workspace_bytes(2) - 1) == -5
    assert step(wsb=lib.doda_optim_workspace_bytes(2) - 1, max_norm=10.0, norm=128) == -5
    # every tensor empty: OK without a launch, with and without the clip; SGD without momentum needs no buffer
    assert step(t=tensors(n=0)) == 0 and step(t=tensors(n=0), max_norm=10.0, norm=128) == 0
    sgd0 = C.pointer(_lib.OptimHyper(1e-3, 0.0, 0.0, 0.0, 0.0, 0, 0))
    assert step(kind=_lib.OPTIM_SGD, hyper=sgd0, t=tensors(n=0, state1=None, state2=None)) == 0


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(**kw):
    return _Cfg(dict(base_lr=0.01, momentum=0.9, weight_decay=1e-4), **kw)


def test_build_optimizer_routing_on_the_cpu_and_with_fused_off():
    """CPU parameters and fused=False return plain torch optimizers, clip_grad or not (the training loop clips there)."""
    from doda_amd.train import build_optimizer
    net = torch.nn.Linear(3, 2)
    for kind, cls in (("sgd", torch.optim.SGD), ("adam", torch.optim.Adam), ("adamw", torch.optim.AdamW)):
        for clip in (False, True):
            for fused in (None, False):
                o = build_optimizer(_cfg(optim=kind, clip_grad=clip), net, fused=fused)
                assert type(o) is cls and not getattr(o, "clips_in_step", False)
                assert o.param_groups[0]["lr"] == 0.01
    assert type(build_optimizer(_cfg(), net)) is torch.optim.SGD
    with pytest.raises(NotImplementedError):
        build_optimizer(_cfg(optim="lamb"), net)


def test_build_optimizer_routing_for_device_parameters(monkeypatch):
    """What build_optimizer hands out for fp32 device parameters, decided on a stand-in for the device test (no GPU here): the
    classes of doda_amd.optim, max_grad_norm = 10 under clip_grad; a non-fp32 parameter keeps torch's class."""
    from doda_amd import optim, train

    class P:                                   # what build_optimizer asks of a parameter
        requires_grad, is_cuda, dtype = True, True, torch.float32

    class Net:
        def __init__(self, ps):
            self.ps = ps

        def parameters(self):
            return iter(self.ps)
    made = []
    for name in ("FusedSGD", "FusedAdam", "FusedAdamW"):
        monkeypatch.setattr(optim, name, (lambda n: lambda params, **kw: made.append((n, kw)) or n)(name))
    for kind, name in (("sgd", "FusedSGD"), ("adam", "FusedAdam"), ("adamw", "FusedAdamW")):
        for clip in (False, True):
            del made[:]
            assert train.build_optimizer(_cfg(optim=kind, clip_grad=clip), Net([P(), P()])) == name
            kw = made[0][1]
            assert kw.pop("lr") == 0.01 and kw.pop("max_grad_norm", None) == (10 if clip else None)
            assert kw == (dict(momentum=0.9, weight_decay=1e-4) if kind == "sgd" else {})
    half = P()
    half.dtype = torch.float16
    monkeypatch.setattr(torch.optim, "AdamW", lambda params, **kw: ("torch", kw))
    assert train.build_optimizer(_cfg(optim="adamw", clip_grad=True), Net([P(), half])) == ("torch", dict(lr=0.01, fused=True))


def _pair(cls, ref, shapes, **kw):
    g = torch.Generator().manual_seed(5)
    a = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    return a, b, cls(a, **kw), ref(b, **{k: v for k, v in kw.items() if k != "max_grad_norm"})


@pytest.mark.parametrize("name", ["FusedAdam", "FusedAdamW"])
@pytest.mark.parametrize("clip", [None, 1.5])
def test_fused_adam_on_cpu_parameters_is_torchs(name, clip):
    """CPU parameters: the parent's step (after torch's clip_grad_norm_ under max_grad_norm), bit for bit; a parameter without a
    gradient, lr changed between steps, a state-dict round trip into a fresh instance."""
    from doda_amd import optim
    cls, ref = getattr(optim, name), getattr(torch.optim, name[5:])
    kw = dict(lr=0.01, weight_decay=0.02, betas=(0.8, 0.99))
    a, b, oa, ob = _pair(cls, ref, [(7, 3), (5,), (2, 2, 2), (4,)], max_grad_norm=clip, **kw)
    assert oa.clips_in_step == (clip is not None) and oa.last_grad_norm is None
    assert isinstance(oa, ref) and oa.param_groups[0]["decoupled_weight_decay"] == (name == "FusedAdamW")
    gg = torch.Generator().manual_seed(9)
    for it in range(4):
        if it == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 0.003
        if it == 3:
            sd = oa.state_dict()
            oa = cls(a, max_grad_norm=clip, **kw)
            oa.load_state_dict(sd)
        for p, q in zip(a[:-1], b[:-1]):
            p.grad = torch.randn(p.shape, generator=gg)
            q.grad = p.grad.clone()
        norm = torch.nn.utils.clip_grad_norm_(b, clip) if clip is not None else None
        oa.step(); ob.step()
        for p, q in zip(a, b):
            assert torch.equal(p, q)
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad)          # (the clipped gradient stays in p.grad)
        if clip is not None:
            assert oa.last_grad_norm.dtype == torch.float32 and torch.equal(oa.last_grad_norm, norm)
    for p, q in zip(a[:-1], b[:-1]):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[p][key], ob.state[q][key])
    assert a[-1] not in oa.state or not oa.state[a[-1]]


@pytest.mark.parametrize("name", ["FusedSGD", "FusedAdam", "FusedAdamW"])
def test_state_dict_round_trips_with_plain_torch(name):
    """state_dict() is torch's, key for key: into the plain optimizer and back, max_grad_norm left out of it."""
    from doda_amd import optim
    cls, ref = getattr(optim, name), getattr(torch.optim, name[5:])
    kw = dict(lr=0.01, momentum=0.9) if name == "FusedSGD" else dict(lr=0.01)
    a, b, oa, ob = _pair(cls, ref, [(3, 2), (4,)], **kw)
    for p, q in zip(a, b):
        p.grad = torch.ones_like(p)
        q.grad = torch.ones_like(q)
    ob.step()
    sd = copy.deepcopy(ob.state_dict())                  # (torch hands out and takes in the step tensors themselves)
    oa.load_state_dict(copy.deepcopy(sd))                # plain -> fused
    back = oa.state_dict()
    assert back["param_groups"] == sd["param_groups"] and "max_grad_norm" not in str(back["param_groups"])
    assert set(back["state"]) == set(sd["state"])
    for k in sd["state"]:
        assert set(back["state"][k]) == set(sd["state"][k])
        for key, v in sd["state"][k].items():
            assert torch.equal(back["state"][k][key], v) and back["state"][k][key].device == v.device
    fresh = ref(b, **kw)
    fresh.load_state_dict(copy.deepcopy(back))           # fused -> plain
    if name != "FusedSGD":                               # CPU parameters: both continue with torch's step, on the same state
        oa.step(); ob.step(); fresh.step()
        for p, q in zip(a, b):
            assert float(oa.state[p]["step"]) == float(fresh.state[q]["step"]) == 2.0
            assert oa.state[p]["step"].device.type == "cpu" and oa.state[p]["step"].dtype == torch.float32


def test_max_grad_norm_is_validated_and_off_by_default():
    from doda_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (optim.FusedSGD, optim.FusedAdam, optim.FusedAdamW):
        o = cls(p, lr=0.1)
        assert o.max_grad_norm is None and not o.clips_in_step and o.last_grad_norm is None
        assert cls(p, lr=0.1, max_grad_norm=10).max_grad_norm == 10.0
        for bad in (0, -1.0, float("nan")):
            with pytest.raises(ValueError):
                cls(p, lr=0.1, max_grad_norm=bad)


def test_fused_adam_fallback_conditions(monkeypatch):
    """_native() is false — the parent's step runs — for amsgrad, capturable, differentiable, an explicit fused / foreach, a tensor
    lr, CPU or non-fp32 parameters and a missing native library; true for fp32 device parameters otherwise (decided here on
    the group flags, with the per-parameter answer given)."""
    from doda_amd import _lib, optim
    p = [torch.nn.Parameter(torch.zeros(3))]

    def native(device_params=True, **kw):
        o = optim.FusedAdamW(p, **kw)
        o._doda_lists = {"fp32_hip": True} if device_params else {}
        return o._native()
    assert native() and native(lr=0.1, weight_decay=0.0, maximize=True)
    assert not native(device_params=False)                       # CPU parameters
    for kw in (dict(amsgrad=True), dict(capturable=True), dict(differentiable=True), dict(foreach=True), dict(lr=torch.tensor(0.01))):
        assert not native(**kw), kw
    o = optim.FusedAdamW(p)
    o.param_groups[0]["fused"] = True                            # (torch's constructor refuses fused=True on CPU parameters)
    o._doda_lists = {"fp32_hip": True}
    assert not o._native()
    half = optim.FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    assert not half._native()
    monkeypatch.setattr(optim, "_ext", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "no_such_library.so"))
    assert not native()
    # sparse gradients are refused where the native step would run
    o = optim.FusedAdam(p)
    p[0].grad = torch.sparse_coo_tensor([[0]], [1.0], (3,))
    with pytest.raises(RuntimeError, match="sparse"):
        o._slow_lists(o.param_groups[0])
    p[0].grad = None


HYPERS = {
    "sgd": [dict(lr=0.05), dict(lr=0.05, momentum=0.9, weight_decay=1e-4), dict(lr=0.05, momentum=0.8, dampening=0.3, maximize=True),
            dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2)],
    "adam": [dict(lr=1e-2), dict(lr=1e-2, weight_decay=0.1, betas=(0.8, 0.99)), dict(lr=1e-2, maximize=True, eps=1e-6)],
    "adamw": [dict(lr=1e-2, weight_decay=1e-2), dict(lr=1e-2, weight_decay=0.1, betas=(0.8, 0.99)), dict(lr=1e-2, weight_decay=0.3, maximize=True)],
}


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
@pytest.mark.parametrize("clip", [None, oc.MAX_NORM])
def test_restatement_is_torchs_optimizer_in_float64(kind, clip):
    """tests/optim_cases.py against torch.optim.SGD / Adam / AdamW(foreach=False) and clip_grad_norm_ on float64 CPU tensors, four
    steps, lr changed after two, a tensor without gradient.  Both sides round every fp64 operation (2^-53) and differ only in how
    they associate a handful of them per step (torch's lerp and addcdiv forms): 1e-10 relative leaves four decimal orders over
    that and stays seven below the fp32 ulp the device tests resolve."""
    specs = [dict(shape=(33,), offset=0, grad=True), dict(shape=(4, 5), offset=0, grad=True), dict(shape=(6,), offset=0, grad=False)]
    cls = dict(sgd=torch.optim.SGD, adam=torch.optim.Adam, adamw=torch.optim.AdamW)[kind]
    for hyper in HYPERS[kind]:
        p0 = oc.make_params(specs, 1)
        tp = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in p0]
        opt = cls(tp, foreach=False, **hyper)
        rs = oc.Restated(kind, p0, max_norm=clip, **hyper)
        for it in range(4):
            if it == 2:
                opt.param_groups[0]["lr"] = rs.hyper["lr"] = hyper["lr"] / 4
            grads = oc.make_grads(specs, "large" if it % 2 == 0 else "small", 10 + it)
            for p, g in zip(tp, grads):
                p.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
            norm_t = torch.nn.utils.clip_grad_norm_(tp, clip) if clip is not None else None
            opt.step()
            norm, coef, scaled = rs.step(grads)
            if clip is not None:
                np.testing.assert_allclose(norm, float(norm_t), rtol=1e-13)
                assert (coef == 1.0) == (it % 2 == 1)            # the 'small' set is below the threshold, the 'large' one above
                for p, g in zip(tp, scaled):
                    if g is not None:
                        np.testing.assert_allclose(p.grad.numpy(), g, rtol=1e-13, atol=0)
            for k, p in enumerate(tp):
                np.testing.assert_allclose(p.detach().numpy(), rs.p[k], rtol=1e-10, atol=1e-13)
                st = opt.state.get(p, {})
                if "momentum_buffer" in st and st["momentum_buffer"] is not None:
                    np.testing.assert_allclose(st["momentum_buffer"].numpy(), rs.s1[k], rtol=1e-10, atol=1e-13)
                if "exp_avg" in st:
                    np.testing.assert_allclose(st["exp_avg"].numpy(), rs.s1[k], rtol=1e-10, atol=1e-13)
                    np.testing.assert_allclose(st["exp_avg_sq"].numpy(), rs.s2[k], rtol=1e-10, atol=1e-16)
        assert rs.s1[2] is None and np.array_equal(rs.p[2], p0[2].astype(np.float64))


def test_designed_sets_cover_what_they_claim():
    T, cap = oc.TILE, oc.NORM_BLOCKS
    sizes = [oc.numel(s) for s in oc.edge_set()]
    assert {1, 3, T - 1, T, T + 1, 2 * T + 5, 27 * 16 * 16, 0} <= set(sizes)
    assert any(s["offset"] == 1 and oc.numel(s) > T for s in oc.edge_set()) and any(not s["grad"] for s in oc.edge_set())
    assert len(oc.many_set()) >= 300
    big = oc.big_set()
    tiles = sum(-(-oc.numel(s) // T) for s in big)
    assert cap < tiles <= cap + 8 and 4 * sum(oc.numel(s) for s in big) < 5 << 20
    for specs in (oc.edge_set(), oc.many_set()):
        n = lambda kind: oc.grad_norm(oc.make_grads(specs, kind, 3))
        assert n("large") > 5 * oc.MAX_NORM and n("small") < oc.MAX_NORM / 2 and np.isnan(n("nan"))
        assert oc.clip_coef(n("small")) == 1.0 and oc.clip_coef(n("large")) < 0.2 and np.isnan(oc.clip_coef(n("nan")))
        mixed = oc.make_grads(specs, "mixed", 3)
        sq = np.concatenate([np.square(g.reshape(-1)) for g in mixed if g is not None])     # fp32 squares
        seq = np.float32(0)
        for v in np.sort(sq)[::-1][:4096]:      # an fp32 running sum, large terms first, stops moving at the small ones
            seq = np.float32(seq + v)
        assert np.float32(seq + np.float32(1e-8)) == seq and sq.min() < 1e-6 < 1e6 < sq.max()

"""doda_spconv_wgrad_multi as ONE call (csrc/spconv_wgrad.hip make_call_plan over csrc/wgrad_plan.hpp): every kernel class — tile, wide, pair lists,
gather table — and every regime of the shared fixed-order reduction (csrc/wgrad_common.hpp wgrad_fold: 1, 2 .. 16 and more
than 16 chunks, the scalar reduce of an element count that is no multiple of four) side by side, in overwrite and in
accumulate mode, plus empty jobs; the workspace / descriptor contract of the call (an error return has enqueued nothing);
and the wide kernel's bit-equality with the gather-table kernel at a small shape.  One raster scene of ~3 000 voxels."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.util import surface_voxels

pytestmark = pytest.mark.gpu

DODA_ERR_WORKSPACE = -5      # include/doda_hip.h


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def ref_dw(x, dy, tbl, n_rows):
    """fp64 dw[o] = sum_{t < n_rows} x[tbl[o][t]]^T dy[t]"""
    out = torch.empty(tbl.shape[0], x.shape[1], dy.shape[1], dtype=torch.float64, device=x.device)
    for o in range(tbl.shape[0]):
        nbo = tbl[o, :n_rows].long()
        ok = nbo >= 0
        out[o] = x[nbo[ok]].double().t() @ dy[:n_rows][ok].double()
    return out


def check(kind, got, ref):
    """the bounds of the existing tests of each class: max error against the largest entry < 1e-4 (test_gpu_round2/3/4,
    and test_gpu_parity's RTOL for float32); the wide class: norm < 1e-4 and max < 1e-3 (test_gpu_wgrad_wide)"""
    err = (got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)
    if kind == "wide":
        rel = float((got.double() - ref).norm() / ref.norm())
        assert rel < 1e-4 and float(err) < 1e-3, (kind, rel, float(err))
    else:
        assert float(err) < 1e-4, (kind, float(err))


@pytest.fixture(scope="module")
def case():
    """[(name, kind, job tuple without dw, fp64 reference)] and the scene's table"""
    from doda_amd import ops
    d = dev()
    shape, batch = [40, 36, 30], 1
    idx = surface_voxels(3001, 3001, batch, list(shape)).astype(np.int64)
    key = ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
    idx = torch.from_numpy(np.ascontiguousarray(idx[np.argsort(key, kind="stable")].astype(np.int32))).to(d)
    tbl = ops.rulebook_subm(idx, shape, batch, 3)
    n = tbl.shape[1]
    assert 2049 <= n <= 4096      # two row ranges of the pair kernel, 2 .. 16 chunks of the gather-table plan
    tb = ops.tilebook_build(tbl)
    pr, num, seg = ops.rulebook_pairs(tbl, n, flip=True, pad=False, with_seg=True)
    g = torch.Generator().manual_seed(5)

    def rnd(rows, c, dt=torch.bfloat16):
        return torch.randn(rows, c, generator=g).to(dt).to(d)
    out = []

    def table_job(name, kind, ca, cb, tilebook=None, table=tbl, rows=n, n_a=n, dt=torch.bfloat16):
        x, dy = rnd(n_a, ca, dt), rnd(rows, cb, dt)
        out.append((name, kind, (x, dy, table, rows, None), tilebook, ref_dw(x, dy, table, rows)))
    table_job("tile 16->16", "tile", 16, 16, tb)
    table_job("wide 48->48", "wide", 48, 48, tb)
    table_job("wide 96->48", "wide", 96, 48, tb)
    # pair lists: the scene's (two row ranges), identity lists of one range and of more than 16 ranges
    x, dy = rnd(n, 16), rnd(n, 32)
    out.append(("pairs 2 ranges", "pairs", (x, dy, tbl, n, (pr[0], pr[1], num, seg)), None, ref_dw(x, dy, tbl, n)))
    for rows in (1500, 34817):
        x, dy = rnd(rows, 16), rnd(rows, 16)
        ident = torch.arange(rows, dtype=torch.int32, device=d).view(1, rows)
        out.append(("pairs identity %d" % rows, "pairs", (x, dy, None, rows, (ident, ident, None, None)), None,
                    (x.double().t() @ dy.double()).view(1, 16, 16)))
    # gather table: 1 chunk (700 rows), 2 .. 16 chunks (the scene), more than 16 chunks (20 000 rows of a random table)
    table_job("dense 1 chunk", "dense", 32, 32, rows=700)
    table_job("dense 2..16 chunks", "dense", 32, 16)
    big = torch.randint(0, n, (27, 20000), generator=g, dtype=torch.int32)
    big[torch.rand(27, 20000, generator=g) < 0.6] = -1
    table_job("dense >16 chunks", "dense", 16, 16, table=big.to(d), rows=20000)
    # float32, 27 x 5 x 5 = 675 elements: no multiple of four, the scalar reduce
    table_job("dense f32 5->5", "dense", 5, 5, dt=torch.float32)
    return out, tbl


def job_list(case, bases):
    """every job in overwrite mode, then every job accumulating into bases[k] (cloned), then an empty job of each mode"""
    d = dev()
    jobs = [j + (None, tbk) for _, _, j, tbk, _ in case]
    jobs += [j + (b.clone(), tbk) for (_, _, j, tbk, _), b in zip(case, bases)]
    empty = (torch.zeros(1, 16, device=d).bfloat16(), torch.zeros(1, 16, device=d).bfloat16(),
             torch.full((27, 1), -1, dtype=torch.int32, device=d), 0, None)
    return jobs + [empty + (None, None), empty + (bases[0].clone(), None)]


@pytest.fixture(scope="module")
def bases(case):
    g = torch.Generator().manual_seed(6)
    return [torch.randn(ref.shape, generator=g).to(dev()) for _, _, _, _, ref in case[0]]


def test_every_class_and_reduce_regime_in_one_call(native_lib, case, bases):
    from doda_amd import ops
    case, _ = case
    jobs = job_list(case, bases)
    outs = ops.spconv_wgrad_multi(jobs)
    nc = len(case)
    for k, (name, kind, _, _, ref) in enumerate(case):
        check(kind, outs[k], ref)
        check(kind, outs[nc + k], ref + bases[k].double())
    assert float(outs[2 * nc].abs().max()) == 0.0                      # the empty job: zeros, or the gradient as it was
    assert torch.equal(outs[2 * nc + 1], bases[0])
    # a repeated call: bit-equal
    again = ops.spconv_wgrad_multi(job_list(case, bases))
    for a, b in zip(outs, again):
        assert torch.equal(a, b)
    # every job in a call of its own: bit-equal — but the tile jobs, whose workgroups' chunks depend on the number of channel
    # blocks in a launch (test_gpu_round3.py: to rounding only)
    for k, job in enumerate(job_list(case, bases)[:2 * nc]):
        alone, = ops.spconv_wgrad_multi([job])
        name, kind = case[k % nc][:2]
        if kind == "tile":
            assert float((alone - outs[k]).abs().max() / outs[k].abs().max()) < 1e-5, name
        else:
            assert torch.equal(alone, outs[k]), (name, k >= nc)


def test_an_error_return_has_enqueued_nothing(native_lib, case, bases):
    """Workspace contract: exactly doda_spconv_wgrad_multi_workspace_bytes succeeds; 256 bytes fewer (the byte count only: the
    buffer stays whole) or a descriptor buffer one byte short return DODA_ERR_WORKSPACE with every dw untouched."""
    from doda_amd import ops
    case, _ = case
    plan = ops.WgradPlan(job_list(case, bases))
    lib, d = ops.lib(), dev()
    need = lib.doda_spconv_wgrad_multi_workspace_bytes(C.addressof(plan._arr), plan._n)
    dneed = lib.doda_spconv_wgrad_multi_desc_bytes(plan._n)
    ws = torch.empty(need, dtype=torch.uint8, device=d)
    desc = torch.empty(dneed, dtype=torch.uint8, device=d)

    def call(ws_bytes, desc_bytes):
        return lib.doda_spconv_wgrad_multi(C.addressof(plan._arr), plan._n, ops._p(ws), ws_bytes, ops._p(desc), desc_bytes,
                                           ops._stream())
    want = [o.clone() for o in plan.outputs]      # (the accumulating jobs: base + sum)
    for o, b in zip(plan.outputs[len(case):], bases):
        o.copy_(b)
    assert call(need, dneed) == 0
    torch.cuda.synchronize()
    for o, w in zip(plan.outputs, want):
        assert torch.equal(o, w)
    for ws_bytes, desc_bytes in ((need - 256, dneed), (need, dneed - 1)):
        for o in plan.outputs:
            o.fill_(-7.5)
        assert call(ws_bytes, desc_bytes) == DODA_ERR_WORKSPACE
        torch.cuda.synchronize()
        for o in plan.outputs:
            assert bool((o == -7.5).all())


def test_wide_is_bit_equal_to_the_gather_table_kernel_at_a_small_shape(native_lib, case):
    """the wide kernel and the gather-table kernel sum over the same row chunks and reduce through the same fold: the same
    bits, in overwrite and accumulate mode (test_gpu_wgrad_wide.py asserts it at bench size)"""
    from doda_amd import ops
    case, tbl = case
    for name, kind, job, tb, _ in case:
        if kind != "wide":
            continue
        wide, = ops.spconv_wgrad_multi([job + (None, tb)])
        dense, = ops.spconv_wgrad_multi([job])
        assert torch.equal(wide, dense), name
        base = torch.randn_like(wide)
        wide_acc, = ops.spconv_wgrad_multi([job + (base.clone(), tb)])
        dense_acc, = ops.spconv_wgrad_multi([job + (base.clone(),)])
        assert torch.equal(wide_acc, dense_acc), name

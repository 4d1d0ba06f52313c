"""Per-layer backend of the coarse-level op list (csrc/layers.hip, ABI 11: doda_layers_run) and the BatchNorm folded into the
convolution's gather (doda_conv_prologue; reference model/unet_block.py:23-30,46-49,67-79: BatchNorm1d -> ReLU -> conv, 65
pairs per forward pass of model/unet.py:42-45), at the row / channel counts of the U-Net's levels 4-7.

Checked against: torch.nn.functional.batch_norm (+ autograd for the backward), the oracle's indice_conv on the normalised rows
(bf16 tolerance: 2^-7 of the tensor's scale), and the UNFOLDED form of the same op list, whose BatchNorm outputs must be
bit-equal (the folded transform is the standalone sweep's arithmetic, operation for operation: csrc/bn_totals.hpp).
"""
import numpy as np
import pytest
import torch

from tests.util import surface_voxels

pytestmark = pytest.mark.gpu

BIG = 1 << 30


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def _bf(t):
    return t.to(torch.bfloat16)


def _pack(w, K, kc, nc, layout, d):
    from doda_amd import ops
    plan = ops.PackPlan([(w, K, kc, nc, layout, 2)], d)
    plan.run()
    return plan.outputs[0]


def _scale_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


LEVELS = [(8400, 64), (1900, 80), (420, 96), (83, 112)]


def _level(seed, n, batch=4):
    side = max(16, int(round((n / batch / 0.08) ** (1 / 3))))   # ~8 % occupancy: 10-14 neighbours per voxel
    shape = [side, side, side]
    idx = surface_voxels(seed, n, batch, shape)
    return np.ascontiguousarray(idx[:n]), shape, batch



def _unet_step(mode, level, dtype=torch.bfloat16, voxels=60000, seed=11, two_pass=False):
    """One training step of the U-Net on a seeded batch with the executor on / off: (logits, loss, {name: grad}, running stats)."""
    from doda_amd import model as M
    from doda_amd.model import SparseConvNet, cross_entropy, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from doda_amd.spconv import functional as Fsp
    from tests.util import deterministic_init
    d = dev()
    cfg = default_cfg()
    batch = make_batch(2, voxels, seed)
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in batch.items()}
    net = deterministic_init(SparseConvNet(cfg), seed=3).to(d).train()
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
    M.set_coarse_mode(mode, level)
    try:
        assert Fsp.set_deferred_wgrad(True)
        net.zero_grad(set_to_none=True)
        scores = voxelize_and_run(cfg, net, bd, d, feature_dtype=dtype)
        loss = cross_entropy(scores, bd["labels"])
        loss.backward()
        if two_pass:   # a second backward pass into the same .grad tensors (tool/st.py:136-198 runs two per optimizer step)
            scores2 = voxelize_and_run(cfg, net, bd, d, feature_dtype=dtype)
            cross_entropy(scores2, bd["labels"]).backward()
        torch.cuda.synchronize()
    finally:
        Fsp.set_deferred_wgrad(False)
        M.set_coarse_mode(*old)
    grads = {n: p.grad.detach().float().clone() for n, p in net.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in net.named_buffers()}
    return scores.detach().float(), float(loss.detach()), grads, bufs


def _subtree(level, n, seed):
    """UBlock(level) of a freshly initialised U-Net plus a level-`level` input of n voxels."""
    from doda_amd.model import SparseConvNet, default_cfg
    from tests.util import deterministic_init
    d = dev()
    net = deterministic_init(SparseConvNet(default_cfg()), seed=seed).to(d).train()
    ub = net.unet
    for _ in range(level - 1):
        ub = ub.u
    idx, shape, batch = _level(seed + n, n)
    q = 2 ** (8 - level)
    shape = [max(q, s + (-s) % q) for s in shape]   # every deeper level keeps >= 2 cells per axis
    ind = torch.from_numpy(idx).to(d)
    return net, ub, ind, shape, batch


def _run_subtree(ub, ind, shape, batch, level, x0, gout, mode):
    from doda_amd import model as M
    from doda_amd import spconv
    from doda_amd.spconv import functional as Fsp
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
    M.set_coarse_mode(mode, level)
    try:
        assert Fsp.set_deferred_wgrad(True)
        for p in ub.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        t = spconv.SparseConvTensor(x, ind, shape, batch)
        spconv.ops.build_pyramid(t, 8 - level, first_level=level)
        y = ub(t).features
        (y.float() * gout.float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        Fsp.set_deferred_wgrad(False)
        M.set_coarse_mode(*old)
    return (y.detach().float(), x.grad.detach().float(), {n: p.grad.detach().float().clone() for n, p in ub.named_parameters()},
            {n: b.detach().clone() for n, b in ub.named_buffers()})




def _tables(ops, idx, shape, batch, d):
    return ops.rulebook_subm(torch.from_numpy(idx).to(d), shape, batch, 3)


def _cast(t, dtype):
    return t.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,c", LEVELS)
def test_forward_fold_vs_torch_oracle_and_unfolded(native_lib, oracle, n, c, dtype):
    """BNFWD ; GEMM as one launch: statistics from totals, normalised rows (side output), running statistics, conv output."""
    from doda_amd import ops
    d = dev()
    esz = 2 if dtype == torch.bfloat16 else 4
    idx, shape, batch = _level(n, n)
    n = idx.shape[0]
    pairs, pn = oracle.indice_pairs_subm(idx, batch, shape, 3)
    tbl = _tables(ops, idx, shape, batch, d)
    g = torch.Generator().manual_seed(n + esz)
    for cin, cout in ((c, c), (2 * c, c)):
        x = _cast(torch.randn(n, cin, generator=g) * 1.7 + 0.3, dtype).to(d)
        res = _cast(torch.randn(n, cout, generator=g), dtype).to(d)
        w = (torch.randn(27, cin, cout, generator=g) * (1.0 / (cin * 9)) ** 0.5).to(d)
        wp = ops.PackPlan([(w, 27, cin, cout, 0, esz)], d)
        wp.run()
        wp = wp.outputs[0]
        gamma = (torch.rand(cin, generator=g) + 0.5).to(d)
        beta = (torch.randn(cin, generator=g) * 0.3).to(d)
        ca = cin // 2 if cin == 2 * c else cin      # the concatenation case: two producers' totals
        out = {}
        for fold in (True, False):
            old = ops.set_pre_rows(BIG if fold else 0, BIG if fold else 0)
            try:
                ta, tb = ops.stats_totals(ca, d), (ops.stats_totals(cin - ca, d) if ca < cin else None)
                a = torch.full((n, cin), float("nan"), dtype=dtype, device=d)
                y = torch.full((n, cout), float("nan"), dtype=dtype, device=d)
                ty = ops.stats_totals(cout, d)
                mean, invstd = torch.zeros(cin, device=d), torch.zeros(cin, device=d)
                rm, rv = torch.zeros(cin, device=d), torch.ones(cin, device=d)
                nbt = torch.zeros(1, dtype=torch.int64, device=d)
                lst = [dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=ca, x_ld=cin, x=x, stats=ta)]
                if tb is not None:
                    lst.append(dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=cin - ca, x_ld=cin, x=x[:, ca:], stats=tb))
                lst += [dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU | ops.CX_F_TRAINING, rows=n, c_in=cin, x_ld=cin, y_ld=cin, x=x, y=a,
                             eps=1e-4, momentum=0.1, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, nbt=nbt, mean=mean,
                             invstd=invstd, stats=ta, stats_b=tb, c_split=ca),
                        dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=n, c_in=cin, c_out=cout, K=27, tbl_ld=n, x_ld=cin, y_ld=cout,
                             res_ld=cout, x=a, w=wp, tbl=tbl, y=y, res=res, stats=ty)]
                launches = ops.layers_run(lst, d, esz)
                torch.cuda.synchronize()
            finally:
                ops.set_pre_rows(*old)
            assert launches == len(lst) - (1 if fold else 0), (launches, fold)
            out[fold] = (a, y, mean, invstd, rm, rv, int(nbt), ops.totals_sums(ty), ops.totals_sums(ta))
        (a1, y1, m1, i1, rm1, rv1, nb1, ty1, tx1), (a0, y0, m0, i0, rm0, rv0, nb0, ty0, _) = out[True], out[False]
        # the folded BatchNorm is the unfolded one, bit for bit; the conv differs only in the summation order over offsets
        assert torch.equal(a1.view(torch.int16 if esz == 2 else torch.int32), a0.view(torch.int16 if esz == 2 else torch.int32))
        assert torch.equal(m1, m0) and torch.equal(i1, i0) and torch.equal(rm1, rm0) and torch.equal(rv1, rv0) and nb1 == nb0 == 1
        tol = 2.0 ** -7 if esz == 2 else 1e-5
        assert _scale_err(y1.float(), y0.float()) < tol
        # statistics op: column sums of x
        xd = x.double()
        assert torch.allclose(tx1[0], xd[:, :ca].sum(0), rtol=1e-6, atol=1e-6 * n)
        assert torch.allclose(tx1[1], (xd[:, :ca] ** 2).sum(0), rtol=1e-6, atol=1e-6 * n)
        # torch: BatchNorm1d(training) + ReLU on the same x
        rm_t, rv_t = torch.zeros(cin, device=d), torch.ones(cin, device=d)
        ref_a = torch.relu(torch.nn.functional.batch_norm(x.float(), rm_t, rv_t, gamma, beta, True, 0.1, 1e-4))
        assert _scale_err(a1.float(), ref_a) < (2.0 ** -7 if esz == 2 else 2e-5)
        assert torch.allclose(rm1, rm_t, rtol=1e-4, atol=1e-5) and torch.allclose(rv1, rv_t, rtol=1e-4, atol=1e-5)
        assert torch.allclose(m1, x.float().mean(0), rtol=1e-4, atol=1e-5)
        # oracle conv on the stored normalised rows
        wq = w.to(dtype).float() if esz == 2 else w
        ref = oracle.indice_conv(a1.float().cpu().numpy(), wq.cpu().numpy().reshape(3, 3, 3, cin, cout), pairs, pn, n, subm=True)
        ref = torch.as_tensor(ref) + res.float().cpu()
        assert _scale_err(y1.float().cpu(), ref) < (2.0 ** -7 if esz == 2 else 1e-4), (cin, cout)
        yd = y1.double()
        assert torch.allclose(ty1[0], yd.sum(0), rtol=1e-5, atol=1e-4 * float(yd.abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,c", LEVELS[1:])
def test_backward_fold_vs_autograd_and_unfolded(native_lib, oracle, n, c, dtype):
    """GEMM(data gradient + BatchNorm-backward totals) ; BNBWD(+ skip gradient) ; GEMM as two launches instead of three: the
    gradient of the BatchNorm's input (side output), dgamma / dbeta and the next data gradient."""
    from doda_amd import ops
    d = dev()
    esz = 2 if dtype == torch.bfloat16 else 4
    idx, shape, batch = _level(n + 5, n)
    n = idx.shape[0]
    pairs, pn = oracle.indice_pairs_subm(idx, batch, shape, 3)
    tbl = _tables(ops, idx, shape, batch, d)
    g = torch.Generator().manual_seed(3 * n + esz)
    u = _cast(torch.randn(n, c, generator=g) * 1.3 - 0.2, dtype).to(d)            # the BatchNorm's input
    dy = _cast(torch.randn(n, c, generator=g), dtype).to(d)                         # gradient of the conv behind the BatchNorm
    add_full = _cast(torch.randn(n, 2 * c, generator=g), dtype).to(d)               # the skip gradient: a column slice (ld = 2c)
    gamma = (torch.rand(c, generator=g) + 0.5).to(d)
    beta = (torch.randn(c, generator=g) * 0.3).to(d)
    w2 = (torch.randn(27, c, c, generator=g) * (1.0 / (c * 9)) ** 0.5).to(d)       # conv behind the BatchNorm (its data gradient)
    w1 = (torch.randn(27, c, c, generator=g) * (1.0 / (c * 9)) ** 0.5).to(d)       # conv in front of it
    plan = ops.PackPlan([(w2, 27, c, c, 2, esz), (w1, 27, c, c, 2, esz)], d)
    plan.run()
    wp2, wp1 = plan.outputs
    xf = u.float()
    mean = xf.mean(0)
    invstd = 1.0 / torch.sqrt(xf.var(0, unbiased=False) + 1e-4)
    zero = torch.zeros(c, device=d)
    for with_add in (False, True):
        out = {}
        for fold in (True, False):
            old = ops.set_pre_rows(BIG if fold else 0, BIG if fold else 0)
            try:
                t_bn, t_prev = ops.stats_totals(c, d), ops.stats_totals(c, d)
                da = torch.full((n, c), float("nan"), dtype=dtype, device=d)
                du = torch.full((n, c), float("nan"), dtype=dtype, device=d)
                dx = torch.full((n, c), float("nan"), dtype=dtype, device=d)
                dg, db = torch.full((c,), float("nan"), device=d), torch.full((c,), float("nan"), device=d)
                lst = [dict(kind=ops.CX_GEMM, flags=ops.CX_F_RELU, rows=n, rows_in=n, c_in=c, c_out=c, K=27, tbl_ld=n, x_ld=c, y_ld=c,
                            x=dy, w=wp2, tbl=tbl, y=da, aux=u, aux_ld=c, mean=mean, invstd=invstd, gamma=gamma, beta=beta, stats=t_bn),
                       dict(kind=ops.CX_BNBWD, flags=ops.CX_F_RELU, rows=n, c_in=c, c_split=c, x_ld=c, y_ld=c, aux_ld=c, x=da, aux=u, y=du,
                            res=(add_full[:, c:] if with_add else None), res_ld=2 * c, stats=t_bn, mean=mean, invstd=invstd,
                            gamma=gamma, beta=beta, dgamma=dg, dbeta=db),
                       # the previous layer's data gradient (no BatchNorm in front of it here: plain statistics of the output)
                       dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=n, c_in=c, c_out=c, K=27, tbl_ld=n, x_ld=c, y_ld=c,
                            x=du, w=wp1, tbl=tbl, y=dx, stats=t_prev)]
                launches = ops.layers_run(lst, d, esz)
                torch.cuda.synchronize()
            finally:
                ops.set_pre_rows(*old)
            assert launches == (2 if fold else 3)
            out[fold] = (da, du, dx, dg, db)
        (da1, du1, dx1, dg1, db1), (da0, du0, dx0, dg0, db0) = out[True], out[False]
        it = torch.int16 if esz == 2 else torch.int32
        assert torch.equal(da1.view(it), da0.view(it))
        assert torch.equal(du1.view(it), du0.view(it)), with_add
        assert torch.equal(dg1, dg0) and torch.equal(db1, db0)
        assert _scale_err(dx1.float(), dx0.float()) < (2.0 ** -7 if esz == 2 else 1e-5)
        # autograd of relu(batch_norm(u)) under the upstream gradient da (as stored), fp64
        ud = u.double().requires_grad_(True)
        a = torch.relu(torch.nn.functional.batch_norm(ud, None, None, gamma.double(), beta.double(), True, 0.1, 1e-4))
        gd = gamma.double().requires_grad_(True)
        bd = beta.double().requires_grad_(True)
        a2 = torch.relu(torch.nn.functional.batch_norm(ud, None, None, gd, bd, True, 0.1, 1e-4))
        gu, gg, gb = torch.autograd.grad(a2, (ud, gd, bd), da1.double())
        ref_du = gu + (add_full[:, c:].double() if with_add else 0.0)
        assert _scale_err(du1.double(), ref_du) < (2.0 ** -6 if esz == 2 else 2e-4), with_add
        assert torch.allclose(dg1.double(), gg, rtol=2e-3, atol=2e-3 * float(gg.abs().max()))
        assert torch.allclose(db1.double(), gb, rtol=2e-3, atol=2e-3 * float(gb.abs().max()))
        # the data gradient in front: oracle on the stored du with mirrored, transposed weights = indice_conv_backward's dx
        wq = (w1.to(dtype).float() if esz == 2 else w1).cpu().double().reshape(3, 3, 3, c, c)
        ref_dx, _ = oracle.indice_conv_backward(torch.zeros(n, c, dtype=torch.float64), wq, du1.cpu().double(), pairs, pn, False, True)
        assert _scale_err(dx1.cpu().double(), torch.as_tensor(ref_dx)) < (2.0 ** -7 if esz == 2 else 1e-4)


def test_fold_accumulates_parameter_gradients_and_takes_strided_operands(native_lib):
    """DODA_CX_F_ACCUM through the folded kernel (second backward pass of tool/st.py:136-198) and a BatchNorm input that is the
    left half of a concatenation (row stride 2c: the strided conv's BatchNorm reads the level's skip features in place)."""
    from doda_amd import ops
    d = dev()
    n, c = 1900, 80
    idx, shape, batch = _level(n + 11, n)
    n = idx.shape[0]
    tbl = _tables(ops, idx, shape, batch, d)
    g = torch.Generator().manual_seed(77)
    cat = _bf(torch.randn(n, 2 * c, generator=g)).to(d)
    u = cat[:, :c]                                                                   # ld = 2c
    da = _bf(torch.randn(n, c, generator=g)).to(d)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(d), (torch.randn(c, generator=g) * 0.3).to(d)
    w1 = (torch.randn(27, c, c, generator=g) * (1.0 / (c * 9)) ** 0.5).to(d)
    wp1 = _pack(w1, 27, c, c, 2, d)
    uf = u.float()
    mean, invstd = uf.mean(0), 1.0 / torch.sqrt(uf.var(0, unbiased=False) + 1e-4)
    # totals of (sum dz, sum dz xhat) as a data-grad epilogue would have left them
    xh = (uf - mean) * invstd
    dz = da.float() * ((xh * gamma + beta) > 0)
    res = {}
    for fold in (True, False):
        old = ops.set_pre_rows(BIG if fold else 0, BIG if fold else 0)
        try:
            t = ops.stats_totals(c, d)
            t[0, 0, :, :4] = dz.double().sum(0).reshape(-1, 4)
            t[0, 1, :, :4] = (dz.double() * xh.double()).sum(0).reshape(-1, 4)
            du = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
            dx = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
            dg, db = torch.full((c,), 2.0, device=d), torch.full((c,), -1.0, device=d)
            lst = [dict(kind=ops.CX_BNBWD, flags=ops.CX_F_RELU | ops.CX_F_ACCUM, rows=n, c_in=c, c_split=c, x_ld=c, y_ld=c, aux_ld=2 * c,
                        x=da, aux=u, y=du, stats=t, mean=mean, invstd=invstd, gamma=gamma, beta=beta, dgamma=dg, dbeta=db),
                   dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=n, c_in=c, c_out=c, K=27, tbl_ld=n, x_ld=c, y_ld=c, x=du, w=wp1,
                        tbl=tbl, y=dx)]
            assert ops.layers_run(lst, d, 2) == (1 if fold else 2)
            torch.cuda.synchronize()
        finally:
            ops.set_pre_rows(*old)
        res[fold] = (du, dx, dg, db)
    assert torch.equal(res[True][0].view(torch.int16), res[False][0].view(torch.int16))
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])
    assert torch.allclose(res[True][2], 2.0 + (dz * xh).sum(0), rtol=1e-4, atol=1e-3)
    assert torch.allclose(res[True][3], -1.0 + dz.sum(0), rtol=1e-4, atol=1e-3)
    assert _scale_err(res[True][1].float(), res[False][1].float()) < 2.0 ** -7
    ref = 1.0 * (gamma * invstd) * (dz - dz.mean(0) - xh * (dz * xh).mean(0))
    assert _scale_err(res[True][0].float(), ref) < 2.0 ** -6


@pytest.mark.parametrize("n,c", LEVELS[1:])
def test_gemm_down_up_and_1x1_with_strided_operands(native_lib, oracle, n, c):
    """k2 s2 convolution (K = 8 tables, both directions) and the 1x1 skip convolution (identity table) with operands that are
    column slices of a wider matrix — the level's concatenation read and written in place (reference model/unet_block.py:89-93)."""
    from doda_amd import ops
    d = dev()
    idx, shape, batch = _level(7 * n, n)
    n = idx.shape[0]
    outids, child, par_off = ops.rulebook_down2(torch.from_numpy(idx).to(d), shape, batch)[:3]
    m = outids.shape[0]
    g = torch.Generator().manual_seed(n + 1)
    c2 = c + 16
    # strided conv fine -> coarse, reading x as the left half of a [n, 2c] matrix
    cat = _bf(torch.randn(n, 2 * c, generator=g)).to(d)
    w = (torch.randn(8, c, c2, generator=g) * (1.0 / (c * 4)) ** 0.5).to(d)
    wp = _pack(w, 8, c, c2, 0, d)
    y = torch.zeros((m, c2), dtype=torch.bfloat16, device=d)
    st = ops.stats_totals(c2, d)
    ops.layers_run([dict(kind=ops.CX_GEMM, flags=0, rows=m, rows_in=n, c_in=c, c_out=c2, K=8, tbl_ld=child.shape[1], x_ld=2 * c, y_ld=c2,
                         x=cat, w=wp, tbl=child, y=y, stats=st)], d)
    lay = ops.spconv_gather(cat[:, :c].contiguous(), w, child, m, 0, c2, packed=wp)
    assert _scale_err(y.float(), lay.float()) < 2.0 ** -7
    yd = y.double()
    assert torch.allclose(ops.totals_sums(st)[0], yd.sum(0), rtol=1e-5, atol=1e-4 * float(yd.abs().max()))
    # inverse conv coarse -> fine, writing the right half of a [n, 2c] matrix
    z = _bf(torch.randn(m, c2, generator=g)).to(d)
    wi = (torch.randn(8, c2, c, generator=g) * (1.0 / c2) ** 0.5).to(d)
    wpi = _pack(wi, 8, c2, c, 0, d)
    out = torch.zeros((n, 2 * c), dtype=torch.bfloat16, device=d)
    ops.layers_run([dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=m, c_in=c2, c_out=c, K=8, tbl_ld=par_off.shape[1], x_ld=c2, y_ld=2 * c,
                         x=z, w=wpi, tbl=par_off, y=out[:, c:], stats=None)], d)
    lay = ops.spconv_gather(z, wi, par_off, n, 0, c, packed=wpi)
    assert _scale_err(out[:, c:].float(), lay.float()) < 2.0 ** -7
    assert float(out[:, :c].abs().max()) == 0.0
    # 1x1 convolution over the concatenation, with a residual that is itself a column slice
    w1 = (torch.randn(1, 2 * c, c, generator=g) * (1.0 / (2 * c)) ** 0.5).to(d)
    wp1 = _pack(w1, 1, 2 * c, c, 0, d)
    s = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    ident = torch.arange(n, dtype=torch.int32, device=d).view(1, n)
    ops.layers_run([dict(kind=ops.CX_GEMM, flags=ops.CX_F_IDENTITY, rows=n, rows_in=n, c_in=2 * c, c_out=c, K=1, tbl_ld=n, x_ld=2 * c, y_ld=c,
                         res_ld=2 * c, x=cat, w=wp1, tbl=ident, y=s, res=out[:, c:], stats=None)], d)
    ref = cat.float() @ w1[0].to(torch.bfloat16).float() + out[:, c:].float()
    assert _scale_err(s.float(), ref) < 2.0 ** -7


@pytest.mark.parametrize("n,c", LEVELS[1:3])
def test_gemm_backward_epilogue_vs_definition(native_lib, oracle, n, c):
    """Data-gradient call: y = dy gathered through W[26-o]^T, stored UNMASKED; totals (sum dz, sum dz * xhat) of the values masked by
    the ReLU of the BatchNorm in front of the conv; also the 2c-channel output (several channel blocks)."""
    from doda_amd import ops
    d = dev()
    idx, shape, batch = _level(3 * n, n)
    n = idx.shape[0]
    pairs, pn = oracle.indice_pairs_subm(idx, batch, shape, 3)
    tbl = ops.rulebook_subm(torch.from_numpy(idx).to(d), shape, batch, 3)
    g = torch.Generator().manual_seed(n + 2)
    for cin, cout in ((c, c), (2 * c, c)):
        x_bn = _bf(torch.randn(n, cin, generator=g)).to(d)            # input of the BatchNorm in front of the conv
        mean = (0.1 * torch.randn(cin, generator=g)).to(d)
        invstd = (1.0 + 0.2 * torch.rand(cin, generator=g)).to(d)
        gamma = (1.0 + 0.1 * torch.randn(cin, generator=g)).to(d)
        beta = (0.1 * torch.randn(cin, generator=g)).to(d)
        dy = _bf(torch.randn(n, cout, generator=g)).to(d)
        w = (torch.randn(27, cin, cout, generator=g) * (1.0 / (cin * 9)) ** 0.5).to(d)
        wpb = _pack(w, 27, cout, cin, 2, d)                           # data-grad layout of a SubM conv
        dz = torch.zeros((n, cin), dtype=torch.bfloat16, device=d)
        st = ops.stats_totals(cin, d)
        ops.layers_run([dict(kind=ops.CX_GEMM, flags=ops.CX_F_RELU, rows=n, rows_in=n, c_in=cout, c_out=cin, K=27, tbl_ld=n, x_ld=cout, y_ld=cin,
                             aux_ld=cin, x=dy, w=wpb, tbl=tbl, y=dz, aux=x_bn, stats=st, mean=mean, invstd=invstd, gamma=gamma, beta=beta)], d)
        torch.cuda.synchronize()
        xn = torch.relu((x_bn.float() - mean) * invstd * gamma + beta)
        din, _ = oracle.indice_conv_backward(xn.cpu().numpy(), w.to(torch.bfloat16).float().cpu().numpy().reshape(3, 3, 3, cin, cout),
                                             dy.float().cpu().numpy(), pairs, pn, subm=True)
        assert _scale_err(dz.float(), torch.as_tensor(din).to(d)) < 2.0 ** -7, (cin, cout)
        xh = (x_bn.float() - mean) * invstd
        zf = dz.double() * ((xh * gamma + beta) > 0).double()
        sums = ops.totals_sums(st)
        assert torch.allclose(sums[0], zf.sum(0), rtol=1e-4, atol=1e-3 * float(zf.abs().max()))
        assert torch.allclose(sums[1], (zf * xh.double()).sum(0), rtol=1e-4, atol=1e-3 * float(zf.abs().max()))


@pytest.mark.parametrize("n,c", LEVELS[1:] + [(300007, 8), (150001, 16), (70001, 24)])
def test_batchnorm_ops_vs_torch(native_lib, n, c):
    """STATS -> BNFWD (training, incl. the two-segment form of a concatenation, running statistics) and BNBWD (with the added skip
    gradient and the split output) as launches of their own against torch.nn.functional.batch_norm + autograd in fp32."""
    from doda_amd import ops
    import torch.nn.functional as F
    d = dev()
    g = torch.Generator().manual_seed(n + 3)
    C2 = 2 * c
    x = _bf(torch.randn(n, C2, generator=g) * 1.5 + 0.3).to(d)
    gamma = (1.0 + 0.1 * torch.randn(C2, generator=g)).to(d)
    beta = (0.1 * torch.randn(C2, generator=g)).to(d)
    rm, rv = torch.zeros(C2, device=d), torch.ones(C2, device=d)
    nbt = torch.zeros((), dtype=torch.int64, device=d)
    sa, sb = ops.stats_totals(c, d), ops.stats_totals(c, d)
    mean, invstd = torch.zeros(C2, device=d), torch.zeros(C2, device=d)
    y = torch.zeros((n, C2), dtype=torch.bfloat16, device=d)
    assert ops.layers_run([
        dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=c, x_ld=C2, x=x, stats=sa),
        dict(kind=ops.CX_STATS, flags=0, rows=n, c_in=c, x_ld=C2, x=x[:, c:], stats=sb),
        dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU | ops.CX_F_TRAINING, rows=n, c_in=C2, x_ld=C2, y_ld=C2, c_split=c, eps=1e-4, momentum=0.1,
             x=x, y=y, stats=sa, stats_b=sb, gamma=gamma, beta=beta, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, nbt=nbt),
    ], d) == 3
    xf = x.float().requires_grad_(True)
    rm_ref, rv_ref = torch.zeros(C2, device=d), torch.ones(C2, device=d)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = torch.relu(F.batch_norm(xf, rm_ref, rv_ref, gr, br, True, 0.1, 1e-4))
    torch.cuda.synchronize()
    assert _scale_err(y.float(), y_ref.detach()) < 2.0 ** -7
    assert torch.allclose(rm, rm_ref, rtol=1e-4, atol=1e-5) and torch.allclose(rv, rv_ref, rtol=1e-4, atol=1e-5)
    assert int(nbt) == 1
    assert torch.allclose(mean, xf.detach().mean(0), rtol=1e-4, atol=1e-5)
    # the same op writing a column slice of a wider matrix (ABI 12: the fine levels take this form too — lay_bn's strided sweep,
    # where the dense form of many rows goes to bn.hip's kernels)
    wide = torch.full((n, C2 + 16), 9.0, dtype=torch.bfloat16, device=d)
    m2, i2 = torch.zeros(C2, device=d), torch.zeros(C2, device=d)
    ops.layers_run([dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU | ops.CX_F_TRAINING, rows=n, c_in=C2, x_ld=C2, y_ld=C2 + 16, c_split=c, eps=1e-4,
                         momentum=0.1, x=x, y=wide[:, 16:], stats=sa, stats_b=sb, gamma=gamma, beta=beta, mean=m2, invstd=i2,
                         running_mean=torch.zeros(C2, device=d), running_var=torch.ones(C2, device=d))], d)
    torch.cuda.synchronize()
    assert _scale_err(wide[:, 16:].float(), y_ref.detach()) < 2.0 ** -7 and bool((wide[:, :16] == 9.0).all())
    assert torch.equal(m2, mean) and torch.equal(i2, invstd)
    # backward: the unmasked gradient as the data-grad GEMM stores it, the totals of its masked values as that GEMM's epilogue leaves them
    dy = _bf(torch.randn(n, C2, generator=g)).to(d)
    add = _bf(torch.randn(n, C2, generator=g)).to(d)
    (y_ref * dy.float()).sum().backward()
    xh = (x.float() - mean) * invstd
    dz = dy.float() * ((xh * gamma + beta) > 0).float()
    st = ops.stats_totals(C2, d)
    st[0, 0, :, :4] = dz.double().sum(0).reshape(-1, 4)
    st[0, 1, :, :4] = (dz.double() * xh.double()).sum(0).reshape(-1, 4)
    dxa = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    dxb = torch.zeros((n, c), dtype=torch.bfloat16, device=d)
    dg, db = torch.zeros(C2, device=d), torch.zeros(C2, device=d)
    ops.layers_run([dict(kind=ops.CX_BNBWD, flags=ops.CX_F_RELU, rows=n, c_in=C2, x_ld=C2, aux_ld=C2, res_ld=C2, y_ld=c, y2_ld=c, c_split=c,
                         x=dy, aux=x, res=add, y=dxa, y2=dxb, stats=st, mean=mean, invstd=invstd, gamma=gamma, beta=beta, dgamma=dg, dbeta=db)], d)
    torch.cuda.synchronize()
    ref = xf.grad + add.float()
    got = torch.cat((dxa, dxb), 1).float()
    assert _scale_err(got, ref) < 2.0 ** -6
    assert torch.allclose(dg, gr.grad, rtol=2e-2, atol=2e-2 * float(gr.grad.abs().max()))
    assert torch.allclose(db, br.grad, rtol=2e-2, atol=2e-2 * float(br.grad.abs().max()))
    # evaluation mode: running statistics
    ye = torch.zeros((n, C2), dtype=torch.bfloat16, device=d)
    ops.layers_run([dict(kind=ops.CX_BNFWD, flags=ops.CX_F_RELU, rows=n, c_in=C2, x_ld=C2, y_ld=C2, c_split=C2, eps=1e-4, momentum=0.1,
                         x=x, y=ye, gamma=gamma, beta=beta, running_mean=rm, running_var=rv)], d)
    ye_ref = torch.relu(F.batch_norm(x.float(), rm, rv, gamma, beta, False, 0.1, 1e-4))
    assert _scale_err(ye.float(), ye_ref) < 2.0 ** -7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("level,n", [(4, 8400), (5, 1900), (5, 700), (6, 420), (7, 83)])
def test_subtree_layers_vs_module_path(native_lib, level, n, dtype):
    """UBlock(level) forward + backward as ONE extension call over the per-layer backend against the same modules run one by
    one (autograd node per op) — same kernels up to the tile shapes, so fp32 agrees to 1e-4 of scale and bf16 sits as close to the
    fp32 run as the module path does."""
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    net, ub, ind, shape, batch = _subtree(level, n, 23)
    g = torch.Generator().manual_seed(level * 100 + n)
    c = 16 * level
    x0 = _bf(torch.randn(ind.shape[0], c, generator=g)).to(dev())
    gout = _bf(torch.randn(ind.shape[0], c, generator=g)).to(dev())
    state = {k: v.clone() for k, v in ub.state_dict().items()}
    yf, dxf, gf, bf_ = _run_subtree(ub, ind, shape, batch, level, x0.float(), gout.float(), "off")
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp(min=1e-20))
    if dtype == torch.float32:
        ub.load_state_dict(state)
        y1, dx1, g1, b1 = _run_subtree(ub, ind, shape, batch, level, x0.float(), gout.float(), "layers")
        fwd, bwd = ext.coarse_launches()
        assert fwd > 0 and bwd > 0
        # (gradients: the two paths derive a small level's BatchNorm statistics differently — fp64 totals here, a shifted two-pass
        # sweep there —, mean / invstd differ in their last bits and a handful of ReLU masks at |pre-activation| ~ 1e-7 flip: each
        # flip moves one element of a gradient by O(1).  The folded-vs-unfolded test below, where the masks agree, is the tight one.)
        assert rel(y1, yf) < 1e-4 and rel(dx1, dxf) < 2e-2, (rel(y1, yf), rel(dx1, dxf))
        for k in gf:
            assert rel(g1[k], gf[k]) < 3e-2, (k, rel(g1[k], gf[k]))
        for k in bf_:
            if k.endswith("num_batches_tracked"):
                assert int(b1[k]) == int(bf_[k]) == 1
            else:
                assert torch.allclose(b1[k], bf_[k], rtol=1e-4, atol=1e-5), k
        return
    ub.load_state_dict(state)
    y0, dx0, g0, b0 = _run_subtree(ub, ind, shape, batch, level, x0, gout, "off")
    ub.load_state_dict(state)
    y1, dx1, g1, b1 = _run_subtree(ub, ind, shape, batch, level, x0, gout, "layers")

    def same_distance(name, e, l, f):
        e_l, l_f, e_f = rel(e, l), rel(l, f), rel(e, f)
        assert e_f < 1.5 * l_f + 2e-2, (name, e_f, l_f)
        assert e_l < 1.5 * l_f + 2e-2, (name, e_l, l_f)

    same_distance("y", y1, y0, yf)
    assert rel(y1, yf) < 2e-2
    same_distance("dx", dx1, dx0, dxf)
    for k in g0:
        same_distance(k, g1[k], g0[k], gf[k])
        assert float(g1[k].abs().max()) > 0, k
    for k in b0:
        if k.endswith("num_batches_tracked"):
            assert int(b0[k]) == int(b1[k]) == 1, k
        else:
            assert torch.allclose(b1[k], b0[k], rtol=1e-2, atol=1e-3), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_subtree_folded_equals_unfolded_and_launch_counts(native_lib, dtype):
    """The same subtree with the folding switched off: every BatchNorm then runs as its own launch.  Forward outputs agree to the
    summation order of the convs; the launch counts are those of DESIGN.md (per residual block 2 instead of 4 forward, 3 instead
    of 4 backward)."""
    from doda_amd import ops
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    level, n = 5, 1900
    net, ub, ind, shape, batch = _subtree(level, n, 29)
    g = torch.Generator().manual_seed(5)
    c = 16 * level
    x0 = _bf(torch.randn(ind.shape[0], c, generator=g)).to(dev())
    gout = _bf(torch.randn(ind.shape[0], c, generator=g)).to(dev())
    state = {k: v.clone() for k, v in ub.state_dict().items()}
    res, counts = {}, {}
    for fold in (True, False):
        ub.load_state_dict(state)
        old = ops.set_pre_rows(BIG if fold else 0, BIG if fold else 0)
        try:
            res[fold] = _run_subtree(ub, ind, shape, batch, level, x0.to(dtype), gout.to(dtype), "layers")
        finally:
            ops.set_pre_rows(*old)
        counts[fold] = ext.coarse_launches()
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp(min=1e-20))
    if dtype == torch.float32:   # same statistics, same masks: only the convs' summation order over offsets differs
        assert rel(res[True][0], res[False][0]) < 1e-5 and rel(res[True][1], res[False][1]) < 2e-3, (rel(res[True][0], res[False][0]), rel(res[True][1], res[False][1]))
        for k in res[True][2]:
            assert rel(res[True][2][k], res[False][2][k]) < 5e-3, k
    else:
        assert rel(res[True][0], res[False][0]) < 2e-2 and rel(res[True][1], res[False][1]) < 0.3
    # levels 5-7: 10 residual blocks (two with a 1x1 skip conv), 2 strided + 2 inverse convs; one statistics op for the input
    n_rb, n_skip, n_updown = 10, 2, 4
    assert counts[False][0] == 1 + 4 * n_rb + n_skip + 2 * n_updown, counts
    assert counts[True][0] == 1 + 2 * n_rb + n_skip + n_updown, counts
    assert counts[False][1] == 4 * n_rb + n_skip + 2 * n_updown, counts
    # backward: every BNBWD folds but the two with two outputs (the concatenations' gradients) and the last (nothing follows it)
    assert counts[True][1] == counts[False][1] - (2 * n_rb + n_updown - 3), counts


@pytest.mark.parametrize("level", [4, 2, 1])
def test_unet_step_layers_vs_module_path_and_fp32(native_lib, level):
    """The whole training step with levels `level`-7 as one extension call (1 = the whole U-Net, the default: tile kernels over
    tilebooks, the weights-in-LDS kernel and the k2 s2 kernels inside the op list, every concatenation written in place) against
    the module-by-module step and fp32."""
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    sf, lf, gf, _ = _unet_step("off", 4, dtype=torch.float32)
    sl, ll, gl, _ = _unet_step("layers", level, dtype=torch.float32)
    assert ext.coarse_launches()[0] > (60 if level == 1 else 20), ext.coarse_launches()   # (the op list did run)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp(min=1e-20))
    assert abs(ll - lf) / lf < 1e-5, (ll, lf)
    assert _scale_err(sl, sf) < 1e-4
    for k in gf:
        assert rel(gl[k], gf[k]) < 1e-2, (k, rel(gl[k], gf[k]))
    s0, l0, g0, b0 = _unet_step("off", 4)
    s1, l1, g1, b1 = _unet_step("layers", level)
    assert abs(l1 - l0) / abs(l0) < 2e-3 and abs(l1 - lf) / lf < 2e-2, (lf, l0, l1)
    assert _scale_err(s1, s0) < 3e-2
    for k in g0:
        e_mod, e_lay = rel(g0[k], gf[k]), rel(g1[k], gf[k])
        assert e_lay < 1.3 * e_mod + 0.05, (k, e_lay, e_mod)
    for k in b0:
        if k.endswith("num_batches_tracked"):
            assert int(b0[k]) == int(b1[k]) == 1, k
        else:
            assert torch.allclose(b1[k], b0[k], rtol=5e-2, atol=5e-3), k


@pytest.mark.parametrize("level", [4, 1])
def test_unet_layers_two_backward_passes_accumulate(native_lib, level):
    """Two forward / backward passes into the same .grad tensors (tool/st.py:136-198)."""
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    _, _, g1, _ = _unet_step("layers", level, voxels=30000)
    _, _, g2, _ = _unet_step("layers", level, voxels=30000, two_pass=True)
    for k in g1:
        if k.startswith("unet.u.u.u." if level == 4 else "unet."):
            assert torch.allclose(g2[k], 2.0 * g1[k], rtol=2e-2, atol=2e-2 * float(g1[k].abs().max())), k


@pytest.mark.parametrize("level", [4, 1])
def test_unet_layers_eval_and_no_grad(native_lib, level):
    """Evaluation mode (running statistics folded into the gathers) and torch.no_grad() in training mode."""
    from doda_amd import model as M
    from doda_amd.model import SparseConvNet, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from tests.util import deterministic_init
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    d = dev()
    cfg = default_cfg()
    batch = make_batch(2, 40000, 5)
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in batch.items()}
    net = deterministic_init(SparseConvNet(cfg), seed=4).to(d)
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
    out = {}
    try:
        for mode in ("eval", "train"):
            net.train(mode == "train")
            for cm in ("off", "layers"):
                M.set_coarse_mode(cm, level)
                state = {k: v.clone() for k, v in net.state_dict().items()}
                for dt in (torch.bfloat16, torch.float32):
                    with torch.no_grad():
                        out[(mode, cm, dt)] = voxelize_and_run(cfg, net, bd, d, feature_dtype=dt).float()
                    net.load_state_dict(state)
    finally:
        M.set_coarse_mode(*old)
    torch.cuda.synchronize()
    for mode in ("eval", "train"):
        assert _scale_err(out[(mode, "layers", torch.bfloat16)], out[(mode, "off", torch.bfloat16)]) < 3e-2, mode
        assert _scale_err(out[(mode, "layers", torch.float32)], out[(mode, "off", torch.float32)]) < 2e-4, mode


def test_backend_selection():
    """choose_coarse_backend: one extension call over the per-layer launches, or module by module (no GPU work)."""
    from doda_amd import model as M
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
    try:
        M.set_coarse_mode("layers")
        assert M.choose_coarse_backend(8400, torch.bfloat16) == "layers" and M.choose_coarse_backend(8400, torch.float32) == "layers"
        assert M.choose_coarse_backend(1, torch.bfloat16) is None and M.choose_coarse_backend(8400, torch.float16) is None
        M.set_coarse_mode("off")
        assert M.choose_coarse_backend(2000, torch.bfloat16) is None
    finally:
        M.set_coarse_mode(*old)


def test_unet_layers_yield_to_hooks_and_frozen_parameters(native_lib, monkeypatch):
    """The one-call subtree must step aside for a forward hook registered on any of its modules (the hook has to fire) and for a
    frozen parameter (no gradient may be deposited): both fall back to the module-by-module path, per call — the plan is cached.
    A submodule replaced after the plan was made is the one the next one-call step runs and trains."""
    from doda_amd import model as M
    from doda_amd.model import SparseConvNet, cross_entropy, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    from doda_amd.spconv import functional as Fsp
    from tests.util import deterministic_init
    from doda_amd._ext import ext
    if ext is None or not hasattr(ext, "coarse_ublock"):
        pytest.skip("compiled extension not built")
    d = dev()
    cfg = default_cfg()
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in make_batch(2, 30000, 9).items()}
    net = deterministic_init(SparseConvNet(cfg), seed=5).to(d).train()
    old = (M.COARSE_MODE, M.COARSE_EXEC_LEVEL)
    M.set_coarse_mode("layers", 1)
    try:
        assert Fsp.set_deferred_wgrad(True)

        def step():
            net.zero_grad(set_to_none=True)
            cross_entropy(voxelize_and_run(cfg, net, bd, d, feature_dtype=torch.bfloat16), bd["labels"]).backward()
            torch.cuda.synchronize()

        one_call = []                                       # what _forward_coarse returned, call by call
        coarse = M.UBlock._forward_coarse
        monkeypatch.setattr(M.UBlock, "_forward_coarse", lambda ub, inp: one_call.append(coarse(ub, inp)) or one_call[-1])
        step()                                              # plan made, one call
        assert one_call[-1] is not None
        old_bn = net.unet.u.blocks.block0.conv_branch[0]
        new_bn = torch.nn.BatchNorm1d(old_bn.num_features, eps=1e-4, momentum=0.1).to(d)
        new_bn.weight.data.fill_(2.0)
        setattr(net.unet.u.blocks.block0.conv_branch, "0", new_bn)
        old_bn.weight.grad = old_bn.bias.grad = None         # (no longer the net's: step() does not clear them)
        step()
        assert one_call[-1] is not None                     # still one call, over the new module
        assert new_bn.weight.grad is not None and float(new_bn.weight.grad.abs().sum()) > 0
        assert int(new_bn.num_batches_tracked) == 1 and int(old_bn.num_batches_tracked) == 1
        assert old_bn.weight.grad is None and old_bn.bias.grad is None
        seen = []
        deep = net.unet.u.u.blocks.block0
        h = deep.register_forward_hook(lambda m, i, o: seen.append(o.features.shape[0]))
        step()
        assert len(seen) == 1, seen                         # the hook fired: the subtree ran module by module
        h.remove()
        w = net.unet.u.blocks.block1.conv_branch[2].weight
        w.requires_grad_(False)
        step()
        assert w.grad is None                               # nothing deposited into the frozen weight
        w.requires_grad_(True)
        step()
        assert w.grad is not None and float(w.grad.abs().sum()) > 0
    finally:
        Fsp.set_deferred_wgrad(False)
        M.set_coarse_mode(*old)


@pytest.mark.parametrize("kernel", ["conv_tile16", "conv_tile", "conv_tile_dual", "conv_wlds48", "conv_up32"])
@pytest.mark.parametrize("form", ["forward", "data_grad"])
def test_lds_staged_kernels_take_strided_output_operands(native_lib, kernel, form):
    """ABI 12: the LDS-staged kernels write y, read the residual and read the BatchNorm input of the data-gradient statistics through
    row strides (the halves of a level's concatenation, in place: reference model/unet_block.py:89-93).  Every kernel, forward form
    (residual + statistics of y) and data-gradient form (ReLU mask and statistics against a BatchNorm input): the strided call must
    give the dense call's bits in the slice, the same totals, and must not touch the other columns of the wide matrices."""
    from doda_amd import ops
    d = dev()
    spec = {"conv_tile16": (27, 16, 16, 200000), "conv_tile": (27, 16, 16, 60000), "conv_tile_dual": (27, 32, 32, 60000),
            "conv_wlds48": (27, 48, 48, 20000), "conv_up32": (8, 32, 16, 60000)}[kernel]
    K, cin, cout, n_req = spec
    idx, shape, batch = _level(1234 + n_req + cin, n_req)
    n = idx.shape[0]
    g = torch.Generator().manual_seed(n + cout)
    tb = None
    if K == 27:
        tbl = _tables(ops, idx, shape, batch, d)
        tbl = tbl[0] if isinstance(tbl, (tuple, list)) else tbl
        rows_in = n
        if kernel != "conv_wlds48":
            tb = ops.tilebook_build(tbl)
            assert tb is not None
    else:
        outids, child, par_off = ops.rulebook_down2(torch.from_numpy(idx).to(d), shape, batch)[:3]
        tbl, rows_in = par_off, outids.shape[0]          # coarse -> fine: one source row per output row
        assert rows_in < n
    assert tbl.shape == (K, n)
    x = _bf(torch.randn(rows_in, cin, generator=g)).to(d)
    w = (torch.randn(K, cin, cout, generator=g) * (1.0 / (cin * 6)) ** 0.5).to(d)
    wp = _pack(w, K, cin, cout, 0, d)
    wide = 2 * cout + 16
    res_d = _bf(torch.randn(n, cout, generator=g)).to(d)
    aux_d = _bf(torch.randn(n, cout, generator=g)).to(d)
    mean, invstd = torch.randn(cout, generator=g).to(d) * 0.1, (torch.rand(cout, generator=g) + 0.5).to(d)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5).to(d), torch.randn(cout, generator=g).to(d) * 0.2

    def run(strided):
        if strided:
            ybuf = torch.full((n, wide), 7.0, dtype=torch.bfloat16, device=d)
            rbuf = torch.full((n, wide), -3.0, dtype=torch.bfloat16, device=d)
            abuf = torch.full((n, wide), 5.0, dtype=torch.bfloat16, device=d)
            y, res, aux = ybuf[:, cout:2 * cout], rbuf[:, 16:16 + cout], abuf[:, wide - cout:]
            res.copy_(res_d); aux.copy_(aux_d)
        else:
            ybuf = torch.zeros((n, cout), dtype=torch.bfloat16, device=d)
            y, res, aux, rbuf, abuf = ybuf, res_d, aux_d, None, None
        st = ops.stats_totals(cout, d)
        op = dict(kind=ops.CX_GEMM, flags=0, rows=n, rows_in=rows_in, c_in=cin, c_out=cout, K=K, tbl_ld=tbl.shape[1], x_ld=cin,
                  y_ld=ybuf.shape[1], x=x, w=wp, tbl=tbl, y=y, stats=st)
        if tb is not None:
            op["tilebook"] = tb.data_ptr()
        if form == "forward":
            op.update(res=res, res_ld=res.stride(0))
        else:
            op.update(flags=ops.CX_F_RELU, aux=aux, aux_ld=aux.stride(0), mean=mean, invstd=invstd, gamma=gamma, beta=beta)
        assert ops.layers_run([op], d) == 1
        torch.cuda.synchronize()
        return y.clone(), ops.totals_sums(st).clone(), ybuf, rbuf, abuf

    y0, s0, _, _, _ = run(False)
    y1, s1, ybuf, rbuf, abuf = run(True)
    assert float(y0.float().abs().max()) > 0.1
    assert torch.equal(y0, y1)
    assert torch.allclose(s0, s1, rtol=1e-12, atol=1e-9)
    assert float(s0.abs().max()) > 0
    keep = torch.ones(wide, dtype=torch.bool, device=d)
    keep[cout:2 * cout] = False
    assert bool((ybuf[:, keep] == 7.0).all())
    assert bool((rbuf[:, :16] == -3.0).all()) and bool((rbuf[:, 16 + cout:] == -3.0).all())
    assert bool((abuf[:, :wide - cout] == 5.0).all())
    # and the dense call is the module path's kernel: against ops.spconv_gather on the same operands
    ref = ops.spconv_gather(x, w, tbl, n, 0, cout, packed=wp, tilebook=tb, residual=res_d if form == "forward" else None)
    ref = ref[0] if isinstance(ref, (tuple, list)) else ref
    assert torch.equal(ref, y0)

"""GPU tests of the tilebook (doda_tilebook_build) and the LDS-staged convolution kernel (conv_tile).

* the tilebook is a lossless re-encoding of the dense gather table: per tile the sorted distinct rows and
  per entry 1 + its position (0 = absent), so  ulist[tile][lidx[tile][o][pos(r)] - 1] == tbl[o][tile*T + r];
* the tile kernel against the CPU oracle's indice_conv on the SAME bf16-rounded operands (products exact in
  fp32, only the summation order differs: 1e-4 relative as north_star states) and against the dense-table
  kernel (fp32 outputs to 1e-5, bf16 outputs within one rounding step);
* every epilogue option (residual, fp32 output, BatchNorm statistics forward and backward form);
* a table whose tiles reference more than the staged capacity falls back to the dense table inside the
  kernel; ragged last tile, NB = 2 (16 -> 32, the data-grad of a 32 -> 16 layer);
* the whole U-Net training step with and without tilebooks.
"""
import numpy as np
import pytest
import torch

from tests.util import deterministic_init, surface_voxels

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _ext_or_skip():
    from doda_amd._ext import ext
    if ext is None:
        pytest.skip("compiled extension not built")
    return ext


def _scene_table(m, seed=0, batch=2, shape=(80, 70, 60)):
    from doda_amd import ops
    d = dev()
    idx = torch.from_numpy(surface_voxels(seed, m, batch, list(shape))).to(d)
    # raster order (the order real scans and the synthetic scenes arrive in): neighbours of a tile overlap
    key = ((idx[:, 0].long() * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
    idx = idx[torch.argsort(key)].contiguous()
    return idx, ops.rulebook_subm(idx, list(shape), batch, 3)


def _far_apart_table(n=400000, second_div=1):
    """Every tile references two clusters of rows 200 000 rows apart (modulo n = 400 000, so from either side) — a span above the
    196 608 bits of the builder's bitmap (tilebook.hpp TB_BITMAP_BITS): the hash + sort form, for EVERY tile (asserted; with
    300 000 rows the second cluster of two tiles in three wrapped around to 100 000 rows from the first, and those tiles took the
    bitmap form) —, up to ~540 distinct rows per tile; some entries absent."""
    t = torch.arange(n, dtype=torch.int64)
    t0 = t // 256 * 256
    tbl = torch.empty(27, n, dtype=torch.int64)
    for o in range(27):
        # (second_div = 2: the second cluster of a tile has half as many rows, ~410 distinct rows per tile)
        tbl[o] = (t + o) % n if o < 13 else (t0 + (t - t0) // second_div + 200000 + o) % n
    g = torch.Generator().manual_seed(3)
    tbl[torch.rand(27, n, generator=g) < 0.3] = -1
    tbl[13] = t   # the centre tap is always present
    nt = -(-n // 256)
    ent = torch.full((27, nt * 256), -1, dtype=torch.int64)
    ent[:, :n] = tbl
    ent = ent.view(27, nt, 256)
    span = ent.amax((0, 2)) - torch.where(ent >= 0, ent, torch.full_like(ent, n)).amin((0, 2)) + 1
    assert int(span.min()) > _bitmap_bits(), int(span.min())      # every tile takes the hash + sort form
    return tbl.int().to(dev())


def _bitmap_bits():
    """tilebook.hpp TB_BITMAP_BITS as tools/gathernumerics.py restates it (tests/test_gather_plan_host.py holds the two together)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gathernumerics", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "tools", "gathernumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TB_BITMAP_BITS


@pytest.mark.parametrize("m", [40000, 1000, 256, 255, -1, -2])
def test_tilebook_is_a_lossless_encoding(native_lib, m):
    """m > 0: scene tables (rows of a tile within a few thousand row numbers: the builder's bitmap form); m = -1: a table
    whose tiles reference two far-apart clusters (the hash + bitonic-sort form).  Same format, same checks."""
    ext = _ext_or_skip()
    tbl = _far_apart_table(second_div=2 if m == -2 else 1) if m < 0 else _scene_table(m, seed=m)[1]
    n = tbl.shape[1]
    t = ext.with_tilebook(tbl)
    assert ext.has_tilebook(t) and torch.equal(t, tbl)
    ulist, lidx, ucount = (v.cpu().numpy() for v in ext.tilebook_parts(t))
    lidx = lidx.view(np.uint16)
    T, UMAX = lidx.shape[2], ulist.shape[1]
    tb = tbl.cpu().numpy()
    for tile in range(ulist.shape[0]):
        rows = np.arange(tile * T, min((tile + 1) * T, n))
        ent = np.full((27, T), -1, np.int64)
        ent[:, :len(rows)] = tb[:, rows]
        uniq = np.unique(ent[ent >= 0])
        assert ucount[tile] == len(uniq) <= UMAX - 1     # (10-bit local indices: at most 1023 distinct rows keep a list)
        assert np.array_equal(ulist[tile, :len(uniq)], uniq) and (ulist[tile, len(uniq):] == -1).all()
        loc = lidx[tile].astype(np.int64)                  # decoded [27, T]; 0 = absent, else 1 + position
        absent = loc == 0
        assert np.array_equal(absent, ent < 0)
        assert loc.max() <= len(uniq)
        back = np.where(absent, -1, ulist[tile][np.maximum(loc - 1, 0)])
        assert np.array_equal(back, ent)


def test_tilebook_hash_form_is_the_same_every_time(native_lib):
    """Round 5 regression: the hash + bitonic-sort form of the builder (tiles whose rows span more than its bitmap covers) used to
    leave out workgroup barriers between sort stages that stay inside one wave's chunk; about once in 50 000 tiles a list came out
    with one key twice and its neighbour missing (wrong local indices, garbage rows in the conv: the rare wrong steps of 1 cm
    batches in Z-order numbering).  A table whose 1172 tiles ALL take that form, built 400 times: every build must
    equal the first byte for byte, and the first is checked by test_tilebook_is_a_lossless_encoding."""
    from doda_amd import ops
    for div in (2, 1):          # ~410 distinct rows per tile (a 512-key sort: where the race was seen) and ~570 (1024 keys)
        tbl = _far_apart_table(second_div=div)
        ref = ops.tilebook_build(tbl)
        torch.cuda.synchronize()
        ref = ref.clone()
        bad = 0
        for _ in range(400):
            bad += int(not torch.equal(ops.tilebook_build(tbl), ref))
        assert bad == 0, "%d of 400 builds differ (second_div %d)" % (bad, div)


def _oracle_conv(x, w, tbl, layout):
    """fp64 reference over the dense table (definition in include/doda_hip.h)."""
    xd, wd = x.double().cpu(), w.double().cpu()
    t = tbl.cpu().long()
    K = t.shape[0]
    y = torch.zeros(t.shape[1], w.shape[2] if layout == 0 else w.shape[1], dtype=torch.float64)
    for o in range(K):
        b = wd[o] if layout == 0 else wd[K - 1 - o].t()
        sel = t[o] >= 0
        y[sel] += xd[t[o][sel]] @ b
    return y


@pytest.mark.parametrize("m,kc,nc,layout", [(40000, 16, 16, 0), (40000, 16, 16, 2), (9000, 16, 32, 2), (777, 16, 16, 0),
                                            (40000, 16, 48, 0), (40000, 32, 32, 0), (40000, 32, 32, 2), (9000, 32, 16, 2),
                                            (5000, 32, 48, 0), (300, 32, 32, 0)])
def test_tile_kernel_matches_oracle_and_dense_kernel(native_lib, m, kc, nc, layout):
    from doda_amd import ops
    d = dev()
    _, tbl = _scene_table(m, seed=3 + m)
    n = tbl.shape[1]
    torch.manual_seed(m + nc + kc)
    x = torch.randn(n, kc, device=d).bfloat16()
    w = (torch.randn(27, kc, nc, device=d) * 0.1).bfloat16().float()   # bf16-representable: products exact
    wk = w if layout == 0 else w.transpose(1, 2).contiguous()            # [K][nc][kc] for layout 2
    tb = ops.tilebook_build(tbl)
    assert tb is not None
    ref = _oracle_conv(x, wk, tbl, layout)
    y32_tile = ops.spconv_gather(x, wk, tbl, n, layout, nc, out_f32=True, tilebook=tb)
    y32_dense = ops.spconv_gather(x, wk, tbl, n, layout, nc, out_f32=True)
    assert rel_err(y32_tile.cpu(), ref) < 1e-4
    assert rel_err(y32_tile.cpu(), y32_dense.cpu()) < 1e-5
    y_tile = ops.spconv_gather(x, wk, tbl, n, layout, nc, tilebook=tb)
    y_dense = ops.spconv_gather(x, wk, tbl, n, layout, nc)
    assert y_tile.dtype == torch.bfloat16
    # one bf16 rounding of nearly equal fp32 sums: at most one step apart, almost always equal
    diff = (y_tile.float() - y_dense.float()).abs()
    assert (diff <= 2.0 ** -7 * y_dense.float().abs() + 1e-6).all()
    assert (y_tile != y_dense).float().mean().item() < 0.02
    res = torch.randn(n, nc, device=d).bfloat16()
    y_res = ops.spconv_gather(x, wk, tbl, n, layout, nc, residual=res, tilebook=tb)
    assert rel_err(y_res.float().cpu(), ref + res.double().cpu()) < 2.0 ** -7


def _oracle_wgrad(x, dy, tbl):
    xd, gd = x.double().cpu(), dy.double().cpu()
    t = tbl.cpu().long()
    dw = torch.zeros(t.shape[0], x.shape[1], dy.shape[1], dtype=torch.float64)
    for o in range(t.shape[0]):
        sel = t[o] >= 0
        dw[o] = xd[t[o][sel]].t() @ gd[sel]
    return dw


@pytest.mark.parametrize("m,nc,layout", [(40000, 16, 0), (40000, 16, 2), (9000, 32, 2), (300, 48, 0)])
def test_tile_kernel_fp32_features(native_lib, m, nc, layout):
    """fp32 features (the reference's precision), 16 input channels: 64-byte rows through the same staging; 1e-4
    against the fp64 oracle as north_star states, 1e-5 against the dense-table fp32 kernel; residual add."""
    from doda_amd import ops
    d = dev()
    _, tbl = _scene_table(m, seed=21 + m)
    n = tbl.shape[1]
    torch.manual_seed(m + nc)
    x = torch.randn(n, 16, device=d)
    w = torch.randn(27, 16, nc, device=d) * 0.1
    wk = w if layout == 0 else w.transpose(1, 2).contiguous()
    tb = ops.tilebook_build(tbl)
    ref = _oracle_conv(x, wk, tbl, layout)
    y_tile = ops.spconv_gather(x, wk, tbl, n, layout, nc, tilebook=tb)
    y_dense = ops.spconv_gather(x, wk, tbl, n, layout, nc)
    assert y_tile.dtype == torch.float32
    assert rel_err(y_tile.cpu(), ref) < 1e-4
    assert rel_err(y_tile.cpu(), y_dense.cpu()) < 1e-5
    res = torch.randn(n, nc, device=d)
    y_res = ops.spconv_gather(x, wk, tbl, n, layout, nc, residual=res, tilebook=tb)
    assert rel_err(y_res.cpu(), ref + res.double().cpu()) < 1e-4


def test_tile_kernel_overflow_tiles_fall_back(native_lib):
    """Random neighbours: every tile references far more than the staged capacity."""
    ext = _ext_or_skip()
    from doda_amd import ops
    d = dev()
    n = 3000
    g = torch.Generator().manual_seed(5)
    tbl = torch.randint(0, n, (27, n), generator=g, dtype=torch.int32)
    tbl[torch.rand(27, n, generator=g) < 0.5] = -1
    tbl = tbl.to(d)
    t = ext.with_tilebook(tbl)
    ulist, _, ucount = ext.tilebook_parts(t)
    assert (ucount > ulist.shape[1]).all()
    tb = ops.tilebook_build(tbl)
    for kc in (16, 32):
        x = torch.randn(n, kc, device=d).bfloat16()
        w = (torch.randn(27, kc, 16, device=d) * 0.1).bfloat16().float()
        y = ops.spconv_gather(x, w, tbl, n, 0, 16, out_f32=True, tilebook=tb)
        assert rel_err(y.cpu(), _oracle_conv(x, w, tbl, 0)) < 1e-4


def test_tile_kernel_statistics_epilogue(native_lib):
    """The conv node of the extension on a table that carries its tilebook: output, statistics rows
    (forward) and the fused BatchNorm backward (data-grad statistics) equal the dense-table kernels."""
    ext = _ext_or_skip()
    from doda_amd import spconv
    from doda_amd.spconv import functional as Fsp
    d = dev()
    idx, tbl = _scene_table(50000, seed=11)
    n = tbl.shape[1]
    torch.manual_seed(0)
    x = torch.randn(n, 16, device=d).bfloat16()
    w = torch.nn.Parameter((torch.randn(3, 3, 3, 16, 16, device=d) * 0.1))
    res = torch.randn(n, 16, device=d).bfloat16()
    t = ext.with_tilebook(tbl)
    y0, s0 = ext.indice_conv_stats(x, w, tbl, tbl, n, 2, None, None, res)
    y1, s1 = ext.indice_conv_stats(x, w, t, t, n, 2, None, None, res)
    # one statistics row per persistent workgroup (<= 768; round 2: one per tile)
    assert s1 is not None and 1 <= s1.shape[0] <= min(768, ((n + 255) // 256 + 7) // 8 * 8)
    assert (y0 != y1).float().mean().item() < 0.02
    from tests.util import stats_sums
    assert rel_err(stats_sums(s1).cpu(), stats_sums(s0).cpu()) < 1e-3
    yf = y1.detach().double()
    assert rel_err(stats_sums(s1)[0].cpu(), yf.sum(0).cpu()) < 1e-5
    assert rel_err(stats_sums(s1)[1].cpu(), (yf * yf).sum(0).cpu()) < 1e-5
    # BatchNorm -> ReLU -> conv, backward through the data-grad statistics
    bn = torch.nn.BatchNorm1d(16, eps=1e-4).to(d).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    conv = spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="k").to(d)
    seq = spconv.SparseSequential(bn, torch.nn.ReLU(), conv).train()
    outs = []
    for tiled in (False, True):
        bn.zero_grad(set_to_none=True)
        conv.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_(True)
        inp = spconv.SparseConvTensor(xin, idx, [80, 70, 60], 2)
        data = spconv.ops.build_subm(idx, 2, [80, 70, 60], 3)
        if tiled:
            data.tbl = ext.with_tilebook(data.tbl)
        inp.indice_dict["k"] = data
        out = seq(inp).features
        out.float().square().mean().backward()
        outs.append((out.detach().clone(), xin.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone(),
                     conv.weight.grad.clone()))
    for a, b in zip(*outs):
        assert rel_err(b.float().cpu(), a.float().cpu()) < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_unet_step_with_and_without_tilebooks(native_lib, dtype, monkeypatch):
    _ext_or_skip()
    from doda_amd import spconv
    from doda_amd.model import SparseConvNet, cross_entropy, default_cfg, voxelize_and_run
    from doda_amd.scene import make_batch
    d = dev()
    cfg = default_cfg()
    bd = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in make_batch(2, 40000, 5).items()}
    net = deterministic_init(SparseConvNet(cfg), seed=1).to(d).train()
    import doda_amd.model as dmodel
    monkeypatch.setattr(dmodel, "tile_levels_for", lambda dt: 2 if dt == torch.bfloat16 else 1)   # fp32: opt in
    runs = []
    old = spconv.ops.TILE_KERNEL
    try:
        for tiled in (False, True):
            spconv.ops.TILE_KERNEL = tiled
            net.zero_grad(set_to_none=True)
            loss = cross_entropy(voxelize_and_run(cfg, net, bd, d, feature_dtype=dtype), bd["labels"])
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.item(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        spconv.ops.TILE_KERNEL = old
    tol = (2e-2, 0.1) if dtype == torch.bfloat16 else (1e-4, 2e-2)
    assert abs(runs[0][0] - runs[1][0]) < tol[0] * abs(runs[0][0])
    for k, g0 in runs[0][1].items():
        g1 = runs[1][1][k]
        assert (g0.float() - g1.float()).norm().item() <= tol[1] * g0.float().norm().item() + 1e-6, k


def test_safety_valve_for_voxel_orders_without_locality(native_lib):
    """A shuffled voxel order makes every tile exceed the staging capacity: the pyramid builder notices (overflow
    counters of the tilebook), hands out plain tables for this batch and skips tilebooks for the next batches."""
    ext = _ext_or_skip()
    from doda_amd import spconv
    d = dev()
    from doda_amd.scene import make_batch
    b = make_batch(1, 40000, 7)                                          # dense surfaces: ~9 neighbours per voxel
    shape = [int(v) for v in b["spatial_shape"]]
    idx = b["voxel_locs"].int()
    idx = idx[torch.randperm(idx.shape[0], generator=torch.Generator().manual_seed(1))].contiguous().to(d)
    state = spconv.ops._tile_state
    saved = dict(state)
    try:
        state["skip"] = 0
        t = spconv.SparseConvTensor(None, idx, shape, 1)
        spconv.ops.build_pyramid(t, 3, with_tiles=2)
        nt, over64, over32 = state["last"]
        assert over32 > 0.9 * nt and state["skip"] == spconv.ops.TILE_BACKOFF
        assert not ext.has_tilebook(t.indice_dict["subm1"].tbl)
        # a well-ordered batch while the valve is closed: no tilebooks either, the counter runs down
        key = ((idx[:, 0].long() * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]
        idx2 = idx[torch.argsort(key)].contiguous()
        t2 = spconv.SparseConvTensor(None, idx2, shape, 1)
        spconv.ops.build_pyramid(t2, 3, with_tiles=2)
        assert not ext.has_tilebook(t2.indice_dict["subm1"].tbl) and state["skip"] == spconv.ops.TILE_BACKOFF - 1
        state["skip"] = 0
        t3 = spconv.SparseConvTensor(None, idx2, shape, 1)
        spconv.ops.build_pyramid(t3, 3, with_tiles=2)
        assert ext.has_tilebook(t3.indice_dict["subm1"].tbl) and state["skip"] == 0
        assert state["last"][2] <= 0.05 * state["last"][0]   # (x-major order: a few tiles above the list capacity)
    finally:
        state.update(saved)


@pytest.mark.parametrize("m,layout", [(20000, 0), (20000, 2), (8300, 0), (90000, 0), (90000, 2)])
def test_weights_in_lds_kernel_48_channels(native_lib, m, layout):
    """conv_wlds48 (bf16 48 -> 48, the level-3 layers): against the fp64 oracle on bf16-representable operands, against
    the streaming-weights kernel (switch off), with residual; statistics rows through the extension.  m = 90000: more than
    256 tiles of 256 rows — workgroups take a SECOND pass (level 3 of batches above ~6 scenes and of every 1 cm batch)."""
    from doda_amd import ops
    from doda_amd._lib import lib
    d = dev()
    _, tbl = (_scene_table(m, seed=31 + m, shape=(160, 140, 90)) if m > 40000 else _scene_table(m, seed=31 + m))
    n = tbl.shape[1]
    assert n >= 8192 and (m < 40000 or n > 256 * 256 + 1000)
    torch.manual_seed(m)
    x = torch.randn(n, 48, device=d).bfloat16()
    w = (torch.randn(27, 48, 48, device=d) * 0.1).bfloat16().float()
    wk = w if layout == 0 else w.transpose(1, 2).contiguous()
    ref = _oracle_conv(x, wk, tbl, layout)
    res = torch.randn(n, 48, device=d).bfloat16()
    try:
        lib().doda_set_option(2, 0)   # DODA_OPT_WLDS_KERNEL
        y_stream = ops.spconv_gather(x, wk, tbl, n, layout, 48)
        lib().doda_set_option(2, 1)
        y = ops.spconv_gather(x, wk, tbl, n, layout, 48)
        y_res = ops.spconv_gather(x, wk, tbl, n, layout, 48, residual=res)
    finally:
        lib().doda_set_option(2, 1)
    assert rel_err(y.float().cpu(), ref) < 2.0 ** -7
    assert (y != y_stream).float().mean().item() < 0.02
    assert rel_err(y_res.float().cpu(), ref + res.double().cpu()) < 2.0 ** -7
    ext = _ext_or_skip()
    wt = torch.nn.Parameter(w.view(3, 3, 3, 48, 48).clone())
    with torch.no_grad():
        yy, st = ext.indice_conv_stats(x, wt, tbl, tbl, n, 2, None, None, res)
    # (rows of the launch, or — ABI 9, the default — the fp64 totals [8, 2, c] its workgroups added their sums to)
    from tests.util import stats_sums
    assert st is not None and (st.shape[0] == (n + 255) // 256 or (st.dtype == torch.float64 and st.shape[0] == 8))
    yf = yy.double()
    assert rel_err(stats_sums(st)[0].cpu(), yf.sum(0).cpu()) < 1e-5
    assert rel_err(stats_sums(st)[1].cpu(), (yf * yf).sum(0).cpu()) < 1e-5

"""The wide LDS-staged weight gradient (csrc/spconv_wwide.hip): bf16 SubM K = 27 layers of 48 .. 224 channels over the
tilebooks of levels 3-7, on the rulebooks of a bench-sized batch (4 x 150 k voxels, the loader's Z-order numbering).
Every dW entry against a direct fp64 evaluation of dW[o] = x[nbr[o]]^T dy, in overwrite and accumulate mode, with tiles
above the list capacity (the dense-table fallback), a repeated call, and one mixed call of every job class."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (level, ca, cb): the SubM layers of levels 3-7 and their 2C -> C tail layers
SHAPES = [(3, 48, 48), (3, 96, 48), (4, 64, 64), (4, 128, 64), (5, 80, 80), (5, 160, 80), (6, 96, 96), (6, 192, 96),
          (7, 112, 112)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pyramid():
    """{level: (indices, SubM table)} for levels 1-7 and the k2 s2 child tables, bench scene in Z order"""
    from doda_amd import ops
    from doda_amd.collate import reorder_voxels
    from doda_amd.scene import make_batch
    d = dev()
    b = reorder_voxels(make_batch(4, 150000, 1000, 50), "morton")
    idx = b["voxel_locs"].int().to(d)
    shape = [int(s) for s in b["spatial_shape"]]
    levels, child = {}, {}
    for lvl in range(1, 8):
        levels[lvl] = (idx, ops.rulebook_subm(idx, shape, 4, 3), list(shape))
        if lvl < 7:
            idx, child[lvl], _, shape = ops.rulebook_down2(idx, shape, 4)
    return levels, child


def ref_dw(x, dy, tbl):
    ca, cb = x.shape[1], dy.shape[1]
    out = torch.empty(tbl.shape[0], ca, cb, dtype=torch.float64, device=x.device)
    for o in range(tbl.shape[0]):
        nbo = tbl[o].long()
        ok = nbo >= 0
        out[o] = x[nbo[ok]].double().t() @ dy[ok].double()
    return out


def check(got, ref):
    rel = float((got.double() - ref).norm() / ref.norm())
    mx = float((got.double() - ref).abs().max() / ref.abs().max())
    assert rel < 1e-4 and mx < 1e-3, (rel, mx)


def operands(n, ca, cb, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, ca, generator=g).bfloat16().to(dev()), torch.randn(n, cb, generator=g).bfloat16().to(dev()))


def test_wide_wgrad_levels_3_to_7_vs_fp64(native_lib, pyramid):
    from doda_amd import ops
    levels, _ = pyramid
    jobs, refs, over = [], [], {}
    for k, (lvl, ca, cb) in enumerate(SHAPES):
        _, tbl, _ = levels[lvl]
        n = tbl.shape[1]
        tb = ops.tilebook_build(tbl)
        nt_over = tb[-8:].view(torch.int32).cpu().tolist()[1]
        over[lvl] = (nt_over, (n + 255) // 256)
        x, dy = operands(n, ca, cb, k)
        jobs.append((x, dy, tbl, n, None, None, tb))
        refs.append(ref_dw(x, dy, tbl))
    print("tiles above the list capacity (level: over, tiles):", over)
    outs = ops.spconv_wgrad_multi(jobs)
    for (lvl, ca, cb), got, ref in zip(SHAPES, outs, refs):
        check(got, ref)
    # repeated call: bit-equal
    again = ops.spconv_wgrad_multi(jobs)
    for a, b in zip(outs, again):
        assert torch.equal(a, b)
    # accumulate mode: an existing dW plus the new sum
    base = [torch.randn_like(o) for o in outs]
    acc = ops.spconv_wgrad_multi([j[:5] + (b.clone(),) + j[6:] for j, b in zip(jobs, base)])
    for got, ref, b in zip(acc, refs, base):
        check(got, ref + b.double())


def test_wide_wgrad_bit_equal_to_gather_table_kernel(native_lib, pyramid):
    """The wide kernel sums over the gather-table kernel's row chunks in its order: the same job without a tilebook (the
    gather-table kernel) gives the same bits, in overwrite and accumulate mode."""
    from doda_amd import ops
    levels, _ = pyramid
    for k, (lvl, ca, cb) in enumerate(SHAPES):
        _, tbl, _ = levels[lvl]
        n = tbl.shape[1]
        tb = ops.tilebook_build(tbl)
        x, dy = operands(n, ca, cb, 60 + k)
        wide, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, None, tb)])
        dense, = ops.spconv_wgrad_multi([(x, dy, tbl, n)])
        assert torch.equal(wide, dense), (lvl, ca, cb)
        base = torch.randn_like(wide)
        wide_acc, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, base.clone(), tb)])
        dense_acc, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, base.clone())])
        assert torch.equal(wide_acc, dense_acc), (lvl, ca, cb)


def test_wide_wgrad_dense_fallback_for_tiles_without_list(native_lib, pyramid):
    """A random voxel order: every level-3 tile references more rows than the list keeps (TB_LMAX) and takes the
    offset-by-offset dense-table path inside the kernel."""
    from doda_amd import ops
    levels, _ = pyramid
    idx, _, shape = levels[3]
    n = idx.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(idx.device)
    idx_r = idx[perm].contiguous()
    tbl = ops.rulebook_subm(idx_r, shape, 4, 3)
    tb = ops.tilebook_build(tbl)
    over = tb[-8:].view(torch.int32).cpu().tolist()[1]
    assert over > 0
    for k, (ca, cb) in enumerate([(48, 48), (96, 48)]):
        x, dy = operands(n, ca, cb, 10 + k)
        got, = ops.spconv_wgrad_multi([(x, dy, tbl, n, None, None, tb)])
        check(got, ref_dw(x, dy, tbl))
        dense, = ops.spconv_wgrad_multi([(x, dy, tbl, n)])
        assert torch.equal(got, dense)


def test_mixed_call_matches_separate_calls(native_lib, pyramid):
    """Level-1/2 tile jobs (wgrad_dma16), coarse wide jobs and K = 8 jobs in one call against the same jobs in calls of
    their own: the unchanged kernels bit-equal, the wide jobs bit-equal too (their plan depends on the wide jobs only)."""
    from doda_amd import ops
    levels, child = pyramid
    jobs = []
    for k, (lvl, c) in enumerate([(1, 16), (2, 32)]):
        _, tbl, _ = levels[lvl]
        n = tbl.shape[1]
        x, dy = operands(n, c, c, 20 + k)
        jobs.append(("tile", (x, dy, tbl, n, None, None, ops.tilebook_build(tbl))))
    wide = []
    for k, (lvl, ca, cb) in enumerate([(3, 48, 48), (5, 80, 80)]):
        _, tbl, _ = levels[lvl]
        n = tbl.shape[1]
        x, dy = operands(n, ca, cb, 30 + k)
        wide.append((x, dy, tbl, n, None, None, ops.tilebook_build(tbl)))
        jobs.append(("wide", wide[-1]))
    for k, (lvl, ca, cb) in enumerate([(3, 48, 64), (4, 64, 80)]):
        ch = child[lvl]                                   # [8, m_out]: fine rows of each coarse row
        n_out, n_in = ch.shape[1], levels[lvl][0].shape[0]
        x, _ = operands(n_in, ca, 16, 40 + k)
        _, dy = operands(n_out, 16, cb, 50 + k)
        jobs.append(("k8", (x, dy, ch, n_out)))
    mixed = ops.spconv_wgrad_multi([j for _, j in jobs])
    sep_wide = ops.spconv_wgrad_multi(wide)
    w = 0
    for (kind, j), got in zip(jobs, mixed):
        if kind == "wide":
            assert torch.equal(got, sep_wide[w])
            check(got, ref_dw(j[0], j[1], j[2]))
            w += 1
        else:
            alone, = ops.spconv_wgrad_multi([j])
            assert torch.equal(got, alone), kind

"""The BatchNorm sweeps of csrc/bn.hip in their two forms.  bn_apply / bn_bwd_apply<T, FIXED> keep a thread on one 16-byte column
(per-channel vectors in registers, 16-byte accesses) and are documented as "same arithmetic, same order: results unchanged bit
for bit" against the general sweeps (FIXED = false: any grid, 4-channel fragments).  The launchers take the general form when an
operand is not 16-byte aligned, so every BatchNorm wrapper of doda_amd.ops is called twice on the same values — x aligned, and x
in a contiguous view that starts 8 bytes into an aligned buffer — and every returned tensor has to be bit-equal.

bf16 only: a bf16 fragment is an 8-byte access, so rows that start 8 bytes past a 16-byte boundary are legal for the general
sweep; an fp32 fragment is a 16-byte access, and no misaligned fp32 operand satisfies that, so fp32 rows always run FIXED
whenever a FIXED grid exists (reference: torch.nn.BatchNorm1d + ReLU of model/unet_block.py:23-30)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 4097          # the smallest row count above BN_SMALL_ROWS: the multi-block kernels run
PARTS = 5         # statistics rows, built from the definition


def _shifted(t):
    """The values of t in a contiguous view that starts 8 bytes into a 16-byte-aligned flat buffer."""
    off = 8 // t.element_size()
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert flat.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8 and v.is_contiguous() and torch.equal(v, t)
    return v


def _same(what, a, b):
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert p.shape == q.shape and torch.equal(p, q), "%s: output %d differs between the aligned and the shifted x" % (what, k)


@pytest.mark.parametrize("c", [16, 48])
def test_general_sweeps_equal_the_fixed_sweeps_bit_for_bit(native_lib, c):
    from doda_amd import ops
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 + c)
    x = (torch.randn(M, c, generator=g) * 2 + 0.3).to(torch.bfloat16).to(d)
    dy = torch.randn(M, c, generator=g).to(torch.bfloat16).to(d)
    gamma = (torch.rand(c, generator=g) + 0.5).to(d)
    beta = (torch.randn(c, generator=g) * 0.1).to(d)
    dense = torch.randn(M, c, generator=g).to(torch.bfloat16).to(d)
    wide = torch.randn(M, 2 * c, generator=g).to(torch.bfloat16).to(d)
    xs = (x, _shifted(x))
    edges = torch.linspace(0, M, PARTS + 1).long()

    def rows_of(a, b):     # [PARTS, 2, c] fp32: (sum a, sum b) over PARTS row ranges
        return torch.stack([torch.stack([a[i:j].sum(0), b[i:j].sum(0)]) for i, j in zip(edges[:-1], edges[1:])]).contiguous()

    def fwd(call):         # forward calls get fresh running statistics, and those are compared too
        outs = []
        for xx in xs:
            rm, rv, nb = torch.zeros(c, device=d), torch.ones(c, device=d), torch.zeros((), dtype=torch.int64, device=d)
            outs.append(tuple(call(xx, rm, rv, nb)) + (rm, rv, nb))
        assert int(outs[0][-1]) == 1
        return outs

    o = fwd(lambda xx, rm, rv, nb: ops.bn_relu_fwd(xx, gamma, beta, rm, rv, True, 0.1, 1e-4, True, nb))
    _same("bn_relu_fwd", *o)
    mu, inv = o[0][1], o[0][2]
    xf = x.float()
    tot = ops.totals_from_rows(rows_of(xf, xf * xf))
    o = fwd(lambda xx, rm, rv, nb: ops.bn_relu_fwd_totals(xx, tot, gamma, beta, rm, rv, 0.1, 1e-4, True, nb))
    _same("bn_relu_fwd_totals", *o)

    xh = (xf - mu) * inv
    dz = torch.where(xh * gamma + beta > 0, dy.float(), torch.zeros((), device=d))
    rows_b = rows_of(dz, dz * xh)
    tot_b = ops.totals_from_rows(rows_b)
    _same("bn_relu_bwd", *[ops.bn_relu_bwd(xx, dy, mu, inv, gamma, beta, True) for xx in xs])
    for name, add in (("none", None), ("dense", dense), ("a column slice", wide[:, c:])):
        if add is not None:
            _same("bn_relu_bwd_add, add " + name, *[ops.bn_relu_bwd_add(xx, dy, mu, inv, gamma, beta, True, add) for xx in xs])
        _same("bn_relu_bwd_stats, add " + name, *[ops.bn_relu_bwd_stats(xx, dy, rows_b, mu, inv, gamma, beta, True, add=add) for xx in xs])
        _same("bn_relu_bwd_totals, add " + name, *[ops.bn_relu_bwd_totals(xx, dy, tot_b, mu, inv, gamma, beta, True, add=add) for xx in xs])

#!/usr/bin/env python
"""Which operators does the torch extension run for a training step, and on which routes?  One forward + backward of the default
SparseConvNet (bf16, deferred weight gradients, the prefetcher's pyramid) on a small seeded batch under DODA_FPLOG=1, three times:
  default       the whole U-Net as one op list per direction (coarse_ublock): its launch counts, the input conv, the output
                BatchNorm and every deferred weight-gradient job
  modules       DODA_COARSE_MODE=off: residual_block / indice_conv / bn_relu and their autograd nodes, statistics as fp64 totals
  modules_rows  ... with set_stats_totals(False): statistics as per-workgroup rows
Prints one JSON line: the rows per level and, per pass, the logged entry names in call order (operator/output, three arguments
[element count]; BatchNorm's third argument is its statistics route 0 / 1 / 2, the weight gradient's the accumulate flag) and
ext.coarse_launches().  --fingerprints adds each entry's fingerprint.  The batch is the smallest that reaches every route: the tool
fails when a condition below does not hold.  Run in a fresh process: the flag is read when the extension is loaded.
usage: DODA_FPLOG=1 extoplog.py [--fingerprints] [scenes=2] [voxels=20000]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from doda_amd import model as M, spconv
from doda_amd._ext import ext
from doda_amd.collate import reorder_voxels
from doda_amd.scene import make_batch

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ns = int(args[0]) if len(args) > 0 else 2
nv = int(args[1]) if len(args) > 1 else 20000
assert os.environ.get("DODA_FPLOG") == "1" and ext is not None
dev = torch.device("cuda:0")
Fsp = spconv.functional
STATS_MIN_ROWS = int(os.environ.get("DODA_STATS_MIN_ROWS", "4096"))

b = reorder_voxels(make_batch(ns, nv, 1000), "morton")
bd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
cfg = M.default_cfg()
torch.manual_seed(0)
net = M.SparseConvNet(cfg).to(dev).train()
assert Fsp.set_deferred_wgrad(True)
state = {k: v.clone() for k, v in net.state_dict().items()}
pf = M.PyramidPrefetcher(dev, len(net.unet.nPlanes))
out = {"levels": None, "passes": {}}


def one_pass(name):
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    pyr = M.PyramidPrefetcher.take(pf.submit(bd, bool(Fsp.WGRAD_PAIRS), M.tile_levels_for(torch.bfloat16), resident=True, now=True), dev)
    book = pyr[1]
    levels = [int(book["subm%d" % (k + 1)].tbl.shape[1]) for k in range(len(net.unet.nPlanes))]
    assert out["levels"] in (None, levels)
    out["levels"] = levels
    assert levels[0] >= spconv.ops.TILE_MIN_ROWS and ext.has_tilebook(book["subm1"].tbl), ("no tilebook at the finest level", levels)
    assert any(r > STATS_MIN_ROWS for r in levels) and any(2 <= r <= STATS_MIN_ROWS for r in levels), ("levels on one side of DODA_STATS_MIN_ROWS", levels)
    ext.fp_log_take()
    loss = M.voxelize_and_run(cfg, net, bd, dev, feature_dtype=torch.bfloat16, inputs_ready=True, pyramid=pyr, labels=bd["labels"])
    loss.backward()
    torch.cuda.synchronize()
    assert ext.pending_wgrads() == 0 and all(p.grad is not None for p in net.parameters())
    log = ext.fp_log_take()
    out["passes"][name] = {"names": [n for n, _ in log], "coarse_launches": list(ext.coarse_launches())}
    if "--fingerprints" in sys.argv:
        out["passes"][name]["fingerprints"] = [int(v) for _, v in log]
    return [n for n, _ in log]


def routes(names, op):
    return {int(n.split()[-2]) for n in names if n.startswith(op + " ")}   # the third argument: the statistics route


try:
    names = one_pass("default")
    fwd, bwd = out["passes"]["default"]["coarse_launches"]
    assert fwd > 0 and bwd > 0, "the coarse levels did not enter coarse_ublock"
    n_dw = sum(1 for n in names if n.startswith("weight gradient/dw "))
    assert n_dw > 0 and routes(names, "weight gradient/dw") == {0}, "no deferred weight-gradient jobs, or one that accumulated"
    assert routes(names, "bn forward/y") == {2} and routes(names, "bn backward/dx") >= {0}

    M.set_coarse_mode("off")
    before = list(ext.coarse_launches())
    names = one_pass("modules")
    assert list(ext.coarse_launches()) == before, "module by module, yet an op list ran"
    # both sides of DODA_STATS_MIN_ROWS: the one-launch kernels (0) below it, statistics from the conv epilogues (2: totals) above
    assert routes(names, "bn forward/y") == {0, 2} and routes(names, "bn backward/dx") == {0, 2}
    assert sum(1 for n in names if n.startswith("weight gradient/dw ")) == n_dw

    ext.set_stats_totals(False)
    names = one_pass("modules_rows")
    assert routes(names, "bn forward/y") == {0, 1} and routes(names, "bn backward/dx") == {0, 1}
finally:
    ext.set_stats_totals(True)
    pf.shutdown()
print(json.dumps(out))

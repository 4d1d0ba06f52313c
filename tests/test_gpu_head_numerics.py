"""What the head and loss kernels COMPUTE at their edges: all 62 compiled kernels of csrc/head.hip, csrc/lovasz.hip and csrc/loss.hip
(tests/test_head_numerics_host.py holds the probed and the compiled names to one set) against fp64 references from the definitions,
element by element, under derived bounds — the probe table, the references and the derivations are tools/headnumerics.py's docstring
and functions.  Per probe, through the C ABI into sentinel-padded buffers: the status, the restated block counts and workspace size,
the exact outputs (valid count / present classes, count partials, zero rows, pred on decided voxels, the meters' histograms), every
other output within  max(4 x the ratio of the reference model's own fp32 path on the same probe and device, the derived operation
count) x u x scale,  each workgroup's own partial row, intact sentinels and the same bits from a repeated call.

One test per group, one case per probe, all in this process (the three files read no environment switch)."""
import importlib.util
import os

import pytest
import torch  # noqa: F401  (before the native library is loaded, as in every GPU test: both then share torch's HIP runtime)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("headnumerics", os.path.join(ROOT, "tools", "headnumerics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hn = _load()
BY_ID = {p["id"]: p for p in hn.probes()}
ids = lambda g: [p["id"] for p in hn.probes(g)]


def _probe(pid):
    p = BY_ID[pid]
    res = hn.run_probe(p)
    print("%s: status %d  %s" % (pid, res["status"], "  ".join("%s %.3g/%s/%.3g" % (k, v[0], "-" if v[1] is None else "%.3g" % v[1], v[2])
                                                                for k, v in res["table"].items())))
    assert res["status"] == p["status"], res
    assert res["guards"] and res["repeat"], res
    assert res["fails"] == [], res
    assert p["status"] or res["table"] or p["group"] == "E", res
    assert all(v[0] <= v[2] for v in res["table"].values()), res


@pytest.mark.parametrize("pid", ids("A"))
def test_head_ce(native_lib, pid):
    _probe(pid)


@pytest.mark.parametrize("pid", ids("B"))
def test_head_dw_bf16(native_lib, pid):
    _probe(pid)


@pytest.mark.parametrize("pid", ids("C"))
def test_voxel_confidence(native_lib, pid):
    _probe(pid)


@pytest.mark.parametrize("pid", ids("D"))
def test_cross_entropy(native_lib, pid):
    _probe(pid)


@pytest.mark.parametrize("pid", ids("E"))
def test_seg_meters(native_lib, pid):
    _probe(pid)


@pytest.mark.parametrize("pid", ids("F"))
def test_lovasz(native_lib, pid):
    _probe(pid)

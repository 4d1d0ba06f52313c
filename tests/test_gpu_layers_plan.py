"""doda_layers_run plans its whole list on the host (csrc/layers_plan.hpp), then launches.  On the MI355X: the launches the
library issues for the probe set of tools/layersplan.py are the plan's steps and the launches recorded before the plan existed
(tests/data/layers_plan_parent.json), and a list with a defect behind a valid op returns its error with NOTHING enqueued — the
first op's outputs, running statistics and batch counter keep their sentinels (before the plan the first op had run)."""
import ctypes as C
import importlib.util
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("layersplan", os.path.join(ROOT, "tools", "layersplan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_traces_equal_the_plan_and_the_record(native_lib, tmp_path):
    """One fresh child process runs every probe with DODA_TRACE_GATHER=1 DODA_TRACE_BN=1."""
    lp = _tool()
    run = lp.run_on_gpu()
    rec = json.load(open(os.path.join(ROOT, "tests", "data", "layers_plan_parent.json")))
    got, record = run["probes"], rec["probes"]
    lists = lp.host_lists()
    plans = lp.planner(str(tmp_path / "plan"))([l for _, _, _, text in lists for l in text])
    assert [g["name"] for g in got] == [r["name"] for r in record] == [l[0] for l in lists]
    for g, r, (name, esz, lst, _), p in zip(got, record, lists, plans):
        assert g["status"] == r["status"] == p["status"], (name, g, p)
        if g["status"] != OK:
            assert g["trace"] == [] and g["launches"] == 0 and p["steps"] == [], (name, g)     # refused before anything launched
            continue
        assert g["trace"] == lp.launched(r["trace"]) and g["launches"] == r["launches"] == len(p["steps"]), (name, g, r)
        assert lp.parse_trace(g["trace"]) == lp.expected(lst, esz, p["steps"]), (name, g, p)
    # the lists the compiled extension builds for UBlock(7) over 83 voxels, forward and backward: the record's launches, in order
    assert [g["name"] for g in run["subtrees"]] == [r["name"] for r in rec["subtrees"]] == ["7_83_2", "7_83_4"]
    for g, r in zip(run["subtrees"], rec["subtrees"]):
        assert g["launches"] == r["launches"] == len(g["trace"]) > 0 and g["trace"] == lp.launched(r["trace"]), (g, r)


@pytest.mark.parametrize("bad", ["bn_264_channels", "gemm_null_w"])
def test_a_refused_list_has_enqueued_nothing(native_lib, bad):
    from doda_amd import ops
    from doda_amd._lib import lib
    lp = _tool()
    d = torch.device("cuda:0")
    A = lp.Alloc(2, d)
    n, c = 64, 32
    first = lp.bnfwd(A, n, c)
    first.update(stats=ops.stats_totals(c, d))
    sent = dict(y=torch.full((n, c), 7.0, dtype=torch.bfloat16, device=d), mean=torch.full((c,), 3.0, device=d),
                invstd=torch.full((c,), 5.0, device=d), running_mean=torch.full((c,), -2.0, device=d),
                running_var=torch.full((c,), 9.0, device=d), nbt=torch.full((1,), 11, dtype=torch.int64, device=d))
    first.update(sent)
    if bad == "bn_264_channels":
        second, status = lp.bnfwd(A, n, 264), UNSUPPORTED
    else:
        second, status = dict(lp.gemm(A, n, c, c, A.feat(n, c)), w=None), INVALID
    lst = [first, second]
    arr = ops._cx_array(lst, 0)
    launches = C.c_int32(-1)
    st = lib().doda_layers_run(C.cast(arr, C.c_void_p), len(lst), 2, C.byref(launches), ops._stream())
    torch.cuda.synchronize()
    assert st == status and launches.value == 0
    for k, v in (("y", 7.0), ("mean", 3.0), ("invstd", 5.0), ("running_mean", -2.0), ("running_var", 9.0), ("nbt", 11)):
        assert bool((sent[k] == v).all()), k
    # the valid op alone does run: the sentinels are what a launch would have overwritten
    assert ops.layers_run([first], d, 2) == 1
    torch.cuda.synchronize()
    assert int(sent["nbt"]) == 12 and not bool((sent["y"] == 7.0).all()) and not bool((sent["mean"] == 3.0).all())

"""The torch extension (doda_amd/csrc_ext/doda_torch.cpp) runs the operators, on the routes, that tests/data/ext_oplog_parent.json
records: tools/extoplog.py, in one fresh child process with DODA_FPLOG=1, makes a forward + backward of the default SparseConvNet
(bf16, deferred weight gradients, the prefetcher's pyramid) as one op list per direction, module by module with statistics as fp64
totals, and module by module with statistics rows.  The names of the logged entries (operator/output, shapes, BatchNorm statistics
route or weight-gradient accumulate flag, element count), in call order, and the op lists' launch counts must equal the recording —
made before the extension's marshals, flush steps and BatchNorm routes were folded into one copy each — entry for entry."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "extoplog.py")


def test_operators_and_routes_equal_the_recording(native_lib):
    env = dict(os.environ, DODA_FPLOG="1")
    for k in ("DODA_STATS_MIN_ROWS", "DODA_STATS_TOTALS", "DODA_COARSE_MODE", "DODA_COARSE_LEVEL", "DODA_POISON", "DODA_NANCHECK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, TOOL], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    want = json.load(open(os.path.join(ROOT, "tests", "data", "ext_oplog_parent.json")))
    assert got["levels"] == want["levels"]
    assert sorted(got["passes"]) == sorted(want["passes"]) == ["default", "modules", "modules_rows"]
    for name, rec in want["passes"].items():
        run = got["passes"][name]
        print("%s: %d entries, op-list launches %s" % (name, len(run["names"]), run["coarse_launches"]))
        assert run["coarse_launches"] == rec["coarse_launches"], name
        assert len(run["names"]) == len(rec["names"]) > 0, name
        first = next((k for k, (a, b) in enumerate(zip(run["names"], rec["names"])) if a != b), None)
        assert first is None, (name, first, run["names"][first], rec["names"][first])

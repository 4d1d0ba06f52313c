"""What every BatchNorm kernel of csrc/bn.hip and every BatchNorm / statistics op of csrc/layers.hip COMPUTES, on every route of the
selection and on both sides of each of its thresholds: all 41 compiled instantiations (tests/test_bn_numerics_host.py holds the
probed and the compiled names to one set) against an fp64 reference from the definition, under derived bounds — the probe table,
the references and the derivations are tools/bnnumerics.py's docstring and functions.  Per probe: the traced launches
(DODA_TRACE_BN: kernel, grid, workgroup) are exactly the expected ones, every statistic, vector and element is within its bound
(error / bound <= 1), the sentinels around every output are intact and an error return wrote nothing.

One fresh child process per group (tools/bnnumerics.py --numerics GROUP: the switches are read once per process), with the group's
environment and the other BatchNorm switches removed, one at a time; after a child that ended on a signal, at its time limit or
with an illegal memory access in its output the remaining groups fail without starting one."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bnnumerics.py")


def _load():
    spec = importlib.util.spec_from_file_location("bnnumerics", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bn = _load()
TIMEOUT = 60       # seconds per child: process start (torch, the library) dominates; the largest probe has 39 063 x 64 elements
_dead = []      # groups whose child ended on a signal, at its time limit or after a fault


@pytest.mark.parametrize("group", list(bn.GROUPS))
def test_every_route_matches_fp64(native_lib, group):
    if _dead:
        pytest.fail("not started: the child of group %s ended on a signal, at its time limit or after a fault" % _dead[0])
    probes = bn.probes(group)
    assert probes
    env = {k: v for k, v in os.environ.items() if k not in bn.SWITCHES}
    env.update(bn.GROUPS[group], DODA_TRACE_BN="1")
    try:
        r = subprocess.run([sys.executable, TOOL, "--numerics", group], env=env, capture_output=True, text=True, timeout=TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append(group)
        raise
    if r.returncode < 0 or "illegal memory access" in r.stdout + r.stderr:
        _dead.append(group)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    res = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    got = [g for g in res if "trace" not in g]
    assert [g["id"] for g in got] == [p["id"] for p in probes]
    assert len([t for t in res if "trace" in t]) == sum(len(bn.routes(p)) for p in probes)
    for p, g in zip(probes, got):
        print("%s: x %.3g  %s" % (g["id"], g["ratio"], json.dumps(g["err"])))
        assert g["status"] == p["status"], g
        assert g["route"] == [list(t) for t in bn.routes(p)], g
        assert g["guards"], g
        assert g["fails"] == [], g
        assert all(v[1] <= 1.0 for v in g["err"].values()) and g["ratio"] <= 1.0, g
        assert p["status"] or g["err"], g

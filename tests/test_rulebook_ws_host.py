"""The rulebook workspace rule, host side (no GPU): doda_rulebook_workspace_bytes_grid is the one statement of how large a
workspace selects the direct-address grid (include/doda_hip.h, ABI 13), and the one workspace carver of csrc/rulebook.hip
returns what the two carvers of the parent commit returned (tests/data/rulebook_workspace_parent.json)."""
import json
import os
import subprocess
import sys

from doda_amd import _lib

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "rulebook_workspace_parent.json")
LIMIT = 0x3fffffff   # the generic builder's bound on m * K

# what a child process prints for a list of (m, batch, shape): the library alone reads the two environment variables, once
CHILD = """
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
for f, args in (("doda_rulebook_workspace_bytes", [C.c_int32]), ("doda_rulebook_workspace_bytes_grid", [C.c_int32, C.c_int32, C.c_void_p])):
    getattr(lib, f).restype, getattr(lib, f).argtypes = C.c_size_t, args
print(json.dumps([[lib.doda_rulebook_workspace_bytes(m), lib.doda_rulebook_workspace_bytes_grid(m, b, (C.c_int32 * 3)(*s))]
                  for m, b, s in json.loads(sys.argv[2])]))
"""


def _align256(n):
    return (n + 255) // 256 * 256


def _grid(lib, m, batch, shape):
    import ctypes as C
    return lib.doda_rulebook_workspace_bytes_grid(m, batch, (C.c_int32 * 3)(*shape))


def _child(env, cases):
    env = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH, json.dumps(cases)], env=env, capture_output=True, text=True,
                       timeout=120, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_grid_workspace_query_states_the_rule(native_lib):
    m = 1000
    base = native_lib.doda_rulebook_workspace_bytes(m)
    # exactly 2^28 cells: the grid; one more: the minimum (hash) workspace
    assert _grid(native_lib, m, 4, [1 << 10, 1 << 8, 1 << 8]) == _align256(base) + 4 * (1 << 28)
    assert _grid(native_lib, m, 1, [(1 << 28) + 1, 1, 1]) == base
    assert _grid(native_lib, m, 2, [100, 90, 80]) == _align256(base) + 4 * 2 * 100 * 90 * 80
    # nothing to build, or no cell map: the minimum
    assert _grid(native_lib, 0, 2, [100, 90, 80]) == native_lib.doda_rulebook_workspace_bytes(0)
    for batch, shape in ((2, [100, 0, 80]), (0, [100, 90, 80]), (2, [-1, 90, 80]), (-2, [100, 90, 80])):
        assert _grid(native_lib, m, batch, shape) == base
    assert native_lib.doda_rulebook_workspace_bytes_grid(m, 2, None) == base


def test_grid_workspace_query_follows_the_library_switches(native_lib):
    cases = [[1000, 2, [100, 90, 80]], [1000, 1, [1 << 10, 1 << 10, 1]], [1000, 1, [(1 << 20) + 1, 1, 1]]]
    for base, got in _child({"DODA_RULEBOOK_GRID": "0"}, cases):
        assert got == base
    (b0, g0), (b1, g1), (b2, g2) = _child({"DODA_RULEBOOK_GRID": "1", "DODA_RULEBOOK_GRID_MAX_LOG2": "20"}, cases)
    assert g0 == b0                                  # 1 440 000 cells: above 2^20
    assert g1 == _align256(b1) + 4 * (1 << 20)       # exactly 2^20
    assert g2 == b2                                  # 2^20 + 1


def test_one_carver_returns_the_parent_sizes(native_lib):
    with open(DATA) as f:
        rec = json.load(f)
    rows, conv = {m: v for m, v in rec["rows"]}, {(m, K): v for m, K, v in rec["conv"]}
    want_m = {0, 1, 511, 512, 513} | {(1 << b) + d for b in range(25) for d in (-1, 0, 1)}
    assert want_m <= set(rows)
    assert {(m, K) for m in want_m for K in (1, 8, 27)} | {(LIMIT // K + d, K) for K in (1, 8, 27) for d in (0, 1)} <= set(conv)
    for m, v in rows.items():
        assert native_lib.doda_rulebook_workspace_bytes(m) == v, m
    for (m, K), v in conv.items():
        assert native_lib.doda_rulebook_conv_workspace_bytes(m, K) == v, (m, K)
        assert (v == 0) == (m * K > LIMIT)

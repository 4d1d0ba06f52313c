"""The C ABI, host side (no GPU): every header under include/ against its record in doda_amd._lib.ABIS (tests/abi_header.py:
prototypes argument by argument, struct layouts, mirrored constants), the built library against the records, the figures a
maintainer carries, and the checker itself against doctored headers."""
import ctypes as C
import os
import re

import pytest

from doda_amd import _lib, ops
from tests import abi_header, optim_cases, pgops_cases, pointops_cases

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
RECORDS = {abi.header: abi for abi in _lib.ABIS}
# header -> (name prefix, number of functions or None, ABI version); a header without a row: ("doda_", None, 1)
PINNED = {"doda_hip.h": ("doda_", 71, 13), "doda_selftrain.h": ("doda_st_", 5, 1), "doda_mix.h": ("doda_mix_", 6, 1),
          "doda_aug.h": ("doda_aug_", None, 1), "doda_eval.h": ("doda_eval_", None, 1), "doda_subsample.h": ("doda_subsample_", None, 1),
          "doda_optim.h": ("doda_optim_", None, 1), "doda_pgops.h": ("doda_pg", 11, 1), "doda_pointops.h": ("doda_po", 12, 1)}
SIZEOF = {"doda_conv_epilogue": 120, "doda_wgrad_job": 120, "doda_sgd_tensor": 40, "doda_cx_op": 224, "doda_eval_scene": 44,
          "doda_optim_tensor": 64, "doda_optim_hyper": 48}
# module-level ints of _lib.py and ops.py that mirror csrc/ constants, not a header's
CSRC_MIRRORS = {"CX_BN_MAX_C", "_PHILOX_M0", "_PHILOX_M1", "_PHILOX_W0", "_PHILOX_W1"}


def _text(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return f.read()


@pytest.mark.parametrize("header", HEADERS)
def test_header_matches_its_record_and_the_library(native_lib, header):
    assert header in RECORDS, "include/%s has no record in doda_amd._lib.ABIS" % header
    abi = RECORDS[header]
    assert abi_header.compare(_text(header), abi) == []
    prefix, count, version = PINNED.get(header, ("doda_", None, 1))
    assert all(name.startswith(prefix) for name in abi.signatures) and count in (None, len(abi.signatures))
    assert abi.version == version == getattr(native_lib, abi.version_fn)()
    for name in abi.signatures:
        assert hasattr(native_lib, name), name
    for name, mirror in abi.structs.items():
        assert C.sizeof(mirror) == SIZEOF[name], name


def test_records_cover_the_headers_with_disjoint_symbol_sets(native_lib):
    assert sorted(RECORDS) == HEADERS and len(_lib.ABIS) == len(RECORDS)
    names = [name for abi in _lib.ABIS for name in abi.signatures]
    assert len(names) == len(set(names))
    assert _lib.EXPORTED_SYMBOLS == tuple(RECORDS["doda_hip.h"].signatures) and _lib.ABI_VERSION == 13
    assert len(_lib.EXPORTED_SYMBOLS) <= 71      # (the boundary a maintainer carries; ABI 8: four executor entry points, ABI 9: BatchNorm over totals, ABI 11: doda_layers_run, ABI 13: the rulebook workspace rule)
    assert native_lib.doda_strerror(-3).decode().startswith("cell id")


def test_every_mirrored_constant_belongs_to_a_record():
    known = {}
    for abi in _lib.ABIS:
        assert not set(known) & set(abi.constants)
        known.update(abi.constants)
    for module in (_lib, ops):
        for name, value in vars(module).items():
            if re.fullmatch(r"_?[A-Z][A-Z0-9_]*", name) and type(value) is int and name not in CSRC_MIRRORS:
                assert known.get(name) == value, "%s.%s mirrors no header's #define" % (module.__name__, name)
    assert _lib.PG_LONG_SEGMENT == pgops_cases.LONG_SEGMENT
    assert (_lib.OPTIM_TILE, _lib.OPTIM_NORM_BLOCKS) == (optim_cases.TILE, optim_cases.NORM_BLOCKS)
    assert (_lib.OPTIM_SGD, _lib.OPTIM_ADAM, _lib.OPTIM_ADAMW) == (0, 1, 2)
    assert (_lib.PO_WAVE_LIST, _lib.PO_FPS_BLOCK, _lib.PO_FPS_REG) == (pointops_cases.WAVE_LIST, pointops_cases.FPS_BLOCK, pointops_cases.FPS_REG)
    assert _lib.SUBSAMPLE_MAX_SEGMENTS >= 32 and _lib.AUG_MAX_GRID_CELLS == 1 << 24
    text = _text("doda_pointops.h")
    assert "deliberate fix" in text and "TIES GO TO THE LOWEST POINT INDEX" in text


# ---- the checker itself: a toy header that its record matches, then one doctored copy per kind of drift -------------------------
TOY = """
/* doda_toy_gone(int) is only mentioned here */
#ifdef __cplusplus
extern "C" {
#endif
#define DODA_TOY_ABI_VERSION 3
#define DODA_TOY_LIMIT (1 << 4)   /* of anything */
typedef struct {
    uint64_t seed;
    int32_t n;
    float scale;
    const float *x, *y;
} doda_toy_item;
int doda_toy_abi_version(void);
int doda_toy_run(const doda_toy_item *items_h, int32_t n, float eps, int64_t *total_h, doda_stream_t stream);
#ifdef __cplusplus
}
#endif
"""


class ToyItem(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n", C.c_int32), ("scale", C.c_float), ("x", C.c_void_p), ("y", C.c_void_p)]


TOY_ABI = _lib.Abi("toy.h", "doda_toy_abi_version", 3, "toy ABI", {
    "doda_toy_abi_version": (C.c_int32, []),
    "doda_toy_run": (C.c_int32, [C.POINTER(ToyItem), C.c_int32, C.c_float, C.POINTER(C.c_int64), C.c_void_p]),
}, structs={"doda_toy_item": ToyItem}, constants={"TOY_LIMIT": 16})
RUN = "int doda_toy_run(const doda_toy_item *items_h, int32_t n, float eps, int64_t *total_h, doda_stream_t stream);\n"
DRIFTS = {   # what changed -> (text of TOY, its replacement, the mismatch the comparison must name)
    "int32_t argument to int64_t": ("int32_t n, float eps", "int64_t n, float eps", "function doda_toy_run: argument 1: header int64_t"),
    "dropped argument": (", float eps", "", "function doda_toy_run: argument count: header 4, table 5"),
    "float to double": ("float eps", "double eps", "function doda_toy_run: argument 2: header double, table c_float"),
    "struct field removed": ("    float scale;\n", "", "struct doda_toy_item: field names"),
    "two struct fields swapped": ("int32_t n;\n    float scale;", "float scale;\n    int32_t n;", "struct doda_toy_item: field names"),
    "uint64_t field to uint32_t": ("uint64_t seed", "uint32_t seed", "struct doda_toy_item: field n: header int32_t at 4 (4 bytes), mirror c_int at 8"),
    "changed #define": ("(1 << 4)", "(1 << 5)", "constant TOY_LIMIT: header 32, mirror 16"),
    "prototype in the header only": (RUN, RUN + "void doda_toy_extra(void);\n", "function doda_toy_extra: in the header only"),
    "prototype in the table only": (RUN, "", "function doda_toy_run: in the table only"),
}


@pytest.mark.parametrize("drift", DRIFTS)
def test_comparison_reports(drift):
    old, new, expected = DRIFTS[drift]
    assert abi_header.compare(TOY, TOY_ABI) == [] and TOY.count(old) == 1
    found = abi_header.compare(TOY.replace(old, new), TOY_ABI)
    assert any(line.startswith(expected) for line in found), found


def test_reader_refuses_what_it_does_not_know():
    for text in ("int doda_toy_f(long double x);", "#define DODA_TOY_X sizeof(int)", "#define DODA_TOY_X (1 << )", "int doda_toy_v = 3;",
                 TOY.replace("float eps", "long eps"), TOY.replace("float scale", "char scale")):
        with pytest.raises(ValueError):
            abi_header.compare(text, TOY_ABI)

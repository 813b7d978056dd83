"""The C ABI of the subdivision (include/ezrt_subdivide.h) against its ctypes table (ezrt_amd/_abi.py: SUBDIVIDE_ABI): the header's names
are the table's, no other table declares them, the library binds them with the table's argument types, and the header carries the rule.
Needs no GPU: the library is only opened, and the one function called (ezrt_subdivide_work_bytes) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_subdivide_rows_device", "ezrt_subdivide_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_subdivide.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.SUBDIVIDE_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.SUBDIVIDE_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    call = " ".join(protos["ezrt_subdivide_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "int mode", "const int32_t* twin", "const uint8_t* edge_class",
                  "const int32_t* vertex", "const int32_t* star_offsets", "const int32_t* star", "const uint8_t* vert_flags", "float* out",
                  "int64_t* summary", "void* work", "size_t work_bytes", "void* stream"):
        assert piece in call, piece
    assert len(call.split(",")) == 15
    assert " ".join(protos["ezrt_subdivide_work_bytes"][1].split()) == "int n_rows, int mode"
    assert re.search(r"#define EZRT_SUBDIVIDE_MIDPOINT 0\b", _header()) and re.search(r"#define EZRT_SUBDIVIDE_LOOP 1\b", _header())
    assert (_abi.SUBDIVIDE_MIDPOINT, _abi.SUBDIVIDE_LOOP) == (0, 1)


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("S1  Output shape", "S2  Midpoint mode", "S3  Loop edge rule", "S4  Usable corner", "S5  Smooth vertex", "S6  Border vertex",
                 "S7  Kept vertex", "S8  Loop normals", "S9  Summary"):
        assert " * " + rule in text, rule
    text = re.sub(r"\s*\n \*\s*", " ", text)                                   # the comment as running text
    for word in ("STATED LIMIT", "What follows from S1 .. S9", "How it is computed", "on the bits", "no contraction", "not renormalised",
                 "48 n_rows + 8", "out overlapping tri36", "INT32_MAX / 12", "n_rows == 0 returns 0 and launches nothing",
                 "0.375f * (a + b) + 0.125f * (c + d)", "(1.0f - (float)k * beta) * p + (beta * 0.5f) * S", "0.75f * p + 0.125f * B",
                 "0.1875f", "16-byte aligned", "no grid-wide barrier", "ezrt_vertex_normals_device", "[1] + [2] + [3] = [4] + [5] = 3 n_rows",
                 "4 F triangles, 2 E + 3 F edges and V + E vertices", "Measured on one MI355X", "No floating-point atomics"):
        assert word in text, word


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_subdivide_rows_host                                           # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "SUBDIVIDE_ABI"]
    assert len(tables) >= 27 and "CLIP_ABI" in tables and "WELD_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_subdivide_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 63, 64, 65, 4096, 4097, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 12, 2 ** 31 - 1]
    for mode in (_abi.SUBDIVIDE_MIDPOINT, _abi.SUBDIVIDE_LOOP):
        got = [f(n, mode) for n in ns]
        assert got == [f(n, mode) for n in ns]                                 # pure
        assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8
        assert all(g % 8 == 0 for g in got)
        assert all(f(n + 1, mode) >= f(n, mode) for n in range(1, 3000))
    assert all(f(n, _abi.SUBDIVIDE_MIDPOINT) == 8 for n in ns)
    for n in (1, 2, 63, 64, 65, 4097, 10 ** 6, (2 ** 31 - 1) // 12):          # four words per possible vertex, and eight bytes
        assert f(n, _abi.SUBDIVIDE_LOOP) == 48 * n + 8, n
    assert f(5, 2) == f(5, -1) == 8                                            # a mode that the call rejects needs nothing


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.SubdivRows._fields == ("rows", "summary", "n_rows")
    for bad in (0, 1, None, "Loop", "smooth"):
        with pytest.raises(ValueError, match="mode"):
            query.subdivide_rows(None, torch.zeros((4, 36)), mode=bad)
    with pytest.raises(TypeError, match="trace.Scene"):
        query.subdivide_rows(None, torch.zeros((4, 36)))

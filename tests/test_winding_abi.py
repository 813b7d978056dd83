"""The C ABI of the winding-number queries (include/ezrt_winding.h) against its ctypes table (ezrt_amd/_abi.py: WINDING_ABI): the
header's names are the table's, no other table declares them, and the library binds them with the table's argument types.  Needs no
GPU: the library is only opened, and the one function called (ezrt_winding_chunks) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_query_winding_device", "ezrt_winding_at_device", "ezrt_winding_chunks"]


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_winding.h")).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.WINDING_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.WINDING_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name                           # (int64_t* fixed is a pointer like the others)
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is C.c_int
    assert "int64_t* fixed" in protos["ezrt_query_winding_device"] and "int64_t* fixed" in protos["ezrt_winding_at_device"]


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_query_winding_host                                            # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "WINDING_ABI"]
    assert len(tables) >= 20 and "OBB_OVERLAP_ABI" in tables and "INSIDE_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_the_chunk_rule_is_a_pure_function():
    """one slice where the points alone give 8192 waves of 64, otherwise enough slices to reach that, none below 256 triangles"""
    f = _abi.load_hip().ezrt_winding_chunks
    assert f(8192 * 64, 70000) == 1 and f(8192 * 64 - 64, 70000) == 2 and f(10 ** 9, 70000) == 1
    assert f(1000, 70000) == 70000 // 256 and f(1, 70000) == 70000 // 256 and f(64, 2 ** 24) == 8192 and f(65, 2 ** 24) == 4096
    assert f(64 * 1024, 70000) == 8 and f(64 * 1024 + 1, 70000) == 8 and f(64 * 1171, 70000) == 7
    assert f(1000, 511) == 1 and f(1000, 512) == 2 and f(1000, 0) == 1 and f(0, 1000) == 1 and f(1, 255) == 1
    assert [f(1000, 70000) for _ in range(3)] == [273] * 3


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    pts = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.winding_number(None, pts)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.winding_number_at(None, pts, torch.zeros(4, dtype=torch.int32))
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="chunks"):
            query.winding_number(None, pts, chunks=bad)

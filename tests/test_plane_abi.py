"""The C ABI of the plane queries (include/ezrt_plane.h) against its ctypes table (ezrt_amd/_abi.py: PLANE_ABI): the header's names
are the table's, no other table declares them, and the library binds them with the table's argument types.  Needs no GPU: the
library is only opened, and the one function called (ezrt_plane_slices) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_plane_section_at_device", "ezrt_plane_slices", "ezrt_query_plane_count_device", "ezrt_query_plane_section_device"]


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_plane.h")).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.PLANE_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.PLANE_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is C.c_int
    assert "int64_t* offsets" in protos["ezrt_query_plane_count_device"] and "int64_t capacity" in protos["ezrt_query_plane_section_device"]
    assert "int8_t* side" in protos["ezrt_plane_section_at_device"] and "int32_t* part" in protos["ezrt_query_plane_count_device"]


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_query_plane_host                                              # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "PLANE_ABI"]
    assert len(tables) >= 21 and "WINDING_ABI" in tables and "INSIDE_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_the_slice_rule_is_a_pure_function():
    """forced: clamped to ceil(n_tri / 64) and 4096; chosen: one slice where the tiles of 64 planes alone give 16384 waves, otherwise
    enough slices to reach that, none below 256 triangles"""
    f = _abi.load_hip().ezrt_plane_slices
    assert f(10, 1000, 1) == 1 and f(10, 1000, 7) == 7 and f(10, 1000, 16) == 16 and f(10, 1000, 17) == 16 and f(10, 1024, 17) == 16
    assert f(10, 1025, 17) == 17 and f(1, 10 ** 6, 10 ** 6) == 4096 and f(1, 2 ** 24, 2 ** 31 - 1) == 4096 and f(1, 64 * 4095, 10 ** 6) == 4095
    assert f(3, 0, 5) == 1 and f(0, 1000, 5) == 5 and f(3, 1, 5) == 1 and f(3, 64, 2) == 1 and f(3, 65, 2) == 2
    assert f(1, 79820, 0) == 79820 // 256 and f(64, 79820, 0) == 311 and f(1000, 79820, 0) == 311 and f(64 * 100, 79820, 0) == 164
    assert f(10000, 79820, 0) == 105 and f(64 * 16384, 79820, 0) == 1 and f(64 * 16383 + 1, 79820, 0) == 1 and f(64 * 16383, 79820, 0) == 2
    assert f(10 ** 9, 79820, 0) == 1 and f(1, 10 ** 6, 0) == 10 ** 6 // 256 and f(1, 2 ** 24, 0) == 4096 and f(10000, 10 ** 6, 0) == 105
    assert f(1000, 10 ** 6, 0) == 1024
    assert f(1, 255, 0) == 1 and f(1, 511, 0) == 1 and f(1, 512, 0) == 2 and f(0, 1000, 0) == 1 and f(5, 0, 0) == 1 and f(-1, -1, -1) == 1
    assert [f(100000, 79820, 0) for _ in range(3)] == [11] * 3


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    planes = torch.zeros((4, 4), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.plane_count(None, planes)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.plane_section(None, planes)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.plane_section_at(None, planes, torch.zeros(4, dtype=torch.int32))
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="slices"):
            query.plane_count(None, planes, slices=bad)
        with pytest.raises(ValueError, match="slices"):
            query.plane_section(None, planes, slices=bad)

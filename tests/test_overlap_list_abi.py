"""The C ABI of the overlap lists (include/ezrt_overlap_list.h) against its ctypes table (ezrt_amd/_abi.py: OVERLAP_LIST_ABI): the
header's names are the table's, no other table declares them, the library binds them with the table's argument types, and the
limits the library reports are inside what the header promises.  Needs no GPU: the library is only opened, and the one function
called (ezrt_overlap_list_limits) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = ["ezrt_query_box_overlap_list_device", "ezrt_query_capsule_overlap_list_device", "ezrt_query_obb_overlap_list_device",
         "ezrt_query_self_overlap_list_device", "ezrt_query_tri_overlap_list_device"]
NAMES = sorted(FILLS + ["ezrt_overlap_list_limits", "ezrt_overlap_offsets_device"])


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_overlap_list.h")).read(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.OVERLAP_LIST_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (res_c, params) in protos.items():
        res, args = _abi.OVERLAP_LIST_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert res is (C.c_int if res_c == "int" else None) and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    assert protos["ezrt_overlap_list_limits"][0] == "void"
    for name in FILLS:                                                         # one tail for the five: the LIST of the header
        tail = [" ".join(p.split()) for p in protos[name][1].split(",")][-5:]
        assert tail == ["const int64_t* offsets", "int64_t capacity", "int32_t* tri_id", "int32_t* n_found", "void* stream"], name
    assert "int64_t* offsets" in protos["ezrt_overlap_offsets_device"][1] and "const int32_t* n_overlap" in protos["ezrt_overlap_offsets_device"][1]


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_query_plane_overlap_list_device                               # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "OVERLAP_LIST_ABI"]
    assert len(tables) >= 22 and "PLANE_ABI" in tables and "BOX_OVERLAP_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_the_limits_are_inside_the_header_s_promise():
    insert_max, tile_max = _abi.overlap_list_limits()
    assert 0 <= insert_max <= 64 < tile_max
    assert tile_max * 4 <= 64 * 1024 and tile_max & (tile_max - 1) == 0       # the ids of a tile fit the LDS of a launch without opt-in
    assert [_abi.overlap_list_limits() for _ in range(3)] == [(insert_max, tile_max)] * 3
    a = C.c_int(-1)
    lib = _abi.load_hip()
    lib.ezrt_overlap_list_limits(C.byref(a), None)                             # either pointer may be NULL
    assert a.value == insert_max
    lib.ezrt_overlap_list_limits(None, C.byref(a))
    assert a.value == tile_max


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    lo = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.box_overlap_list(None, lo, lo)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.obb_overlap_list(None, lo, torch.zeros((4, 3, 3)))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_overlap_list(None, torch.zeros((4, 9)))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.capsule_overlap_list(None, torch.zeros((4, 6)), torch.zeros(4))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.self_overlap_list(None, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="trace.Scene"):
        query.self_overlap_list(None)
    assert query.OverlapList._fields == ("offsets", "tri", "n_found")

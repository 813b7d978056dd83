"""The C ABI of the oriented-box queries (include/ezrt_obb_overlap.h) against its ctypes table (ezrt_amd/_abi.py: OBB_OVERLAP_ABI):
the header's names are the table's, no other table declares them, and the library binds them with the table's argument types.  Needs
no GPU: the library is only opened."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_obb_overlap_at_device", "ezrt_query_obb_overlap_device"]


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_obb_overlap.h")).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.OBB_OVERLAP_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.OBB_OVERLAP_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is C.c_int


def test_the_signatures_are_box_overlaps():
    """centre3 and axes9 stand where box_lo3 and box_hi3 stand: the same argument lists"""
    pairs = (("ezrt_query_obb_overlap_device", "ezrt_query_box_overlap_device"), ("ezrt_obb_overlap_at_device", "ezrt_box_overlap_at_device"))
    for obb, box in pairs:
        assert _abi.OBB_OVERLAP_ABI[obb] == _abi.BOX_OVERLAP_ABI[box]


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_query_obb_overlap_host                                        # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "OBB_OVERLAP_ABI"]
    assert len(tables) >= 19 and "SEGMENT_ABI" in tables and "BOX_OVERLAP_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_the_row_limit_is_the_headers():
    src = open(os.path.join(ROOT, "include", "ezrt_obb_overlap.h")).read()
    assert int(re.search(r"#define\s+EZRT_OBB_OVERLAP_MAX\s+(\d+)", src).group(1)) == _abi.OBB_OVERLAP_MAX == 64


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.ObbOverlap._fields == ("tri", "n_overlap")
    centre, axes = torch.zeros((4, 3), dtype=torch.float32), torch.zeros((4, 3, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.obb_overlap(None, centre, axes)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.obb_overlap_at(None, centre, axes, torch.zeros(4, dtype=torch.int32))
    for bad in (-1, 65, 8.0, True):
        with pytest.raises(ValueError, match="max_k"):
            query.obb_overlap(None, centre, axes, max_k=bad)
    with pytest.raises(ValueError, match="count=True"):
        query.obb_overlap(None, centre, axes, max_k=0)

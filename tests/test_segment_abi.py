"""The C ABI of the segment queries (include/ezrt_segment.h) against its ctypes table (ezrt_amd/_abi.py: SEGMENT_ABI):
the header's names are the table's, no other table declares them, and the library binds them with the table's argument types.  Needs
no GPU: the library is only opened."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_query_capsule_overlap_device", "ezrt_query_segment_distance_device", "ezrt_segment_distance_at_device"]


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_segment.h")).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.SEGMENT_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.SEGMENT_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is C.c_int


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "SEGMENT_ABI"]
    assert len(tables) >= 18 and "SPHERE_CAST_ABI" in tables and "TRI_DISTANCE_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_the_row_limit_is_the_headers():
    src = open(os.path.join(ROOT, "include", "ezrt_segment.h")).read()
    assert int(re.search(r"#define\s+EZRT_CAPSULE_OVERLAP_MAX\s+(\d+)", src).group(1)) == _abi.CAPSULE_OVERLAP_MAX == 64


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.SegmentDistance._fields == ("tri", "dist", "point_query", "point_scene", "crosses")
    assert query.CapsuleOverlap._fields == ("tri", "n_overlap")
    segs = torch.zeros((4, 6), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.segment_distance(None, segs)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.segment_distance_at(None, segs, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.capsule_overlap(None, segs, torch.zeros(4))
    for bad in (-1, 65, 8.0, True):
        with pytest.raises(ValueError, match="max_k"):
            query.capsule_overlap(None, segs, torch.zeros(4), max_k=bad)
    with pytest.raises(ValueError, match="count=True"):
        query.capsule_overlap(None, segs, torch.zeros(4), max_k=0)

"""The C ABI of the sphere-cast queries (include/ezrt_sphere_cast.h) against its ctypes table (ezrt_amd/_abi.py: SPHERE_CAST_ABI):
the header's names are the table's, no other table declares them, and the library binds them with the table's argument types.  Needs
no GPU: the library is only opened."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_query_sphere_cast_device", "ezrt_sphere_cast_at_device"]


def _protos():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ezrt_sphere_cast.h")).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.SPHERE_CAST_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.SPHERE_CAST_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is C.c_int


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "SPHERE_CAST_ABI"]
    assert len(tables) >= 17 and "TRI_DISTANCE_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_wrapper_checks_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.SphereCast._fields == ("tri", "t", "point", "touching")
    with pytest.raises(TypeError, match="GPU tensor"):
        query.sphere_cast(None, torch.zeros((4, 6), dtype=torch.float32), torch.zeros(4))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.sphere_cast_at(None, torch.zeros((4, 6), dtype=torch.float32), torch.zeros(4), torch.zeros(4, dtype=torch.int32))

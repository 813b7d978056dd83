"""The stream-ordered surface query ABI (include/ezrt_surface.h) is declared, bound and exported (dlopen only, no compute call)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ezrt_[a-z0-9_]+)\s*\(", src)))


def test_surface_binding_table_matches_header():
    from ezrt_amd import _abi
    names = _declared("ezrt_surface.h")
    assert names == ["ezrt_query_surface_device"]
    assert set(names) == set(_abi.SURFACE_ABI)
    assert not set(names) & set(_abi.TRACE_ABI)          # ezrt.h (and with it the oracle's ABI) is unchanged
    assert not set(names) & set(_abi.QUERY_ABI)          # ezrt_query.h is unchanged
    # s, rays, t_max, n_rays, integrator, tri_id, t_hit, hit_point, normal, inside, stream
    res, args = _abi.SURFACE_ABI["ezrt_query_surface_device"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6


def test_hip_library_exports_the_surface_entry_point():
    from ezrt_amd import _abi
    hip = _abi.load_hip()  # dlopen only
    for n in _declared("ezrt_surface.h"):
        assert hasattr(hip, n), n
        assert getattr(hip, n).argtypes == _abi.SURFACE_ABI[n][1]
        assert getattr(hip, n).restype is C.c_int


def test_surface_module_function():
    from ezrt_amd import query
    assert callable(query.surface)
    assert query.Surface._fields == ("tri", "t", "point", "normal", "inside")

"""The stream-ordered path query ABI (include/ezrt_path.h) is declared, bound and exported (dlopen only, no compute call)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p
# name -> argtypes, written out from the header's prototypes
WANT = {
    "ezrt_camera_rays_device": [P, P, P, C.c_int, P, P],                              # s, p, sample_xyf, n, rays_od6, stream
    "ezrt_query_radiance_device": [P, C.c_int, C.c_int, C.c_float, P, P, C.c_int, P, P],  # s, integrator, max_bounce, env_clamp,
                                                                                      # rays_od6, sample_xyf, n, radiance, stream
}
OTHER_HEADERS = ("ezrt.h", "ezrt_query.h", "ezrt_surface.h", "ezrt_shade.h", "ezrt_refit.h", "ezrt_build.h", "ezrt_mgpu.h", "ezrt_tiles.h",
                 "ezrt_scene_c.h")
OTHER_TABLES = ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI")


def _header(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared(header):
    return sorted(set(re.findall(r"\b(ezrt_[a-z0-9_]+)\s*\(", _header(header))))


def _ctype(param):
    """The ctypes type of one parameter of a prototype: every pointer is an address, the scalars are int and float."""
    if "*" in param:
        return P
    return {"int": C.c_int, "float": C.c_float}[param.split()[0]]


def test_path_binding_table_matches_header():
    from ezrt_amd import _abi
    names = _declared("ezrt_path.h")
    assert names == sorted(WANT)
    assert set(names) == set(_abi.PATH_ABI)
    for other in OTHER_TABLES:
        assert not set(names) & set(getattr(_abi, other)), other
    for h in OTHER_HEADERS:                                                           # no other header declares them
        assert not set(names) & set(_declared(h)), h
    # the table equals the prototypes, parameter by parameter
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header("ezrt_path.h")))
    assert sorted(protos) == names
    for n in names:
        res, args = _abi.PATH_ABI[n]
        assert res is C.c_int
        assert args == WANT[n], n
        assert args == [_ctype(p.strip()) for p in protos[n].split(",")], n


def test_hip_library_exports_the_path_entry_points():
    from ezrt_amd import _abi
    hip = _abi.load_hip()  # dlopen only; load_hip declares the table with the other device tables
    for n in _declared("ezrt_path.h"):
        assert hasattr(hip, n), n
        assert getattr(hip, n).argtypes == _abi.PATH_ABI[n][1]
        assert getattr(hip, n).restype is C.c_int


def test_path_module_functions():
    import inspect

    from ezrt_amd import _abi, path, query, shade
    par = inspect.signature(path.camera_rays).parameters
    assert list(par) == ["scene", "params", "xyf", "stream"] and par["stream"].default is None
    par = inspect.signature(path.radiance).parameters
    assert list(par) == ["scene", "rays", "xyf", "integrator", "max_bounce", "env_clamp", "stream"]
    assert par["integrator"].default == _abi.INTEGRATOR_P5_MIS == 51
    assert par["max_bounce"].default == 2 and par["env_clamp"].default == 0.0 and par["stream"].default is None
    # the stream and allocator handling is query.py's own and the tensor checks are shade.py's, not copies
    assert path._OnStream is query._OnStream
    assert path._tensor is shade._tensor

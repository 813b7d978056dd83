"""The stream-ordered shading query ABI (include/ezrt_shade.h) is declared, bound and exported (dlopen only, no compute call)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p
# name -> argtypes, written out from the header's prototypes
WANT = {
    "ezrt_query_material_device": [P, P, C.c_int, P, P],                        # s, tri_id, n, mat18, stream
    "ezrt_shade_eval_device": [P, C.c_int, P, P, P, P, C.c_int, P, P, P],       # s, integrator, tri_id, V, N, L, n, f_r, pdf, stream
    "ezrt_shade_sample_device": [P, C.c_int, P, P, P, P, C.c_int, P, P],        # s, integrator, tri_id, xi, V, N, n, L, stream
    "ezrt_env_eval_device": [P, P, C.c_int, C.c_float, P, P, P],                # s, L, n, env_clamp, colour, pdf, stream
    "ezrt_env_sample_device": [P, P, C.c_int, P, P],                            # s, xi, n, L, stream
}


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


def test_shade_binding_table_matches_header():
    from ezrt_amd import _abi
    names = _declared("ezrt_shade.h")
    assert names == sorted(WANT)
    assert set(names) == set(_abi.SHADE_ABI)
    for other in ("TRACE_ABI", "QUERY_ABI", "SURFACE_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(names) & set(getattr(_abi, other)), other
    for h in ("ezrt.h", "ezrt_query.h", "ezrt_surface.h"):                      # the older headers declare none of them
        assert not set(names) & set(_declared(h)), h
    # the table equals the prototypes, parameter by parameter
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header("ezrt_shade.h")))
    assert sorted(protos) == names
    for n in names:
        res, args = _abi.SHADE_ABI[n]
        assert res is C.c_int
        assert args == WANT[n], n
        assert args == [_ctype(p.strip()) for p in protos[n].split(",")], n


def test_hip_library_exports_the_shade_entry_points():
    from ezrt_amd import _abi
    hip = _abi.load_hip()  # dlopen only
    for n in _declared("ezrt_shade.h"):
        assert hasattr(hip, n), n
        assert getattr(hip, n).argtypes == _abi.SHADE_ABI[n][1]
        assert getattr(hip, n).restype is C.c_int


def test_shade_module_functions():
    import inspect

    from ezrt_amd import query, shade
    for name, lead in (("material", ["scene", "tri"]), ("evaluate", ["scene", "tri", "V", "N", "L"]),
                       ("sample", ["scene", "tri", "xi", "V", "N"]), ("env_evaluate", ["scene", "L"]), ("env_sample", ["scene", "xi"])):
        par = inspect.signature(getattr(shade, name)).parameters
        assert list(par)[:len(lead)] == lead, name
        assert par["stream"].default is None, name
    assert inspect.signature(shade.evaluate).parameters["want_pdf"].default is True
    assert inspect.signature(shade.env_evaluate).parameters["env_clamp"].default == 0.0
    # the stream and allocator handling is query.py's own, not a copy
    assert shade._OnStream is query._OnStream

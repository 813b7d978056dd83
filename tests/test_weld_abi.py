"""The C ABI of the vertex weld and the smooth normals (include/ezrt_vertices.h) against its ctypes table (ezrt_amd/_abi.py: WELD_ABI):
the header's names are the table's, no other table declares them, the library binds them with the table's argument types, and the
header carries the rule.  Needs no GPU: the library is only opened, and the functions called (the two *_work_bytes) do no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_mesh_weld_at_device", "ezrt_mesh_weld_device", "ezrt_vertex_normals_device", "ezrt_vertex_normals_work_bytes", "ezrt_weld_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_vertices.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.WELD_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.WELD_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    dev = " ".join(protos["ezrt_mesh_weld_device"][1].split())
    for piece in ("EzrtScene* s", "int32_t* vertex", "int32_t* vert_corner", "int32_t* star_offsets", "int32_t* star", "int32_t* fans",
                  "uint8_t* vert_flags", "int64_t* summary", "void* work", "size_t work_bytes", "void* stream"):
        assert piece in dev, piece
    assert len(dev.split(",")) == 11
    at = " ".join(protos["ezrt_mesh_weld_at_device"][1].split())
    for piece in ("const int32_t* corner_a", "const int32_t* corner_b", "int n", "int8_t* same", "void* stream"):
        assert piece in at, piece
    assert len(at.split(",")) == 6
    nrm = " ".join(protos["ezrt_vertex_normals_device"][1].split())
    for piece in ("EzrtScene* s", "float* tri36", "int n_tri", "const int32_t* vertex", "const int32_t* star_offsets", "const int32_t* star",
                  "void* work", "size_t work_bytes", "void* stream"):
        assert piece in nrm, piece
    assert len(nrm.split(",")) == 9


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("W1  Key, live", "W2  Vertices", "W3  Stars", "W4  Incident edges", "W5  Fans", "W6  Flags", "W7  Summary", "N1  Face normal",
                 "N2  Vertex sum", "N3  Corner normals", "N4  Robustness"):
        assert rule in text, rule
    for word in ("KNOWN LIMIT", "O(k^2)", "FLAGS GROUP", "NOT TOUCHED", "CLOSED 2-MANIFOLD exactly when", "summary[1] - T[1] + T[0]", "BY VALUE",
                 "DIFFER from", "starting from +0", "No floating-point atomics".lower(), "device-scope atomics only"):
        assert word in text, word
    assert (_abi.VERTEX_BORDER, _abi.VERTEX_NONMANIFOLD_EDGE, _abi.VERTEX_PINCHED) == tuple(
        int(re.search(r"#define EZRT_VERTEX_%s (\d)" % k, text).group(1)) for k in ("BORDER", "NONMANIFOLD_EDGE", "PINCHED"))


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_mesh_weld_host                                                # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "WELD_ABI"]
    assert len(tables) >= 24 and "TOPOLOGY_ABI" in tables and "REFIT_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_are_pure_and_monotone():
    hip = _abi.load_hip()
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 5, 6, 85, 86, 1000, 8192, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3, 2 ** 31 - 1]
    for f in (hip.ezrt_weld_work_bytes, hip.ezrt_vertex_normals_work_bytes):
        got = [f(n) for n in ns]
        assert got == [f(n) for n in ns]                                       # pure
        assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] > 8
        assert all(g % 8 == 0 for g in got)
    # the weld: two int64 arrays of 3 n + 1, an int64 per scan tile of 2048 corners and one, one int a slot of the topology's table, six ints a
    # corner; the normals: three floats a triangle
    for n in (1, 2, 85, 86, 1000, 8192, 10 ** 6):
        slots = 8
        while slots < 6 * n:
            slots *= 2
        assert hip.ezrt_weld_work_bytes(n) == (16 * (3 * n + 1) + 8 * ((3 * n + 2047) // 2048 + 1) + 4 * slots + 72 * n + 7) // 8 * 8, n
        assert hip.ezrt_vertex_normals_work_bytes(n) == (12 * n + 7) // 8 * 8, n
    assert 144 * 10 ** 6 <= hip.ezrt_weld_work_bytes(10 ** 6) <= 168 * 10 ** 6 + 16   # as the header and the wrapper's docstring say


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    with pytest.raises(TypeError, match="trace.Scene"):
        query.mesh_weld(None)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.mesh_weld(None, flags=bad)
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.mesh_weld_at(None, ids, ids)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.mesh_weld_at(None, None, None)
    with pytest.raises(TypeError, match="trace.Scene"):
        query.vertex_normals(None, torch.zeros((4, 36)), None)
    with pytest.raises(ValueError, match="n_tri"):
        query.indexed_mesh(query.MeshWeld(*([torch.zeros((4, 3), dtype=torch.int32)] + [None] * 8)), torch.zeros((5, 36)))

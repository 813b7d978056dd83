"""The C ABI of the boundary loops and caps (include/ezrt_boundary.h) against its ctypes table (ezrt_amd/_abi.py: BOUNDARY_ABI): the
header's names are the table's, no other table declares them, the library binds them with the table's argument types, and the header
carries the rule.  Needs no GPU: the library is only opened, and the one function called (ezrt_boundary_work_bytes) does no device
work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_boundary_work_bytes", "ezrt_cap_rows_device", "ezrt_mesh_boundary_device"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_boundary.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.BOUNDARY_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.BOUNDARY_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    dev = " ".join(protos["ezrt_mesh_boundary_device"][1].split())
    for piece in ("EzrtScene* s", "const int32_t* twin", "const uint8_t* edge_class", "int32_t* next", "int32_t* loop", "int32_t* pos",
                  "int32_t* order", "int32_t* loop_offsets", "uint8_t* lflags", "int64_t* area2", "int64_t* summary", "void* work",
                  "size_t work_bytes", "void* stream"):
        assert piece in dev, piece
    assert len(dev.split(",")) == 14
    cap = " ".join(protos["ezrt_cap_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_tri", "const int32_t* order", "const int32_t* loop", "const int32_t* pos",
                  "const int32_t* loop_offsets", "const uint8_t* lflags", "const int64_t* summary", "float* cap", "uint8_t* cap_valid",
                  "void* stream"):
        assert piece in cap, piece
    assert len(cap.split(",")) == 12


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("B1  Inputs by value", "B2  Successor, by rotation about the end vertex", "B3  Chains", "B4  Numbering and output", "B5  Flags",
                 "B6  Scale", "B7  Area vector", "B8  Summary", "C1  Valid rows", "C2  Triangle", "C3  Normals and materials",
                 "C4  Invalid rows and limit"):
        assert rule in text, rule
    for word in ("KNOWN LIMIT", "TAKES PART", "BOUNDARY half-edge", "AREA GROUP", "EVERY LOOP IS CLOSED", "round to nearest even", "no contraction",
                 "Nothing out of bounds is read", "NOT TOUCHED", "This is Stokes", "injective", "3 n_tri steps", "FLIPPED and NONMANIFOLD edges end the walk",
                 "folded cap", "132 n_tri + 4 (n_tri mod 2) + 8 ceil(3 n_tri / 2048) + 56", "orient and rewind first", "on the bits"):
        assert word in text, word
    assert _abi.LOOP_CLOSED == int(re.search(r"#define EZRT_LOOP_CLOSED (\d)", text).group(1)) == 1


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_mesh_boundary_host                                            # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "BOUNDARY_ABI"]
    assert len(tables) >= 25 and "TOPOLOGY_ABI" in tables and "ORIENT_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_boundary_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 682, 683, 2047, 2048, 2049, 8192, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3, 2 ** 31 - 1]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] > 8
    assert all(g % 8 == 0 for g in got)
    # per half-edge four int64 (two prefix sums, the ranking's two buffers) and three ints; padding to 8; an int64 per scan tile of
    # 2048 half-edges; seven words of eight bytes
    for n in (1, 2, 3, 682, 683, 2047, 2048, 2049, 8192, 10 ** 6, (2 ** 31 - 1) // 3):
        assert f(n) == 132 * n + 4 * (n % 2) + 8 * ((3 * n + 2047) // 2048) + 56, n
    assert all(f(n + 1) > f(n) for n in range(1, 3000))                       # monotone across the parities and the tiles
    assert f(10 ** 6) < 133 * 10 ** 6                                          # 132 B per triangle, as the wrapper's docstring says


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    with pytest.raises(TypeError, match="trace.Scene"):
        query.mesh_boundary(None)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.mesh_boundary(None, area=bad)
    with pytest.raises(TypeError, match="trace.Scene"):
        query.cap_rows(None, torch.zeros((4, 36)), None)
    none = query.MeshBoundary(*([None] * 8), 0, 0, True, 0)
    with pytest.raises(TypeError, match="MeshBoundary"):
        query.boundary_points(none, torch.zeros((4, 36)))
    with pytest.raises(TypeError, match="MeshBoundary"):
        query.boundary_points(None, torch.zeros((4, 36)))
    with pytest.raises(TypeError, match="MeshBoundary"):
        query.loop_area(none)
    with pytest.raises(TypeError, match="MeshBoundary"):
        query.loop_area(none._replace(area2=torch.zeros((2, 3), dtype=torch.int64), scale=1.5))
    b = none._replace(area2=torch.tensor([[2, -4, 0], [1, 0, 3]], dtype=torch.int64), scale=-2)
    assert query.loop_area(b).tolist() == [[0.25, -0.5, 0.0], [0.125, 0.0, 0.375]]

"""The C ABI of the plane loops (include/ezrt_plane_loops.h) against its ctypes table (ezrt_amd/_abi.py: PLANE_LOOPS_ABI): the header's
names are the table's, no other table declares them, the library binds them with the table's argument types, and the header carries
the rule.  Needs no GPU: the library is only opened, and the two functions called (ezrt_plane_loops_work_bytes,
ezrt_plane_loops_limits) do no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_plane_loops_device", "ezrt_plane_loops_limits", "ezrt_plane_loops_work_bytes"]
TYPES = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_plane_loops.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.PLANE_LOOPS_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.PLANE_LOOPS_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    dev = protos["ezrt_plane_loops_device"][1]
    for piece in ("const int64_t* offsets", "const float* seg", "int64_t capacity", "int tile_rows", "int64_t* next", "int64_t* order",
                  "int64_t* plane_loops", "int64_t loop_capacity", "int64_t* loop_offsets", "uint8_t* closed", "void* work", "size_t work_bytes",
                  "void* stream"):
        assert piece in dev, piece
    assert len(dev.split(",")) == 15


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("L1  Key", "L2  Chained planes", "L3  Degenerate rows", "L4  Pairing", "L5  Chains", "L6  Numbering and output"):
        assert rule in text, rule


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_plane_loops_host                                              # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "PLANE_LOOPS_ABI"]
    assert len(tables) >= 22 and "PLANE_ABI" in tables and "OVERLAP_LIST_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_plane_loops_work_bytes
    caps = [-2 ** 62, -1, 0, 1, 2, 7, 63, 64, 65, 1000, 2 ** 20, 24_400_000, 2 ** 31, 2 ** 40]
    got = [f(c) for c in caps]
    assert got == [f(c) for c in caps]                                         # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] > 8
    assert all(g % 8 == 0 for g in got)
    # per row: the table of twice the rows (three ints a slot), eight arrays of ints, one of int64
    assert f(1000) - f(999) == 2 * 3 * 4 + 8 * 4 + 8 == 64 and f(1000) == 64 * 1000 + 8


def test_the_limits_are_stable():
    a = [_abi.plane_loops_limits() for _ in range(3)]
    assert a[0] == a[1] == a[2] and a[0] >= 64
    assert a[0] * 11 * 4 <= 64 * 1024                                          # the tile's eleven ints per row fit a launch's LDS
    _abi.load_hip().ezrt_plane_loops_limits(None)                              # a NULL pointer is ignored


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    planes = torch.zeros((4, 4), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.plane_loops(None, planes)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.plane_loops_of(None, torch.zeros(5, dtype=torch.int64), torch.zeros((3, 2, 3)))
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="tile_rows"):
            query.plane_loops(None, planes, tile_rows=bad)
        with pytest.raises(ValueError, match="tile_rows"):
            query.plane_loops_of(None, None, None, tile_rows=bad)
    with pytest.raises(ValueError, match="loop_capacity"):
        query.plane_loops_of(None, None, None, loop_capacity=-1)
    with pytest.raises(ValueError, match="capacity"):
        query.plane_loops_of(None, None, None, capacity=-1)

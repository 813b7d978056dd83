"""The C ABI of the plane clipping (include/ezrt_clip.h) against its ctypes table (ezrt_amd/_abi.py: CLIP_ABI): the header's names are
the table's, no other table declares them, the library binds them with the table's argument types, and the header carries the rule.
Needs no GPU: the library is only opened, and the one function called (ezrt_clip_work_bytes) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_clip_count_device", "ezrt_clip_rows_device", "ezrt_clip_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_clip.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.CLIP_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.CLIP_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    cnt = " ".join(protos["ezrt_clip_count_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "const float* plane4", "int64_t* offsets", "int64_t* summary", "void* work",
                  "size_t work_bytes", "void* stream"):
        assert piece in cnt, piece
    assert len(cnt.split(",")) == 9
    fill = " ".join(protos["ezrt_clip_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "const float* plane4", "const int64_t* offsets", "int64_t capacity",
                  "float* out", "int32_t* src", "int8_t* cut_edge", "void* stream"):
        assert piece in fill, piece
    assert len(fill.split(",")) == 10


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("K1  Inputs by value", "K2  Sides", "K3  Pieces per row", "K4  Points", "K5  Normals and materials of a cut piece", "K6  Order",
                 "K7  Summary", "K8  Fill trusts nothing"):
        assert " * " + rule in text, rule
    text = re.sub(r"\s*\n \*\s*", " ", text)                                   # the comment as running text
    for word in ("STATED LIMIT", "What follows from K1 .. K8", "How it is computed", "on the bits", "No contraction", "NOT renormalised",
                 "whole or not at all", "It never depends on P4's arithmetic", "8 ceil(n_rows / 2048) + 8", "out overlapping tri36", "INT32_MAX / 2",
                 "n_rows == 0 returns 0 and launches nothing", "no FLIPPED and no NONMANIFOLD edge", "which is outward", "16-byte aligned",
                 "no grid-wide barrier", "ezrt_mesh_boundary_device", "ezrt_cap_rows_device", "[1] + [2] + [3] + [4] = n_rows"):
        assert word in text, word


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_clip_rows_host                                                # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "CLIP_ABI"]
    assert len(tables) >= 26 and "BOUNDARY_ABI" in tables and "PLANE_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_clip_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 2047, 2048, 2049, 4096, 4097, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 2, 2 ** 31 - 1]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] == 16
    assert all(g % 8 == 0 for g in got)
    for n in (1, 2, 2047, 2048, 2049, 4096, 4097, 10 ** 6, (2 ** 31 - 1) // 2):   # an int64 per scan tile of 2048 rows, and their total
        assert f(n) == 8 * ((n + 2047) // 2048) + 8, n
    assert all(f(n + 1) >= f(n) for n in range(1, 5000))


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.ClipRows._fields == ("rows", "src", "cut_edge", "summary", "n_rows")
    with pytest.raises(TypeError, match="trace.Scene"):
        query.clip_rows(None, torch.zeros((4, 36)), (0, 0, 1, 0))
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.clip_rows(None, torch.zeros((4, 36)), (0, 0, 1, 0), src=bad)
    none = query.ClipRows(None, None, None, None, 0)
    with pytest.raises(TypeError, match="ClipRows"):
        query.cut_segments(none)
    with pytest.raises(TypeError, match="ClipRows"):
        query.cut_segments(None)
    with pytest.raises(TypeError, match="ClipRows"):
        query.cut_segments(none._replace(rows=torch.zeros((4, 36))))          # made with src=False: no cut_edge

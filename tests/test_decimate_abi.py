"""The C ABI of the decimation (include/ezrt_decimate.h) against its ctypes table (ezrt_amd/_abi.py: DECIMATE_ABI): the header's names
are the table's, no other table declares them, the library binds them with the table's argument types, and the header carries the
rule.  Needs no GPU: the library is only opened, the one function called with work to do (ezrt_decimate_work_bytes) does no device
work, and the calls that are rejected are rejected before any."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_decimate_count_device", "ezrt_decimate_rows_device", "ezrt_decimate_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "void": None}
EZRT_ERR_INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_decimate.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.DECIMATE_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.DECIMATE_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    cnt = " ".join(protos["ezrt_decimate_count_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "const float* grid4", "int flags", "int32_t* cell", "int32_t* cell_corner",
                  "float* cell_point", "int64_t* offsets", "int64_t* summary", "void* work", "size_t work_bytes", "void* stream"):
        assert piece in cnt, piece
    assert len(cnt.split(",")) == 13
    fill = " ".join(protos["ezrt_decimate_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "const int32_t* cell", "const float* cell_point", "const int64_t* offsets",
                  "int64_t capacity", "float* out", "int32_t* src", "void* stream"):
        assert piece in fill, piece
    assert len(fill.split(",")) == 10
    assert re.search(r"#define EZRT_DECIMATE_DEDUP 1\b", _header()) and _abi.DECIMATE_DEDUP == 1


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("D1  Grid", "D2  Fixed point", "D3  Cells", "D4  Representative point", "D5  Kept component", "D6  Survivors", "D7  Duplicates",
                 "D8  Output row", "D9  Order and summary", "D10 Fill trusts nothing"):
        assert " * " + rule in text, rule
    text = re.sub(r"\s*\n \*\s*", " ", text)                                   # the comment as running text
    for word in ("STATED LIMITS", "What follows from D1 .. D10", "How it is computed", "on the bits", "no contraction", "Measured",
                 "does not preserve manifoldness", "may round to one float value", "may round onto a face of its cell", "emitted, not filtered",
                 "whole or not at all", "belongs to the upper cell", "u = ((double)x - (double)o) / (double)h", "w = u * 16777216.0",
                 "x = (float)((double)o + ((double)i + m * 0x1p-24) * (double)h)", "[-2^44, 2^44)", "-0 as +0",
                 "40 n_rows + 8 ceil(3 n_rows / 2048) + 64 P(6 n_rows) + 4 P(2 n_rows) + 16", "out overlapping tri36", "INT32_MAX / 3",
                 "n_rows == 0 returns 0 and launches nothing", "16-byte aligned", "No floating-point atomics", "no grid-wide barrier",
                 "no workgroup waits for another", "[0] + [1] + [2] + [3] = n_rows", "Identity", "Idempotence", "KNOWN LIMIT"):
        assert word in text, word


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_decimate_rows_host                                            # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "DECIMATE_ABI"]
    assert len(tables) >= 28 and "SUBDIVIDE_ABI" in tables and "CLIP_ABI" in tables and "WELD_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def _p2(x):
    p = 8
    while p < x:
        p *= 2
    return p


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_decimate_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 4, 5, 682, 683, 2047, 2048, 2049, 4096, 4097, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3, 2 ** 31 - 1]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8
    assert all(g % 8 == 0 for g in got)
    for n in (1, 2, 3, 4, 5, 682, 683, 2047, 2048, 2049, 4096, 4097, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3):   # the header's closed formula
        assert f(n) == 40 * n + 8 * ((3 * n + 2047) // 2048) + 64 * _p2(6 * n) + 4 * _p2(2 * n) + 16, n
    assert all(f(n + 1) >= f(n) for n in range(1, 5000))
    assert all(424 * n <= f(n) for n in range(2, 5000)) and all(f(n) <= 830 * n for n in range(8, 5000))


def test_rejected_before_any_device_work():
    lib = _abi.load_hip()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.ezrt_decimate_count_device(None, p, 1, p, 1, p, p, p, p, p, p, 2 ** 20, None) == EZRT_ERR_INVALID
    assert b"NULL" in lib.ezrt_last_error()
    assert lib.ezrt_decimate_rows_device(None, p, 1, p, p, p, 1, p, p, None) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error()
    assert not any(buf)


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.DecimatedRows._fields == ("rows", "src", "cell", "cell_point", "summary", "n_rows")
    with pytest.raises(TypeError, match="trace.Scene"):
        query.decimate_rows(None, torch.zeros((4, 36)), 1.0)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.decimate_rows(None, torch.zeros((4, 36)), 1.0, src=bad)
        with pytest.raises(ValueError, match="bool"):
            query.decimate_rows(None, torch.zeros((4, 36)), 1.0, dedup=bad)
    assert "ezrt_decimate_work_bytes" in query.decimate_rows.__doc__ and "MEMORY" in query.decimate_rows.__doc__

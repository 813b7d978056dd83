"""The C ABI of the mesh smoothing (include/ezrt_smooth.h) against its ctypes tables (ezrt_amd/_abi.py: SMOOTH_ABI for the call,
SMOOTH_SIZES for ezrt_smooth_work_bytes and ezrt_smooth_limits): the header's names are the tables', no other table declares them, the
library binds them with the tables' argument types, the header carries the rule, and the size function is its formula.  Needs no GPU:
the library is only opened, and the functions called do no device work."""
import ctypes as C
import os
import re
import sys

import pytest

from ezrt_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_expected as SM  # noqa: E402
from test_mesh_work_bytes import NS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_smooth_rows_device", "ezrt_smooth_limits", "ezrt_smooth_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "float": C.c_float, "void": None}
ROW_LIMIT = (2 ** 31 - 1) // 3


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_smooth.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_tables_match_the_header():
    protos = _protos()
    table = {**_abi.SMOOTH_ABI, **_abi.SMOOTH_SIZES}
    assert sorted(_abi.SMOOTH_ABI) == NAMES[:1] and sorted(_abi.SMOOTH_SIZES) == NAMES[1:] and sorted(protos) == sorted(table) == sorted(NAMES)
    assert not any(k.endswith("_work_bytes") for k in _abi.SMOOTH_ABI)
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = table[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    call = " ".join(protos["ezrt_smooth_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* tri36", "int n_rows", "const uint8_t* edge_class", "const int32_t* vertex",
                  "const int32_t* star_offsets", "const int32_t* star", "const uint8_t* vert_flags", "int steps", "float lambda", "float mu",
                  "int flags", "int tile_rows", "float* out", "int64_t* summary", "void* work", "size_t work_bytes", "void* stream"):
        assert piece in call, piece
    assert len(call.split(",")) == 18
    assert " ".join(protos["ezrt_smooth_work_bytes"][1].split()) == "int n_rows"
    assert " ".join(protos["ezrt_smooth_limits"][1].split()) == "int* tile_rows_max"
    assert re.search(r"#define EZRT_SMOOTH_PIN_BORDER 1\b", _header()) and re.search(r"#define EZRT_SMOOTH_STEPS_MAX 1024\b", _header())
    assert (_abi.SMOOTH_PIN_BORDER, _abi.SMOOTH_STEPS_MAX) == (1, 1024) == (SM.PIN_BORDER, SM.STEPS_MAX)


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("U1  Output shape", "U2  Usable, active", "U3  State", "U4  The rule of a vertex", "U5  Weight", "U6  SMOOTH step",
                 "U7  BORDER step", "U8  KEPT, and the output", "U9  Summary"):
        assert " * " + rule in text, rule
    text = re.sub(r"\s*\n \*\s*", " ", text)                                   # the comment as running text
    for word in ("STATED LIMIT", "KNOWN LIMIT", "What follows from U1 .. U9", "How it is computed", "on the bits", "no contraction",
                 "division is IEEE", "x_{j+1} = x_j + w_j * (m - x_j)", "m = S / (float)(2 * k)", "m = B * 0.5f", "the inner sum formed first",
                 "lambda = 0.5f, mu = -0.53f", "out == tri36 exactly is allowed", "INT32_MAX / 3", "1 .. EZRT_SMOOTH_STEPS_MAX",
                 "n_rows == 0 returns 0 and launches nothing", "45 H + 8 (b + 1) + 8 (c + 1)", "ezrt_weld_work_bytes(n_rows)",
                 "[1] + [2] + [3] = 3 n_rows", "these cannot collide", "no grid-wide barrier", "No floating-point atomics", "16-byte aligned",
                 "k sequential gathers per step in one lane", "tile_rows_max", "an observation, not a rule", "Measured on one MI355X",
                 "entries of star_offsets beyond V are never looked at", "36 V + 32 K"):
        assert word in text, word


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_smooth_rows_host                                              # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.isupper() and isinstance(getattr(_abi, k), dict) and k not in ("SMOOTH_ABI", "SMOOTH_SIZES")]
    assert len(tables) >= 29 and "SUBDIVIDE_ABI" in tables and "WELD_ABI" in tables and "ISO_SIZES" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_its_formula_pure_monotone_and_within_the_welds():
    hip = _abi.load_hip()
    f, weld = hip.ezrt_smooth_work_bytes, hip.ezrt_weld_work_bytes
    ns = [-2 ** 31] + NS + [ROW_LIMIT - 1, ROW_LIMIT]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert got == [SM.work_bytes(n) for n in ns]                               # the header's formula
    assert all(b >= a for a, b in zip(got, got[1:])) and all(g % 8 == 0 for g in got)
    assert f(-2 ** 31) == f(-1) == f(0) == 8 and f(1) == 45 * 3 + 16 + 16 + 1
    assert f(2 ** 31 - 1) >= f(ROW_LIMIT)                                      # a count the call rejects: still monotone
    small = [f(n) for n in range(0, 6000)]
    assert all(b >= a for a, b in zip(small, small[1:]))
    for n in list(range(1, 6000)) + [n + d for n in NS[6:] + [ROW_LIMIT - 2] for d in (-1, 0, 1, 2)]:
        assert f(n) % 8 == 0 and f(n) <= weld(n), n                            # a buffer that served the weld of these rows serves this call
    assert 134 * 10 ** 6 < f(10 ** 6) < 136 * 10 ** 6


def test_limits():
    tile_rows_max = _abi.smooth_limits()
    assert tile_rows_max >= 64 and tile_rows_max * 72 <= 64 * 1024             # both position buffers of a tile fit one launch's LDS
    _abi.load_hip().ezrt_smooth_limits(None)                                   # a null pointer is ignored


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.SmoothRows._fields == ("rows", "summary", "n_rows")
    with pytest.raises(TypeError, match="trace.Scene"):
        query.smooth_rows(None, torch.zeros((4, 36)), None, None)

"""The C ABI of the isosurface extraction (include/ezrt_isosurface.h) against its ctypes tables (ezrt_amd/_abi.py: ISO_ABI for the two
calls, ISO_SIZES for ezrt_iso_work_bytes): the header's names are the tables', no other table declares them, the library binds them
with the tables' argument types, and the header carries the rule.  Needs no GPU: the library is only opened, the one function called
with work to do (ezrt_iso_work_bytes) does no device work, and the calls that are rejected are rejected before any."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_iso_count_device", "ezrt_iso_rows_device", "ezrt_iso_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64, "void": None}
EZRT_ERR_INVALID = -1


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_isosurface.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    table = {**_abi.ISO_ABI, **_abi.ISO_SIZES}
    assert sorted(_abi.ISO_ABI) == NAMES[:2] and sorted(_abi.ISO_SIZES) == NAMES[2:] and sorted(protos) == sorted(table) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = table[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    cnt = " ".join(protos["ezrt_iso_count_device"][1].split())
    for piece in ("EzrtScene* s", "const float* values", "int nx", "int ny", "int nz", "const float* grid8", "int64_t* offsets", "int64_t* summary",
                  "void* work", "size_t work_bytes", "void* stream"):
        assert piece in cnt, piece
    assert len(cnt.split(",")) == 11
    fill = " ".join(protos["ezrt_iso_rows_device"][1].split())
    for piece in ("EzrtScene* s", "const float* values", "int nx", "int ny", "int nz", "const float* grid8", "const float* material18",
                  "const int64_t* offsets", "int64_t capacity", "float* out", "int32_t* cell", "void* stream"):
        assert piece in fill, piece
    assert len(fill.split(",")) == 12
    assert " ".join(protos["ezrt_iso_work_bytes"][1].split()) == "int nx, int ny, int nz"
    assert re.search(r"#define EZRT_ISO_BLOCK 256\b", _header()) and _abi.ISO_BLOCK == 256


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("G1  Inputs by value", "G2  Positions", "G3  Inside", "G4  Tetrahedra", "G5  Pieces per tet", "G6  Points", "G7  Output row",
                 "G8  Order, offsets, summary", "G9  Fill trusts nothing"):
        assert " * " + rule in text, rule
    text = re.sub(r"\s*\n \*\s*", " ", text)                                   # the comment as running text
    for word in ("STATED LIMITS", "What follows from G1 .. G9", "How it is computed", "on the bits", "no contraction", "Measured",
                 "MARCHING TETRAHEDRA on the Kuhn split", "(float)((double)o_a + (double)i * (double)h_a)", "INSIDE when f < iso and OUTSIDE when f >= iso",
                 "(k (ny - 1) + j) (nx - 1) + i", "xyz, xzy, yxz, yzx, zxy, zyx", "the exchanged masks are 2, 5, 8, 10, 11, 14",
                 "(q(a,c), q(a,d), q(b,d)) then (q(a,c), q(b,d), q(b,c))", "t = ((double)iso - (double)fA) / ((double)fB - (double)fA)",
                 "(float)(pA + t * (pB - pA))", "N1 of ezrt_vertices.h", "a degenerate row gets NaN", "EZRT_ISO_BLOCK = 256",
                 "[1] + [2] + [3] = n_cells", "whole or not at all", "offsets[b + 1] - offsets[b] == c", "pads the field with one layer of outside values",
                 "A position that overflows is emitted as it is", "Adding a constant to values and iso alike, where exact, changes nothing",
                 "closed box of its cell", "8 ceil(n_blocks / 2048) + 8", "8 for no cells", "out overlapping values", "nx ny nz above INT32_MAX",
                 "a dimension < 1", "returns 0 and launches nothing", "16-byte aligned", "No floating-point atomics", "no grid-wide barrier",
                 "no workgroup waits for another", "no loop that is not bounded by a constant", "profiles/r39/iso_rates.txt"):
        assert word in text, word


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_iso_rows_host                                                 # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.isupper() and isinstance(getattr(_abi, k), dict) and k not in ("ISO_ABI", "ISO_SIZES")]
    assert len(tables) >= 29 and "DECIMATE_ABI" in tables and "CLIP_ABI" in tables and "WELD_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def _formula(nx, ny, nz):
    if min(nx, ny, nz) < 2:
        return 8
    n_blocks = ((nx - 1) * (ny - 1) * (nz - 1) + 255) // 256
    return 8 * ((n_blocks + 2047) // 2048) + 8


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_iso_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 9, 17, 65, 81, 82, 129, 257, 1025, 1290]
    got = [f(n, n, n) for n in ns]
    assert got == [f(n, n, n) for n in ns]                                     # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == got[3] == 8 and got[4] == 16
    assert all(g % 8 == 0 for g in got)
    for n in ns:
        assert f(n, n, n) == _formula(n, n, n), n
    for dims in ((1, 5, 5), (5, 5, 1), (5, 1, 5), (2, 2, 2), (2, 9, 40), (130, 66, 66), (2 ** 20, 2, 2), (2, 2, 2 ** 30 - 1), (2 ** 31 - 1, 1, 1),
                 (2 ** 15, 2 ** 15, 2), (1291, 1290, 1289), (0, 7, 7), (7, -3, 7)):
        assert f(*dims) == _formula(*dims), dims
    assert f(130, 66, 66) == 24 and f(129, 66, 66) == 24 and f(82, 81, 81) == 16   # 2130 blocks: two scan tiles; 2025 blocks: one
    for a in range(1, 40):                                                     # monotone in each dimension
        assert f(a + 1, 300, 300) >= f(a, 300, 300) and f(300, a + 1, 300) >= f(300, a, 300) and f(300, 300, a + 1) >= f(300, 300, a)


def test_rejected_before_any_device_work():
    lib = _abi.load_hip()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    cnt, fill = lib.ezrt_iso_count_device, lib.ezrt_iso_rows_device
    assert cnt(None, p, 2, 2, 2, p, p, p, p, 2 ** 20, None) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error()
    assert fill(None, p, 2, 2, 2, p, p, p, 1, p, p, None) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error()
    s = p                                                                      # not a scene: every call below fails before it is looked at
    for k in (1, 5, 6, 7, 8):                                                  # values, grid8, offsets, summary, work
        args = [s, p, 2, 2, 2, p, p, p, p, 2 ** 20, None]
        args[k] = None
        assert cnt(*args) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in (1, 5, 6, 7, 9):                                                  # values, grid8, material18, offsets, out (capacity > 0)
        args = [s, p, 2, 2, 2, p, p, p, 1, p, p, None]
        args[k] = None
        assert fill(*args) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for dims in ((0, 2, 2), (2, -1, 2), (2, 2, 0), (-2 ** 31, 2, 2)):
        assert cnt(s, p, *dims, p, p, p, p, 2 ** 20, None) == EZRT_ERR_INVALID and b"dimension < 1" in lib.ezrt_last_error(), dims
        assert fill(s, p, *dims, p, p, p, 1, p, p, None) == EZRT_ERR_INVALID and b"dimension < 1" in lib.ezrt_last_error(), dims
    for dims in ((2 ** 16, 2 ** 15, 1), (1291, 1291, 1291), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2, 1)):
        assert cnt(s, p, *dims, p, p, p, p, 2 ** 40, None) == EZRT_ERR_INVALID and b"INT32_MAX" in lib.ezrt_last_error(), dims
        assert fill(s, p, *dims, p, p, p, 1, p, p, None) == EZRT_ERR_INVALID and b"INT32_MAX" in lib.ezrt_last_error(), dims
    assert cnt(s, p, 3, 3, 3, p, p, p, p, 15, None) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert cnt(s, p, 3, 3, 3, p, p, p, C.c_void_p(p.value + 4), 64, None) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    assert fill(s, p, 3, 3, 3, p, p, p, -1, p, p, None) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert fill(s, p, 3, 3, 3, p, p, p, 2 ** 62, p, p, None) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert fill(s, p, 3, 3, 3, p, p, p, 1, p, p, None) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error()   # out is values
    assert fill(s, p, 3, 3, 3, p, p, p, 1, C.c_void_p(p.value + 104), p, None) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error()
    # a grid with a dimension of 1 has no cells: 0, and nothing is looked at
    assert cnt(s, p, 1, 5, 5, p, p, p, p, 8, None) == 0 and fill(s, p, 5, 5, 1, p, p, p, 1, p, p, None) == 0
    assert not any(buf)


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.IsoRows._fields == ("rows", "cell", "summary", "shape")
    with pytest.raises(TypeError, match="trace.Scene"):
        query.isosurface_rows(None, torch.zeros((4, 4, 4)), 0.0)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.isosurface_rows(None, torch.zeros((4, 4, 4)), 0.0, cell=bad)
    for shape in ((4, 4), (0, 4, 4), (4, 4, 4, 4), (2 ** 11, 2 ** 10, 2 ** 10)):
        with pytest.raises(ValueError, match="shape|vertices"):
            query.grid_points(shape, device="cpu")
    with pytest.raises(ValueError, match="origin"):
        query.grid_points((2, 2, 2), origin=(0, 0), device="cpu")
    with pytest.raises(ValueError, match="spacing"):
        query.grid_points((2, 2, 2), spacing=(1, 2), device="cpu")
    doc = query.isosurface_rows.__doc__
    assert "ezrt_iso_work_bytes" in doc and "MEMORY" in doc and "signed_distance" in doc and "grid_points" in query.isosurface_rows.__doc__
    assert "isosurface_rows(scene, sd.dist.reshape(shape), r, origin, spacing)" in query.grid_points.__doc__


def test_grid_points_are_g2_on_the_bits():
    """on the CPU device: the same torch operations as on a GPU"""
    torch = pytest.importorskip("torch")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import iso_expected as IE
    from ezrt_amd import query
    for shape, o, h in (((3, 4, 5), (0.1, -0.3, 2.7), (0.37, 0.11, 1.3)), ((7, 2, 9), (1e3, -1e3, 0), 1e-3), ((1, 1, 1), (0, 0, 0), 1.0)):
        got = query.grid_points(shape, o, h, device="cpu")
        want = IE.positions(shape, IE.grid8(o, h, 0.0))
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
        assert IE.bits(got.numpy()).tolist() == IE.bits(want).tolist()

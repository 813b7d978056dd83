"""The C ABI of the mesh orientation (include/ezrt_orient.h) against its ctypes table (ezrt_amd/_abi.py: ORIENT_ABI): the header's
names are the table's, no other table declares them, the library binds them with the table's argument types, and the header carries
the rule.  Needs no GPU: the library is only opened, and the one function called (ezrt_orient_work_bytes) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_mesh_orient_device", "ezrt_orient_work_bytes", "ezrt_rewind_device"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_orient.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.ORIENT_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.ORIENT_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    dev = " ".join(protos["ezrt_mesh_orient_device"][1].split())
    for piece in ("EzrtScene* s", "const int32_t* twin", "const uint8_t* edge_class", "int outward", "uint8_t* flip", "int32_t* patch_root",
                  "int32_t* patch", "int32_t* proot", "int32_t* psize", "uint8_t* pflags", "int64_t* vol6", "int64_t* summary", "void* work",
                  "size_t work_bytes", "void* stream"):
        assert piece in dev, piece
    assert len(dev.split(",")) == 15
    rw = " ".join(protos["ezrt_rewind_device"][1].split())
    for piece in ("EzrtScene* s", "float* tri36", "int n_tri", "const uint8_t* flip", "void* stream"):
        assert piece in rw, piece
    assert len(rw.split(",")) == 5


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("O1  Inputs taken by value", "O2  Links", "O3  Patches", "O4  Orientable, flip", "O5  Closed", "O6  Volume", "O7  Outward",
                 "O8  Flags and summary"):
        assert rule in text, rule
    for word in ("KNOWN LIMIT", "TAKES PART", "NONORIENTABLE", "REWOUND", "INWARD", "round to nearest even", "no contraction",
                 "Nothing out of bounds is read", "CONSISTENTLY WOUND exactly when", "Applied twice it restores the rows", "NOT TOUCHED"):
        assert word in text, word
    assert (_abi.PATCH_OPEN, _abi.PATCH_NONORIENTABLE, _abi.PATCH_REWOUND, _abi.PATCH_INWARD) == tuple(
        int(re.search(r"#define EZRT_PATCH_%s (\d)" % k, text).group(1)) for k in ("OPEN", "NONORIENTABLE", "REWOUND", "INWARD")) == (1, 2, 4, 8)


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_mesh_orient_host                                              # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "ORIENT_ABI"]
    assert len(tables) >= 24 and "TOPOLOGY_ABI" in tables and "WELD_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_orient_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 2047, 2048, 2049, 8192, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3, 2 ** 31 - 1]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] > 8
    assert all(g % 8 == 0 for g in got)
    # per triangle two int64 (the number, the volume) and four ints; an int64 per scan tile of 2048; three words of eight bytes
    for n in (1, 2, 2047, 2048, 2049, 8192, 10 ** 6, (2 ** 31 - 1) // 3):
        assert f(n) == 32 * n + 8 * ((n + 2047) // 2048) + 24, n
    assert f(10 ** 6) < 33 * 10 ** 6                                           # 32 B per triangle, as the wrapper's docstring says


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    with pytest.raises(TypeError, match="trace.Scene"):
        query.mesh_orient(None)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bool"):
            query.mesh_orient(None, outward=bad)
    with pytest.raises(TypeError, match="trace.Scene"):
        query.rewind(None, torch.zeros((4, 36)), None)
    with pytest.raises(TypeError, match="MeshOrient"):
        query.patch_volume(query.MeshOrient(None, None, None, None, None, None, None, None, 0, True, 0))
    with pytest.raises(TypeError, match="MeshOrient"):
        query.patch_volume(query.MeshOrient(None, None, None, None, None, None, torch.zeros(2, dtype=torch.int64), None, 2, True, 1.5))
    o = query.MeshOrient(None, None, None, None, None, None, torch.tensor([6, -12], dtype=torch.int64), None, 2, True, -3)
    assert query.patch_volume(o).tolist() == [0.125, -0.25]

"""The C ABI of the mesh topology (include/ezrt_topology.h) against its ctypes table (ezrt_amd/_abi.py: TOPOLOGY_ABI): the header's
names are the table's, no other table declares them, the library binds them with the table's argument types, and the header carries
the rule.  Needs no GPU: the library is only opened, and the one function called (ezrt_topology_work_bytes) does no device work."""
import ctypes as C
import os
import re

import pytest

from ezrt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ezrt_mesh_topology_at_device", "ezrt_mesh_topology_device", "ezrt_topology_work_bytes"]
TYPES = {"int": C.c_int, "size_t": C.c_size_t, "void": None}


def _header():
    return open(os.path.join(ROOT, "include", "ezrt_topology.h")).read()


def _protos():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t|void)\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_binding_table_matches_the_header():
    protos = _protos()
    assert sorted(protos) == sorted(_abi.TOPOLOGY_ABI) == NAMES
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (ret, params) in protos.items():
        res, args = _abi.TOPOLOGY_ABI[name]
        want = [C.c_void_p if "*" in p else TYPES[p.split()[0]] for p in params.split(",")]
        assert res is TYPES[ret] and args == want, name
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res
    dev = " ".join(protos["ezrt_mesh_topology_device"][1].split())
    for piece in ("EzrtScene* s", "int32_t* twin", "uint8_t* edge_class", "int32_t* mult", "int32_t* root", "int32_t* component",
                  "int32_t* comp_root", "int32_t* comp_size", "uint8_t* comp_flags", "int64_t* summary", "void* work", "size_t work_bytes",
                  "void* stream"):
        assert piece in dev, piece
    assert len(dev.split(",")) == 13
    at = " ".join(protos["ezrt_mesh_topology_at_device"][1].split())
    for piece in ("const int32_t* tri_a", "const int32_t* edge_a", "const int32_t* tri_b", "int n", "int8_t* shared", "int8_t* opposite", "void* stream"):
        assert piece in at, piece
    assert len(at.split(",")) == 8


def test_the_header_carries_the_rule():
    text = _header()
    for rule in ("M1  Vertex key", "M2  TOPO-live", "M3  Half-edges and edges", "M4  Class", "M5  Twin", "M6  Components", "M7  Summary"):
        assert rule in text, rule
    for word in ("BOUNDARY", "MANIFOLD", "FLIPPED", "NONMANIFOLD", "WIDER than the LIVE of ezrt_tri_overlap.h", "after a refit", "CLOSED exactly when",
                 "CONSISTENTLY WOUND exactly when", "KNOWN LIMIT"):
        assert word in text, word
    assert (_abi.EDGE_BOUNDARY, _abi.EDGE_MANIFOLD, _abi.EDGE_FLIPPED, _abi.EDGE_NONMANIFOLD) == tuple(
        int(re.search(r"#define EZRT_EDGE_%s (\d)" % k, text).group(1)) for k in ("BOUNDARY", "MANIFOLD", "FLIPPED", "NONMANIFOLD"))


def test_the_library_exports_the_symbols():
    lib = C.CDLL(os.path.join(_abi.LIB_DIR, "libezrt_hip.so"))                 # a handle of its own, nothing declared on it
    for name in NAMES:
        assert getattr(lib, name) is not None, name
    with pytest.raises(AttributeError):
        lib.ezrt_mesh_topology_host                                            # (a name that is not exported raises)


def test_names_are_in_no_other_table():
    tables = [k for k in dir(_abi) if k.endswith("_ABI") and isinstance(getattr(_abi, k), dict) and k != "TOPOLOGY_ABI"]
    assert len(tables) >= 23 and "PLANE_LOOPS_ABI" in tables and "OVERLAP_LIST_ABI" in tables and "TRACE_ABI" in tables
    for other in tables:
        assert not set(NAMES) & set(getattr(_abi, other)), other


def test_work_bytes_is_pure_and_monotone():
    f = _abi.load_hip().ezrt_topology_work_bytes
    ns = [-2 ** 31, -1, 0, 1, 2, 3, 5, 6, 85, 86, 1000, 8192, 10 ** 6, 2 ** 24, (2 ** 31 - 1) // 3, 2 ** 31 - 1]
    got = [f(n) for n in ns]
    assert got == [f(n) for n in ns]                                           # pure
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] == got[1] == got[2] == 8 and got[3] > 8
    assert all(g % 8 == 0 for g in got)
    # the table: two ints a slot, the next power of two of at least 6 n_tri slots (8 at the least); per triangle 9 ints and an int64
    for n in (1, 2, 85, 86, 1000, 8192, 10 ** 6):
        slots = 8
        while slots < 6 * n:
            slots *= 2
        assert f(n) == (8 * (n + 1) + 8 * slots + 36 * n + 7) // 8 * 8, n
    assert f(10 ** 6) < 120 * 10 ** 6                                          # about 100 B per triangle, as the wrapper's docstring says


def test_wrappers_check_before_any_library_call():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    with pytest.raises(TypeError, match="trace.Scene"):
        query.mesh_topology(None)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="bools"):
            query.mesh_topology(None, components=bad)
        with pytest.raises(ValueError, match="bools"):
            query.mesh_topology(None, mult=bad)
    ids = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.mesh_topology_at(None, ids, ids, ids)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.mesh_topology_at(None, None, None, None)

"""The stream-ordered query ABI (include/ezrt_query.h) is declared, bound and exported (dlopen only, no compute call)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ezrt_[a-z0-9_]+)\s*\(", src)))


def test_query_binding_table_matches_header():
    from ezrt_amd import _abi
    names = _declared("ezrt_query.h")
    assert names == ["ezrt_query_closest_device", "ezrt_query_occluded_device"]
    assert set(names) == set(_abi.QUERY_ABI)
    assert not set(names) & set(_abi.TRACE_ABI)          # ezrt.h (and with it the oracle's ABI) is unchanged


def test_hip_library_exports_the_query_entry_points():
    from ezrt_amd import _abi
    hip = _abi.load_hip()  # dlopen only
    for n in _declared("ezrt_query.h"):
        assert hasattr(hip, n), n
        assert getattr(hip, n).argtypes == _abi.QUERY_ABI[n][1]


def test_query_module_imports():
    from ezrt_amd import query
    assert callable(query.closest) and callable(query.occluded)

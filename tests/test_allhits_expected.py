"""The yardstick of the all-hits tests pinned to the CPU oracle before the device is compared with it, and the argument errors of the
binding that need no device (include/ezrt_multihit.h, ezrt_amd/query.py).

tests/allhits_expected.py restates "all hits of a ray" on the oracle's hitAABB and hitTriangle tables.  Here, on the scenes and rays
tests/test_gpu_allhits.py uses: slot 0 of its lists is ezrt_query_hits of the oracle on the bits for every ray (the closest hit is
the first-visited triangle of the smallest t), the lists are sorted, and the ray mix meets the conditions the device test rests on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_expected as E  # noqa: E402
import allhits_scenes as A  # noqa: E402

_cache = {}


def _lists(name, oracle, bunny_small):
    if name not in _cache:
        tri, nodes, rays = A.scene(name, bunny_small)
        visits = E.visit_lists(oracle, tri, nodes, rays)
        _cache[name] = (tri, nodes, rays, visits, E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits))
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", A.SCENES)
def test_slot_0_is_the_oracles_closest_hit(oracle, bunny_small, name):
    tri, nodes, rays, visits, lists = _lists(name, oracle, bunny_small)
    to, do = oracle.scene_create(tri, nodes).query_hits(rays)
    wt, wd, count = E.rows(lists, 1)
    assert 0.05 < (to >= 0).mean() < 0.95
    assert np.array_equal(wt[:, 0], to), "%d triangle ids differ" % int((wt[:, 0] != to).sum())
    assert np.array_equal(_bits(wd[:, 0]), _bits(do))
    assert np.array_equal(count > 0, to >= 0)
    for ids, t in lists:
        assert np.all(t[1:] >= t[:-1]) and np.all(t >= np.float32(0.0005)) and np.all(t < E.EZ_INF)
    # with a bound: the oracle's hit where it lies below it
    rng = np.random.default_rng(5)
    t_max = rng.uniform(0.0, 8.0, rays.shape[0]).astype(np.float32)
    t_max[::17] = np.nan
    t_max[1::17] = np.inf
    bt, bd, bc = E.rows(E.expected_all_hits(oracle, tri, nodes, rays, t_max, visits=visits), 1)
    with np.errstate(invalid="ignore"):
        hit = (to >= 0) & (do < t_max)
    assert np.array_equal(bt[:, 0], np.where(hit, to, -1))
    assert np.array_equal(_bits(bd[:, 0]), _bits(np.where(hit, do, E.EZ_INF)))
    assert np.array_equal(bc > 0, hit)
    if name != "not_nested":                                       # (a leaf with two parents is visited twice)
        assert all(np.unique(ids).size == ids.size for ids, t in lists)


def test_the_tie_scene_is_not_vacuous(oracle, bunny_small):
    """What the truncation and tie checks of the device test rest on, decided by the reference's values alone."""
    tri, nodes, rays, visits, lists = _lists("ties", oracle, bunny_small)
    count = np.array([ids.size for ids, t in lists])
    assert (count >= 2).mean() >= 0.25
    assert (count > 5).mean() >= 0.05
    assert (count == 0).mean() >= 0.05
    K = 2
    assert any(t.size > K and t[K - 1] == t[K] for ids, t in lists)           # an exact tie straddling position K


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    cpu_rays = torch.zeros((4, 6), dtype=torch.float32)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_hits"):
            query.all_hits(None, cpu_rays, bad)
    with pytest.raises(TypeError, match="GPU tensor"):                        # as query.closest: CPU tensors are refused
        query.all_hits(None, cpu_rays, 4)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.surface_at(None, cpu_rays, torch.zeros(4, dtype=torch.int32), torch.zeros(4))
    with pytest.raises(TypeError):
        query.closest(None, cpu_rays)


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ezrt_multihit.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.MULTIHIT_ABI) == ["ezrt_query_all_hits_device", "ezrt_surface_at_device"]
    assert int(re.search(r"#define\s+EZRT_ALL_HITS_MAX\s+(\d+)", src).group(1)) == _abi.ALL_HITS_MAX == 64
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.MULTIHIT_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other

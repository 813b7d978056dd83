"""tests/build_edge_scenes.py -- the edge inputs that tests/test_gpu_build_edges.py feeds the device builders -- held against what
their table claims, so that the device comparisons cannot be vacuous.  Needs no GPU: the host builder (the device SAH and median
builders' reference), the numpy restatement of both builders (oracle/np_oracle.py) and chapter 2's brute-force query.

Host builder against `NPO.build_bvh`: the restatement refuses equal centroid keys inside a range it sorts (std::sort leaves their
order to the library).  Where it accepts an input, the host builder equals it on the bits; where it refuses (REFUSED below), the
host builder with its stable sort IS the reference, the rule tests/test_gpu_lbvh.py's ties cases already use."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import build_edge_scenes as B  # noqa: E402
import np_oracle as NPO  # noqa: E402

from ezrt_amd import scene as S  # noqa: E402

MIN_NORMAL = np.float32(1.1754944e-38)
# (case, sah) that the numpy restatement takes; every other one it refuses for equal keys
ACCEPTED = {(name, sah) for name in ("big", "beyond_inf", "beyond_sentinel", "tiny", "subnormal") for sah in (True, False)}
ACCEPTED |= {("line", False), ("flat", False)}
NPO_NAMES = ("line", "flat", "signed0", "big", "beyond_inf", "beyond_sentinel", "tiny", "subnormal", "inf", "overflow_centroid")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(T, sah=True, leaf_n=8):
    hs = S.HostScene()
    hs.addTriangles(T)
    (hs.buildBVHwithSAH if sah else hs.buildBVH)(leaf_n)
    tri, nodes = hs.encode()
    return tri, nodes, hs.buildStats()


def test_every_case_has_its_size_and_its_tags():
    for name in B.ALL_NAMES:
        T = B.case(name)
        assert T.dtype == np.float32 and T.ndim == 2 and T.shape[1] == 36
        assert np.array_equal(T[:, 18], np.arange(T.shape[0], dtype=np.float32))        # repeated triangles stay distinguishable
    assert B.case("dup_chain").shape[0] == 4200 and B.case("line").shape[0] == 150 and B.case("near_flt_max").shape[0] == 40
    assert [B.case("size_%d" % n).shape[0] for n in B.SIZES] == list(B.SIZES)
    assert [B.case("ties_%d" % n).shape[0] for n in B.TIES] == list(B.TIES)
    for name in ("flat", "signed0", "big", "beyond_inf", "beyond_sentinel", "tiny", "subnormal", "inf", "overflow_centroid",
                 "nan_vertex"):
        assert B.case(name).shape[0] == 300
    assert set(B.PARITY_NAMES) | set(B.LBVH_ONLY) == set(B.ALL_NAMES) and set(B.HITTABLE) <= set(B.PARITY_NAMES)


@pytest.mark.parametrize("name", ["dup_chain", "line"])
def test_the_chains_are_deeper_than_4096_levels(name):
    """one triangle peeled per level: identical triangles (cost S (r - l + 1), first minimum at l) and a box with two zero extents
    (every cost +0).  depth n - leaf_n + 1"""
    T = B.dup_chain(4200) if name == "dup_chain" else B.line(4200)
    _, nodes, st = _host(T, True, 8)
    assert st["max_depth"] == 4193 > 4096 and nodes.shape[0] == 8386
    # 4105 triangles: the smallest size whose depth exceeds 4096 at leaf_n = 8
    if name == "dup_chain":
        assert _host(B.dup_chain(4105), True, 8)[2]["max_depth"] == 4098
        assert B.case("dup_chain").shape[0] >= 4105 and len(np.unique(_bits(B.case("dup_chain")[:, :9]), axis=0)) == 1


def test_line_is_a_chain_at_its_own_size_and_flat_is_flat():
    T = B.case("line")
    P = T[:, :9].reshape(-1, 3, 3)
    assert np.all(P[:, :, 1:] == 0) and np.all(P[:, 0] == P[:, 1]) and np.all(P[:, 0] == P[:, 2])       # points on the x axis
    assert len(np.unique(P[:, 0, 0])) == T.shape[0] and not np.all(np.diff(P[:, 0, 0]) > 0)              # distinct, shuffled
    assert _host(T, True, 8)[2]["max_depth"] == T.shape[0] - 8 + 1
    F = B.case("flat")[:, :9].reshape(-1, 3)
    assert np.all(F[:, 2] == np.float32(0.25)) and np.ptp(F[:, 0]) > 1 and np.ptp(F[:, 1]) > 1


def test_signed0_has_both_zeros_among_its_centroids():
    T = B.case("signed0")
    P = T[:, :9]
    assert np.array_equal(P * 2, np.round(P * 2))                                                        # the half-integer grid
    assert ((P == 0) & np.signbit(P)).sum() > 50 and ((P == 0) & ~np.signbit(P)).sum() > 50
    c = B.centroids(T)
    neg = ((c == 0) & np.signbit(c)).sum(0)
    pos = ((c == 0) & ~np.signbit(c)).sum(0)
    print("signed0 centroids: -0.0 per axis %s, +0.0 per axis %s" % (neg, pos))
    assert np.any((neg >= 2) & (pos >= 2))


def test_the_scaled_cases_reach_the_caps_they_name():
    sentinel = np.float32(1145141919)
    T = B.case("beyond_sentinel")
    assert T[:, :9].min() > sentinel
    _, nodes, _ = _host(T, True, 8)
    assert np.array_equal(_bits(nodes[1, 6:9]), _bits(np.full(3, sentinel, np.float32)))                 # AA never leaves its start value
    T = B.case("beyond_inf")
    assert np.abs(T[:, :9]).max() > 114514 and np.abs(T[:, :9]).max() < sentinel
    _, nodes, st = _host(T, True, 1)
    inner = int((nodes[1:, 3] == 0).sum())
    assert inner == T.shape[0] - 1 and st["inf_cap_nodes"] == inner                                       # every node is capped
    _, nodes, st = _host(B.case("big"), True, 1)
    assert 0 < st["inf_cap_nodes"] < int((nodes[1:, 3] == 0).sum())                                      # the top levels only


def test_tiny_and_subnormal_underflow_where_they_say():
    T = B.case("tiny")
    V = T[:, :9].reshape(-1, 3)
    ext = V.max(0) - V.min(0)
    with np.errstate(under="ignore"):
        area = ext[0] * ext[1]
    assert 0 < area < MIN_NORMAL and np.abs(V).min() > MIN_NORMAL                                        # normal coordinates, subnormal area
    T = B.case("subnormal")
    c = B.centroids(T)
    assert np.all(c != 0) and np.all(np.abs(c) < MIN_NORMAL) and np.all(np.abs(T[:, :9]) < MIN_NORMAL)
    assert _host(T, True, 8)[2]["max_depth"] > 100                                                       # the costs do underflow to ties


def test_the_non_finite_cases():
    for name in ("inf", "overflow_centroid"):
        c = B.centroids(B.case(name))
        assert np.isinf(c).any() and not np.isnan(c).any()
    T = B.case("inf")
    assert (T[:, :9] == np.inf).any(1).sum() == 9 and (T[:, :9] == -np.inf).any(1).sum() == 8
    assert not ((T[:, :9] == np.inf).any(1) & (T[:, :9] == -np.inf).any(1)).any()                       # never both signs in one triangle
    assert np.isfinite(B.case("overflow_centroid")[:, :9]).all()
    T = B.case("nan_vertex")
    assert np.isnan(B.centroids(T)).any(1).sum() == 3 and np.isnan(T[:, :9]).sum() == 3
    T = B.case("near_flt_max")
    x = T[:, 0:9:3]
    assert np.all(x >= np.float32(3.401e38)) and np.all(x <= np.float32(3.402e38)) and np.isfinite(T[:, :9]).all()
    assert np.all(x > np.float32(3.4e38))                                                                # beyond the linear BVH's former box seed


@pytest.mark.parametrize("leaf_n", [8, 1])
@pytest.mark.parametrize("sah", [True, False])
@pytest.mark.parametrize("name", NPO_NAMES)
def test_host_builder_against_the_numpy_restatement(name, sah, leaf_n):
    T = B.case(name)
    try:
        with np.errstate(all="ignore"):
            order, ref_nodes = NPO.build_bvh(T, leaf_n, sah)
    except AssertionError as e:
        assert "equal centroid keys" in str(e)
        assert (name, sah) not in ACCEPTED, "the restatement must take this input"
        return        # refused: the host builder with its stable sort is the reference
    assert (name, sah) in ACCEPTED
    tri, nodes, _ = _host(T, sah, leaf_n)
    assert np.array_equal(_bits(tri), _bits(T[order]))
    assert nodes.shape == (len(ref_nodes), 12) and np.array_equal(_bits(nodes), _bits(NPO.encode_nodes(ref_nodes)))


def test_which_cases_rays_can_hit():
    """The device test compares traces three ways on the HITTABLE cases and wants more than zero hits there.  `tiny` is the
    exception, and provably so: hitTriangle (P2/main.cpp:212-238) normalises cross(p2 - p1, p3 - p1), whose squared length --
    edges of about 1e-20 to the fourth power -- underflows to zero, so no ray hits any of its triangles (and t < 0.0005 rejects
    what starts inside its box).  It stays in the three-way comparison, where all three must agree on zero hits."""
    for name in B.HITTABLE:
        T = B.case(name)
        _, idx, _ = S.p2Query(T[:, :9], B.rays_at(T, 600, B.SEED), use_bvh=False)
        hits = int((idx >= 0).sum())
        print("%s: %d of 600 rays hit (brute force)" % (name, hits))
        assert (hits == 0) if name in B.UNHITTABLE else (hits > 0)
    P = B.case("tiny")[:, :9].reshape(-1, 3, 3)
    with np.errstate(under="ignore"):
        n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).astype(np.float32)
        assert np.all((n * n).sum(1, dtype=np.float32) == 0)

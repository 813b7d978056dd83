"""tests/winding_expected.py -- the numpy restatement of include/ezrt_winding.h that the GPU test and the host check compare with on
the bits -- held against the real-number value and against the header's own claims.  Needs no GPU and no library.

* Against the truth: a float64 evaluation (np.arctan2, summed in float64) on the voxel solid, the same with every fifth face
  removed, the small Bunny and the adversarial scene, within the header's DERIVED bound
      (2^-22 sum_k |t_k| + n_tri 2^-37) / (2 pi) + 2^-24 |winding|
  on every point where the float64 evaluation itself can be trusted (its own error, estimated per point, below 1 % of the bound:
  that leaves out the points constructed ON the surface, where the real-number value jumps).  Largest measured error / bound:
  voxel solid 0.208, open solid 0.158, Bunny 0.181, adversarial 0.245 (errors up to 1.03e-7, on the adversarial scene's 2 812
  triangles).
* 1.0f inside and 0 outside the closed solid, by the occupancy grid, within the bound.
* On the bits of `fixed`: the order of the triangles, the six vertex orders (three keep, three negate), a doubled mesh, additivity.
* Terms that are 0: points in a triangle's plane on and off it, on vertices and edges, repeated and non-finite vertices, non-finite
  points.  The int64 budget.  ez_atan2 in numpy against np.arctan2."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_point_expected as E  # noqa: E402
import inside_scenes as IS  # noqa: E402
import winding_expected as WE  # noqa: E402
import winding_scenes as WS  # noqa: E402

NAMES = WS.CPU_NAMES


_cache = {}


def _case(name, bunny_small):
    """(tri, points, S, sum |t|) -- computed once"""
    if name not in _cache:
        tri, nodes = WS.scene(name, bunny_small)
        pts, _ = E.points_for(tri, nodes, WS.SEED + NAMES.index(name))
        pts = pts[::2]                                               # every kind, the non-finite ones included
        S, abs_t = WE.fixed(pts, tri, abs_t=True)
        _cache[name] = (tri, pts, S, abs_t)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_against_the_float64_truth(bunny_small, name):
    tri, pts, S, abs_t = _case(name, bunny_small)
    w = WE.winding_of(S)
    assert w.dtype == np.float32 and S.dtype == np.int64
    tw, tA, terr = WE.truth(pts, tri)
    bd = WE.bound(tA, tri.shape[0], tw)
    finite = np.isfinite(pts).all(1)
    kept = finite & (terr <= 0.01 * bd)
    assert kept.sum() >= 0.55 * finite.sum()                         # (the rest lies on the surface: constructed there)
    err = np.abs(w.astype(np.float64) - tw)
    ratio = float((err[kept] / bd[kept]).max())
    print("%s: %d triangles, %d of %d points, max error %.3g, max error / bound %.3f" % (name, tri.shape[0], kept.sum(), pts.shape[0],
                                                                                         err[kept].max(), ratio))
    assert ratio <= 1.0, ratio
    assert np.allclose(abs_t[kept], tA[kept], rtol=1e-5, atol=1e-6)   # (the bound's own sum does not depend on whose |t| it is)
    assert not S[~finite].any() and (~finite).sum() >= 20             # a non-finite point: S = 0
    assert np.abs(tw[kept]).max() > 0.9 and np.abs(tw[kept]).min() < 0.01


def test_one_inside_and_zero_outside_the_closed_solid():
    v = IS.voxel_solid()
    tri, pts, truth, kept = v["tri"], v["points"], v["truth"], v["kept"]
    centres = kept & (v["kind"] == 0)                                 # voxel centres: never on the surface
    S, abs_t = WE.fixed(pts[centres], tri, abs_t=True)
    w = WE.winding_of(S).astype(np.float64)
    want = truth[centres].astype(np.float64)
    assert want.sum() >= 50 and (1 - want).sum() >= 200
    assert np.all(np.abs(w - want) <= WE.bound(abs_t, tri.shape[0], want))
    assert np.count_nonzero(w[want == 1] == 1.0) >= 0.5 * want.sum()  # mostly 1.0f exactly
    # the grid's own vertices and line points that are off the surface, too
    off = kept & (v["kind"] > 0)
    S, abs_t = WE.fixed(pts[off], tri, abs_t=True)
    want = truth[off].astype(np.float64)
    assert np.all(np.abs(WE.winding_of(S).astype(np.float64) - want) <= WE.bound(abs_t, tri.shape[0], want))


def test_the_order_of_the_triangles_does_not_matter(bunny_small):
    for name in ("open_solid", "nasty"):
        tri, pts, S, _ = _case(name, bunny_small)
        perm = np.random.default_rng(5).permutation(tri.shape[0])
        assert np.array_equal(WE.fixed(pts, tri[perm]), S), name


def test_vertex_orders_keep_or_negate_exactly(bunny_small):
    tri, pts, S, _ = _case("nasty", bunny_small)
    P = WE.vertices(tri)
    q = WE.terms(pts[:300], P)
    assert np.count_nonzero(q) > 0.9 * q.size * np.isfinite(pts[:300]).all(1).mean()
    for order in itertools.permutations(range(3)):
        even = order in ((0, 1, 2), (1, 2, 0), (2, 0, 1))
        got = WE.terms(pts[:300], P[:, list(order)])
        assert np.array_equal(got, q if even else -q), order
    # every triangle flipped: the sum is negated
    assert np.array_equal(WE.fixed(pts, P[:, [0, 2, 1]]), -S)


def test_a_doubled_mesh_and_a_split_mesh(bunny_small):
    tri, pts, S, _ = _case("open_solid", bunny_small)
    assert np.array_equal(WE.fixed(pts, np.concatenate([tri, tri])), 2 * S)
    cut = tri.shape[0] // 3 + 1
    assert np.array_equal(WE.fixed(pts, tri[:cut]) + WE.fixed(pts, tri[cut:]), S)
    assert np.array_equal(WE.terms(pts, tri).sum(1), S)


def test_terms_that_are_zero():
    # a triangle in the plane z = 2 and points of that plane: on it, on its edges and vertices, off it
    P = np.float32([[[1, 1, 2], [5, 1, 2], [1, 4, 2]]])
    on = np.float32([[2, 2, 2], [1.5, 1.25, 2], [3, 1, 2], [1, 2.5, 2], [3, 2.5, 2], [1, 1, 2], [5, 1, 2], [1, 4, 2], [9, 9, 2], [-3, 0.5, 2], [1e6, 3, 2]])
    assert not WE.terms(on, P).any()
    off = np.float32([[2, 2, 2.5], [2, 2, 1.5], [2, 2, 2 + 2.0 ** -20]])
    q = WE.terms(off, P)[:, 0]
    assert q[0] < 0 and q[1] == -q[0] and q[2] < -0.99 * np.pi * 2.0 ** 36  # (the normal points to +z: the point in front of the face sees -, the one behind +)
    # the voxel solid (integer coordinates): a point on a vertex or on the midpoint of an edge gets nothing from the triangles
    # that hold that vertex or edge
    tri = IS.voxel_solid()["tri"]
    V = WE.vertices(tri)
    k = np.arange(0, V.shape[0], 3)
    for e in range(3):
        assert not WE.terms_at(V[k, e], tri, k).any()
        assert not WE.terms_at((V[k, e] + V[k, (e + 1) % 3]) * np.float32(0.5), tri, k).any()
    # repeated vertices (two equal by value, -0 against +0 included) and non-finite vertices
    p = np.float32([[0.3, 0.2, 1.0], [0.1, -0.4, -2.0]])
    a, b, c = np.float32([0, 0, 0]), np.float32([1, 0, 0]), np.float32([0, 1, 0])
    dead = [[a, a, c], [a, b, b], [c, b, c], [a, a, a], [a, b, np.float32([-0.0, 0.0, -0.0])]]
    for bad in (np.inf, -np.inf, np.nan):
        for i in range(3):
            x = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
            x[i, (i + 1) % 3] = bad
            dead.append(x)
    assert not WE.terms(p, np.float32(dead)).any()
    assert WE.terms(p, np.float32([[a, b, c]])).all()
    assert WE.terms(p, np.float32([[a, b, np.float32([3e38, -3e38, 3e38])]])).all()       # huge but finite: no overflow in fp64
    # non-finite points
    bad_p = np.float32([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf]])
    assert not WE.terms(bad_p, np.float32([[a, b, c]])).any() and not WE.fixed(bad_p, tri).any()
    assert np.array_equal(WE.terms_at(p, tri, np.int32([[-1, tri.shape[0]], [2 ** 30, -2 ** 31]])), np.zeros((2, 2), np.int64))


def test_the_int64_budget():
    t = np.float32([np.pi, -np.pi, 3.14159265358979323846])
    q = np.rint(t.astype(np.float64) * WE.SCALE).astype(np.int64)
    assert np.abs(q).max() < WE.Q_MAX == 2 ** 38                      # |t| <= pi < 4
    assert WE.Q_MAX * WE.N_TRI_MAX == 2 ** 62 and 2 * WE.Q_MAX * WE.N_TRI_MAX - 1 <= np.iinfo(np.int64).max   # two scenes added still fit
    full = WE.ez_atan2(np.float32([0.0, -0.0, 1e-30, -1e-30]), np.float32([-1.0, -1.0, -1.0, -1.0]))
    assert np.abs(full).max() <= np.float32(np.pi)                    # the largest |t| the definition returns
    assert WE.winding_of(np.int64([0, 2 ** 62]))[0] == 0 and float.hex(WE.INV_2PI) == "0x1.45f306dc9c883p-3"
    assert abs(WE.INV_2PI * 2 * np.pi - 1) < 2.0 ** -52


def test_numpy_ez_atan2_is_an_atan2():
    rng = np.random.default_rng(23)
    y, x = rng.normal(size=200000).astype(np.float32), rng.normal(size=200000).astype(np.float32)
    y[:1000] *= np.float32(1e-6)
    x[1000:2000] *= np.float32(1e-6)
    got = WE.ez_atan2(y, x).astype(np.float64)
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    assert np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref) + 1e-45)         # "a few fp32 ulps of |t|": the bound's first term
    s = np.float32([0.0, 1.0, -1.0, 0.0, 2.0, -2.0])
    assert np.array_equal(WE.ez_atan2(s, np.zeros(6, np.float32)), np.float32([0, np.pi / 2, -np.pi / 2, 0, np.pi / 2, -np.pi / 2]))

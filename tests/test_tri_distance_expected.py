"""The yardstick of the triangle-distance tests pinned to true geometry before the device is compared with it, and the parts of the
binding that need no device (include/ezrt_tri_distance.h, ezrt_amd/query.py).

tests/tri_distance_expected.py restates the header's definition in numpy float32.  Here:

* its distances agree with a float64 truth written differently -- the point-triangle distance by plane projection and the three edges
  (as tests/test_closest_point_expected.py), the segment-segment distance as the distance of the two lines where the feet of their
  common perpendicular lie on both segments, and 0 where an EXACT edge-against-triangle test says the pair crosses: the float32
  coordinates are put on one integer grid (they are dyadic) and every predicate is a sign of an integer determinant;
* constructed pairs on integer grids give their known answers, the piercing pair with all 15 sub-candidates positive;
* d_max cuts at the winner's own distance exactly, queries and scene triangles that are not live are left out;
* the pruning inequality holds on the bits: lb <= dist2 against each triangle's own bounding box and against every box above it, for
  all pairs of 300 queries over the base set of tests/tree_shapes.py, tie queries among them;
* the pruned evaluation of the restatement (what the device tests use on the larger scenes) equals the full one;
* the binding table equals the header's prototypes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import tree_shapes as T  # noqa: E402
import tri_distance_expected as TD  # noqa: E402
import tri_distance_scenes as DS  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

F = np.float32
# |dist32 - dist64| <= MARGIN * max(dist64, largest |coordinate| of the query and of the scene).  4 x the largest value measured on the
# CPU for the fixed seeds below (5.26e-8 on `nasty`, 2026-10-18; voxel_solid 3.71e-8, bunny 4.60e-8, ties 2.20e-8): the seeds are
# fixed, and the bound only has to catch a wrong region or a missed feature (an error of the size of a triangle), not a rounding.
MEASURED = 5.26e-8
MARGIN = 4 * MEASURED
SCENES = ("voxel_solid", "bunny", "nasty", "ties")
N_TRUTH = 300                                                      # queries per scene held against the truth


# ---- the float64 truth, per pair

def _d(u, w):
    return np.einsum("...k,...k", u, w)


def _seg(p, a, b):
    ab = b - a
    t = np.clip(_d(p - a, ab) / np.maximum(_d(ab, ab), 1e-300), 0.0, 1.0)
    return np.linalg.norm(p - (a + ab * t[..., None]), axis=-1)


def _point_triangle(p, a, b, c):
    d = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
    n = np.cross(b - a, c - a)
    nn = _d(n, n)
    with np.errstate(all="ignore"):
        h = _d(p - a, n) / nn
        f = p - n * h[..., None]                                       # the foot of the perpendicular
        inside = ((_d(np.cross(b - a, f - a), n) >= 0) & (_d(np.cross(c - b, f - b), n) >= 0) & (_d(np.cross(a - c, f - c), n) >= 0) & (nn > 0))
        return np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn)), d)


def _lines(p1, q1, p2, q2):
    """the distance of the two lines where the feet of the common perpendicular lie on both segments, else +inf (the end points are
    the point-triangle distances' business)"""
    d1, d2, w = q1 - p1, q2 - p2, p2 - p1
    n = np.cross(d1, d2)
    nn = _d(n, n)
    with np.errstate(all="ignore"):
        s, t = _d(np.cross(w, d2), n) / nn, _d(np.cross(w, d1), n) / nn
        return np.where((nn > 0) & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1), np.abs(_d(w, n)) / np.sqrt(nn), np.inf)


def apart64(Q, V):
    """float64 [p]: the distance of triangles Q and V [p, 3, 3] that do not cross"""
    Q, V = Q.astype(np.float64), V.astype(np.float64)
    d = np.full(Q.shape[0], np.inf)
    for i in range(3):
        d = np.minimum(d, _point_triangle(Q[:, i], V[:, 0], V[:, 1], V[:, 2]))
        d = np.minimum(d, _point_triangle(V[:, i], Q[:, 0], Q[:, 1], Q[:, 2]))
        for j in range(3):
            d = np.minimum(d, _lines(Q[:, i], Q[:, (i + 1) % 3], V[:, j], V[:, (j + 1) % 3]))
    return d


# ---- the exact crossing test: integers

def on_a_grid(*arrays):
    """the float32 arrays as nested lists of python ints on one grid of 2^k steps (exact: a float32 is an integer times a power of two)"""
    flat = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in arrays])
    m, e = np.frexp(flat)
    mi = np.round(m * 2.0 ** 24).astype(np.int64)
    assert np.array_equal(mi.astype(np.float64) * 2.0 ** -24, m)
    e = e - 24
    emin = int(e[mi != 0].min()) if (mi != 0).any() else 0
    ints = np.array([int(a) << max(int(b) - emin, 0) for a, b in zip(mi.tolist(), e.tolist())], dtype=object)
    out, at = [], 0
    for a in arrays:
        out.append(ints[at:at + a.size].reshape(a.shape).tolist())
        at += a.size
    return out


def _sub(u, w):
    return (u[0] - w[0], u[1] - w[1], u[2] - w[2])


def _cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def _dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def _sgn(x):
    return (x > 0) - (x < 0)


def _orient2(u, v, w):
    return _sgn((v[0] - u[0]) * (w[1] - u[1]) - (v[1] - u[1]) * (w[0] - u[0]))


def _segments_meet_2d(p, q, u, v):
    o1, o2, o3, o4 = _orient2(p, q, u), _orient2(p, q, v), _orient2(u, v, p), _orient2(u, v, q)
    if o1 == o2 == o3 == o4 == 0:                                      # on one line: the intervals must overlap on both axes
        return all(max(min(p[c], q[c]), min(u[c], v[c])) <= min(max(p[c], q[c]), max(u[c], v[c])) for c in (0, 1))
    return o1 * o2 <= 0 and o3 * o4 <= 0


def _in_triangle_2d(p, a, b, c):
    o = (_orient2(a, b, p), _orient2(b, c, p), _orient2(c, a, p))
    return min(o) >= 0 or max(o) <= 0


def segment_meets_triangle(p, q, a, b, c):
    """exact: does the closed segment [p, q] meet the closed triangle (a, b, c) with a normal that is not zero?"""
    n = _cross(_sub(b, a), _sub(c, a))
    sp, sq = _sgn(_dot(n, _sub(p, a))), _sgn(_dot(n, _sub(q, a)))
    if sp == 0 and sq == 0:                                            # in the plane: drop a coordinate along which the normal is not zero
        j = 0 if n[0] != 0 else (1 if n[1] != 0 else 2)
        flat = lambda x: tuple(x[k] for k in range(3) if k != j)
        p, q, a, b, c = flat(p), flat(q), flat(a), flat(b), flat(c)
        return (_in_triangle_2d(p, a, b, c) or _in_triangle_2d(q, a, b, c) or _segments_meet_2d(p, q, a, b) or
                _segments_meet_2d(p, q, b, c) or _segments_meet_2d(p, q, c, a))
    if sp * sq > 0:
        return False
    d = _sub(q, p)                                                     # the line through p and q passes the three edges on one side
    o = (_sgn(_dot(_cross(_sub(a, p), _sub(b, p)), d)), _sgn(_dot(_cross(_sub(b, p), _sub(c, p)), d)), _sgn(_dot(_cross(_sub(c, p), _sub(a, p)), d)))
    return min(o) >= 0 or max(o) <= 0


def triangles_cross(q, s):
    """exact: two closed proper triangles share a point when an edge of one meets the other (a triangle inside the other's plane
    region has its edges there)"""
    return any(segment_meets_triangle(q[i], q[(i + 1) % 3], *s) or segment_meets_triangle(s[i], s[(i + 1) % 3], *q) for i in range(3))


def true_distance(Q, V):
    """float64 [n]: the distance of each live triangle of Q [n, 3, 3] from the live triangles of V [m, 3, 3]; NaN for one that is not live"""
    ql, vl = TE.live(Q), TE.live(V)
    V = V[vl]
    Qd, Vd = Q.astype(np.float64), V.astype(np.float64)
    out = np.full(Q.shape[0], np.nan)
    qi, vi = on_a_grid(Q[ql], V)
    lo, hi = Vd.min(1), Vd.max(1)
    for at, i in enumerate(np.nonzero(ql)[0]):
        gap = np.sqrt((np.maximum(np.maximum(lo - Qd[i].max(0), Qd[i].min(0) - hi), 0.0) ** 2).sum(1))
        touching = np.nonzero(gap == 0)[0]
        if any(triangles_cross(qi[at], vi[k]) for k in touching):
            out[i] = 0.0
            continue
        seeds = np.argsort(gap)[:8]
        U = apart64(np.repeat(Qd[i:i + 1], seeds.size, 0), Vd[seeds]).min()
        keep = np.nonzero(gap <= U * (1 + 1e-9))[0]                    # a box farther than a distance already found holds nothing nearer
        out[i] = apart64(np.repeat(Qd[i:i + 1], keep.size, 0), Vd[keep]).min()
    return out


# ---- the tests

_cache = {}


def _case(name, bunny_small):
    if name not in _cache:
        if name == "ties":
            tri, nodes, _ = A.scene(name, bunny_small)
            q = DS.tris_for(tri, nodes, DS.SEED + 7)
        else:
            tri, nodes, q = DS.host_case(name, bunny_small)
        q = q[:N_TRUTH]
        _cache[name] = (tri, nodes, q, TD.query(q, tri, prune=True))
    return _cache[name]


@pytest.mark.parametrize("name", SCENES)
def test_against_true_geometry(bunny_small, name):
    tri, nodes, q, (win, dist, x, y, crosses) = _case(name, bunny_small)
    Q, V = q.reshape(-1, 3, 3), TE.vertices(tri)
    d64 = true_distance(Q, V)
    live = ~np.isnan(d64)
    assert np.array_equal(live, TE.live(Q)) and (win[~live] < 0).all() and (win[live] >= 0).all()
    scale = np.maximum(d64[live], np.maximum(np.abs(Q[live]).max((1, 2)), float(np.abs(V[TE.live(V)]).max())))
    err = np.abs(dist[live].astype(np.float64) - d64[live]) / scale
    print("%s: largest relative error %.3g (%d live queries, %d cross, %d apart)" % (name, err.max(), live.sum(), (d64[live] == 0).sum(),
                                                                                     (d64[live] > 0).sum()))
    assert (d64[live] == 0).sum() >= 30 and (d64[live] > 0).sum() >= 30
    assert err.max() <= MARGIN
    # crosses is the exact answer wherever the winner decides it: a pair that crosses has dist 0, and a winner apart does not cross
    assert (crosses[live][d64[live] > 0] == 0).all() and (dist[live][crosses[live] == 1] == 0).all()
    # the outputs belong together: |x - y| = dist where the pair does not cross, x in the query's bounding box, y in the winner's
    W = V[np.maximum(win, 0)]
    apart = live & (crosses == 0)
    assert np.all(np.abs(np.linalg.norm(x[apart].astype(np.float64) - y[apart], axis=1) - dist[apart]) <= 4 * MARGIN * scale[apart[live]])
    assert ((x[live] >= Q[live].min(1)) & (x[live] <= Q[live].max(1))).all() and ((y[live] >= W[live].min(1)) & (y[live] <= W[live].max(1))).all()


def test_the_exact_crossing_test_itself():
    a, b, c = (0, 0, 0), (8, 0, 0), (0, 8, 0)
    assert segment_meets_triangle((2, 2, -3), (2, 2, 3), a, b, c) and segment_meets_triangle((2, 2, 0), (2, 2, 3), a, b, c)
    assert not segment_meets_triangle((2, 2, 1), (2, 2, 3), a, b, c) and not segment_meets_triangle((5, 5, -1), (5, 5, 1), a, b, c)
    assert segment_meets_triangle((4, 4, -1), (4, 4, 1), a, b, c)                      # through the hypotenuse
    assert segment_meets_triangle((-2, 1, 0), (1, 1, 0), a, b, c) and not segment_meets_triangle((-2, 1, 0), (-1, 1, 0), a, b, c)
    assert segment_meets_triangle((1, 1, 0), (2, 2, 0), a, b, c)                      # inside, in the plane
    assert segment_meets_triangle((-4, 0, 0), (0, 0, 0), a, b, c) and segment_meets_triangle((-4, 0, 0), (12, 0, 0), a, b, c)
    assert not segment_meets_triangle((9, 0, 0), (12, 0, 0), a, b, c)                  # on an edge's line, beside it
    assert triangles_cross(((1, 1, 0), (2, 1, 0), (1, 2, 0)), (a, b, c))              # one inside the other, coplanar
    assert not triangles_cross(((1, 1, 1), (2, 1, 1), (1, 2, 1)), (a, b, c))
    ints = on_a_grid(F([0.75, -3.0, 0.0]), F([[1e-3, 2.0 ** -20]]))
    assert ints[0][1] < 0 and ints[0][2] == 0 and ints[0][0] * 4 == -ints[0][1] and ints[1][0][1] * 2 ** 20 * 3 == -ints[0][1]


def test_constructed_pairs_and_d_max():
    for leaf in (4, 8):
        tri, nodes, q, S, d2, crosses = DS.constructed(leaf)
        V = TE.vertices(tri)
        win, dist, x, y, cr = TD.query(q, tri)
        lowest = np.array([np.nonzero((V == S[i]).all((1, 2)))[0].min() for i in range(q.shape[0])])
        assert np.array_equal(win, lowest) and np.array_equal(dist, np.sqrt(d2)) and np.array_equal(cr, crosses)
        assert len(np.nonzero((V == S[DS.COPIES]).all((1, 2)))[0]) == DS.N_COPIES
    # the piercing pair: every one of the 15 sub-candidates is positive, and the points are those of their minimum
    sub = TD.all_d2(q[DS.PIERCING].reshape(3, 3), S[DS.PIERCING])
    assert sub.shape == (TD.N_SUB,) and (sub > 0).all() and dist[DS.PIERCING] == 0 and cr[DS.PIERCING] == 1
    e = x[DS.PIERCING] - y[DS.PIERCING]
    assert (e * e).sum() == sub.min()
    # nearest features of the others: |x - y|^2 is the pair's dist2, exactly
    e = (x - y).astype(np.float64)
    apart = crosses == 0
    assert np.array_equal((e * e).sum(1)[apart], d2[apart].astype(np.float64))
    # d_max at the winner's own distance keeps it, one ulp below loses it, NaN and negative values miss
    assert np.array_equal(TD.query(q, tri, dist)[0], win)
    below = TD.query(q, tri, np.nextafter(dist, F(-np.inf)))
    assert (below[0] < 0).all() and np.isposinf(below[1]).all() and not below[2].any() and not below[3].any() and not below[4].any()
    assert np.array_equal(TD.query(q, tri, np.nextafter(dist, F(np.inf)))[0], win)
    for bad in (np.nan, -1.0, -0.5):
        assert (TD.query(q, tri, np.full(q.shape[0], bad, F))[0] < 0).all()
    assert np.array_equal(TD.query(q, tri, np.full(q.shape[0], np.inf, F))[0], win)
    # the _at form: the winners again, an id outside the scene misses
    at = TD.at(q, tri, win)
    assert np.array_equal(at[0], dist) and np.array_equal(at[1], x) and np.array_equal(at[2], y) and np.array_equal(at[3], cr)
    assert np.isposinf(TD.at(q, tri, np.full(q.shape[0], tri.shape[0]))[0]).all() and np.isposinf(TD.at(q, tri, np.full(q.shape[0], -1))[0]).all()


def test_triangles_that_are_not_live():
    tri, nodes, q, S, d2, crosses = DS.constructed(4)
    win = TD.query(q, tri)[0]
    dead = q.copy().reshape(-1, 3, 3)
    dead[0, 1, 2] = np.nan
    dead[1, 0, 0] = np.inf
    dead[2, 2] = dead[2, 0]                                            # a repeated vertex
    dead[3] = np.stack([dead[3, 0], dead[3, 0] + F([1, 2, -1]), dead[3, 0] + F([2, 4, -2])])   # collinear
    got = TD.query(dead.reshape(-1, 9), tri)
    assert (got[0][:4] < 0).all() and np.isposinf(got[1][:4]).all() and not got[2][:4].any() and not got[4][:4].any()
    assert np.array_equal(got[0][4:], win[4:])
    # a scene triangle that is not live is never a candidate: the winner of case 0 made degenerate, the next nearest takes over
    bad = tri.copy()
    bad[win[0], 3:6] = bad[win[0], 0:3]
    other = TD.query(q[:1], bad)
    assert other[0][0] != win[0] and other[0][0] >= 0 and other[1][0] > 3
    bad[win[0], 3] = np.nan
    assert np.array_equal(TD.query(q[:1], bad)[0], other[0])


def _below(nodes, i, out):
    """the triangles below node i, for every node: out[i] = index array"""
    n, index = int(nodes[i, 3]), int(nodes[i, 4])
    if n > 0:
        out[i] = np.arange(index, index + n)
    else:
        out[i] = np.concatenate([_below(nodes, int(nodes[i, 0]), out), _below(nodes, int(nodes[i, 1]), out)])
    return out[i]


def test_the_pruning_inequality_on_the_bits():
    tri, nodes, _ = T.shape("sah8")
    V = TE.vertices(tri)
    ties, h = DS.tie_tris(tri)
    q = np.concatenate([DS.tris_for(tri, nodes, 77, 600)[:300 - ties.shape[0]], ties])
    Q = q.reshape(-1, 3, 3)
    live = TE.live(Q)
    cand, d2, cross = TD.dist2_all(q, tri)
    assert tri.shape[0] == 1209 and cand.sum() > 300_000 and cross.sum() > 500
    with np.errstate(all="ignore"):
        qlo, qhi = Q.min(1), Q.max(1)
        own = TD.box_lb(qlo[:, None], qhi[:, None], V.min(1)[None], V.max(1)[None])
    assert (own[cand] <= d2[cand]).all() and (own[cross] == 0).all()
    assert (own[cand] == d2[cand]).sum() > 1000                         # (boxes that overlap and triangles that touch: 0 == 0; the ties below)
    key = np.where(cand, d2, F(np.inf))
    below = {}
    _below(nodes, 1, below)
    assert len(below) > 250 and below[1].size == 1209
    at_the_bound = 0
    for i, ids in below.items():                                       # every box above a triangle: the node's own, as the walk meets them
        lb = TD.box_lb(qlo, qhi, nodes[i, 6:9][None], nodes[i, 9:12][None])
        nearest = key[:, ids].min(1)
        assert (lb[live] <= nearest[live]).all(), i
        at_the_bound += int((lb[live] == nearest[live]).sum())
    assert at_the_bound > 1000
    # the tie queries: lb of the winner's own box, the radius d_max * d_max and dist2 are one float32
    first = q.shape[0] - ties.shape[0]
    win, dist = TD.query(q, tri, table=(cand, d2, cross))[:2]
    r = np.arange(first, q.shape[0])
    assert np.array_equal(dist[first:], h) and np.array_equal(own[r, win[first:]], h * h) and np.array_equal(d2[r, win[first:]], h * h)
    assert np.array_equal(TD.query(q[first:], tri, h)[0], win[first:])


def test_the_pruned_evaluation_equals_the_full_one(bunny_small):
    for name, n in (("voxel_solid", 2100), ("nasty", 250)):
        tri, nodes, q = DS.host_case(name, bunny_small)
        full, pruned = TD.query(q[:n], tri), TD.query(q[:n], tri, prune=True)
        for a, b in zip(full, pruned):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    tri, nodes, q, S, d2, crosses = DS.constructed(4)
    for a, b in zip(TD.query(q, tri), TD.query(q, tri, prune=True)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_query_mix_of_the_device_test(bunny_small):
    """the shares the device test asserts again: at least 10 % of the queries cross, at least 10 % lie at a positive finite distance"""
    for name in ("voxel_solid", "bunny", "nasty", "ties"):
        win, dist, _, _, crosses = _case(name, bunny_small)[3]
        assert crosses.mean() >= 0.10 and ((dist > 0) & np.isfinite(dist)).mean() >= 0.10 and (win < 0).any(), name


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.TriDistance._fields == ("tri", "dist", "point_query", "point_scene", "crosses")
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_distance(None, torch.zeros((4, 9), dtype=torch.float32))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_distance(None, np.zeros((4, 9), np.float32))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_distance_at(None, torch.zeros((4, 9), dtype=torch.float32), torch.zeros(4, dtype=torch.int32))


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ezrt_tri_distance.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.TRI_DISTANCE_ABI) == ["ezrt_query_tri_distance_device", "ezrt_tri_distance_at_device"]
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.TRI_DISTANCE_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "NEAREST_ABI", "INSIDE_ABI", "BOX_OVERLAP_ABI", "TRI_OVERLAP_ABI", "SELF_OVERLAP_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other

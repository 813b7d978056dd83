"""The yardstick of the segment tests pinned to true geometry before the device is compared with it (include/ezrt_segment.h).

tests/segment_expected.py restates the header's definition in numpy float32.  Here:

* its distances agree with a float64 truth written differently -- the point-triangle distance by plane projection and the three edges,
  the segment-segment distance as the distance of the two lines where the feet of their common perpendicular lie on both segments,
  with the end points of either against the other as fall-backs, and 0 where an EXACT segment-against-triangle test says the pair
  crosses: the float32 coordinates are put on one integer grid and every predicate is a sign of an integer determinant (the helpers
  are tests/test_tri_distance_expected.py's, imported);
* independent of that truth: dist is no larger than the closest_point distance of 33 points sampled along the segment;
* a == b: the segment test with its zero directions equals the exact point-in-triangle answer on every zero-length query of the three
  scenes against every triangle whose box holds the point;
* constructed pairs on integer grids give their known answers, the piercing pair with all five sub-candidates positive;
* d_max and the radius cut at the winner's own distance exactly;
* the pruning inequality holds on the bits, lb <= dist2, against each triangle's own bounding box and against every box above it on
  every host tree shape of tests/tree_shapes.py;
* the consequences the header states between segment_distance, capsule_overlap and segment_distance_at;
* T1: a search for a pair that the segment test alone calls crossing while the boxes are disjoint;
* the sandwich against the sphere cast's restatement;
* the caps that keep the batches of the device test from hiding a failure."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_point_expected as E  # noqa: E402
import segment_expected as SX  # noqa: E402
import segment_scenes as SS  # noqa: E402
import self_overlap_expected as SE  # noqa: E402
import sphere_cast_expected as CE  # noqa: E402
import test_sphere_cast_expected as TC  # noqa: E402
import test_tri_distance_expected as TT  # noqa: E402
import tree_shapes as T  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

F = np.float32
# |dist32 - dist64| <= MARGIN * max(dist64, largest |coordinate| of the query and of the scene).  MEASURED: the largest value over the
# three scenes with the fixed seeds, ALL their queries (voxel_solid 7.38e-8 of 2 249 live queries, bunny 9.26e-9 of 1 916, nasty
# 4.13e-6 of 1 916); MARGIN: twice that, rounded up to a power of two.  The adversarial scene's figure is closest_point_triangle's on
# its slivers -- a point next to a triangle 2 long and 1e-3 high is put in the region of the wrong edge, an error of the size of the
# triangle's height, which the edge pairs then cut to a quarter; without such triangles the figure is that of tri_distance, 5e-8.
# test_against_true_geometry holds the first N_TRUTH queries of each scene against the truth and prints their figure.
MEASURED = 4.13e-6
MARGIN = 2.0 ** -16                                                # 1.53e-5 >= 2 * 4.13e-6 > 2 ** -17
N_TRUTH = 400                                                      # queries per scene held against the truth

_cache = {}


def _case(name, bunny_small):
    if name not in _cache:
        tri, nodes, segs, d_max, radius = SS.host_case(name, bunny_small)
        table = SX.dist2_all(segs, tri, prune=True, reach=np.maximum(d_max, radius))
        _cache[name] = dict(tri=tri, nodes=nodes, segs=segs, d_max=d_max, radius=radius, table=table, free=SX.query(segs, tri, None, table),
                            limited=SX.query(segs, tri, d_max, table), capsule=SX.capsule(segs, radius, tri, SS.MAX_K, table))
    return _cache[name]


# ---- the float64 truth

def apart64(A, B, V):
    """float64 [p]: the distance of segments [A, B] and triangles V [p, 3, 3] that do not cross"""
    A, B, V = A.astype(np.float64), B.astype(np.float64), V.astype(np.float64)
    d = np.minimum(TT._point_triangle(A, V[:, 0], V[:, 1], V[:, 2]), TT._point_triangle(B, V[:, 0], V[:, 1], V[:, 2]))
    for j in range(3):
        d = np.minimum(d, TT._lines(A, B, V[:, j], V[:, (j + 1) % 3]))
        d = np.minimum(d, TT._seg(V[:, j], A, B))                      # a vertex of the triangle against the segment
    return d


def true_answer(segs, V):
    """(float64 [n]: the distance of each live segment from the live triangles of V, NaN for one that is not live; bool [n]: does it
    meet one exactly; int [n]: the lowest triangle it meets, -1)"""
    ql, vl = SX.live(segs), TE.live(V)
    ids = np.nonzero(vl)[0]
    V = V[vl]
    A, B = SX.split(segs)
    Ad, Bd, Vd = A.astype(np.float64), B.astype(np.float64), V.astype(np.float64)
    out = np.full(A.shape[0], np.nan)
    first = np.full(A.shape[0], -1)
    ai, bi, vi = TT.on_a_grid(A[ql], B[ql], V)
    lo, hi = Vd.min(1), Vd.max(1)
    for at, i in enumerate(np.nonzero(ql)[0]):
        qlo, qhi = np.minimum(Ad[i], Bd[i]), np.maximum(Ad[i], Bd[i])
        gap = np.sqrt((np.maximum(np.maximum(lo - qhi, qlo - hi), 0.0) ** 2).sum(1))
        met = [k for k in np.nonzero(gap == 0)[0] if TT.segment_meets_triangle(ai[at], bi[at], *vi[k])]
        if met:
            out[i], first[i] = 0.0, ids[met[0]]
            continue
        seeds = np.argsort(gap)[:8]
        U = apart64(np.repeat(Ad[i:i + 1], seeds.size, 0), np.repeat(Bd[i:i + 1], seeds.size, 0), Vd[seeds]).min()
        keep = np.nonzero(gap <= U * (1 + 1e-9))[0]
        out[i] = apart64(np.repeat(Ad[i:i + 1], keep.size, 0), np.repeat(Bd[i:i + 1], keep.size, 0), Vd[keep]).min()
    return out, first >= 0, first


@pytest.mark.parametrize("name", SS.NAMES)
def test_against_true_geometry(bunny_small, name):
    c = _case(name, bunny_small)
    segs, V = c["segs"][:N_TRUTH], TE.vertices(c["tri"])
    win, dist, x, y, crosses, sub = [a[:N_TRUTH] for a in c["free"]]
    d64, meets, first = true_answer(segs, V)
    live = ~np.isnan(d64)
    assert np.array_equal(live, SX.live(segs)) and (win[~live] < 0).all() and (win[live] >= 0).all()
    scale = np.maximum(d64[live], np.maximum(np.abs(segs[live]).max(1), float(np.abs(V[TE.live(V)]).max())))
    err = np.abs(dist[live].astype(np.float64) - d64[live]) / scale
    print("%s: largest relative error %.3g (%d live queries, %d cross, %d apart)" % (name, err.max(), live.sum(), meets.sum(),
                                                                                     (d64[live] > 0).sum()))
    assert meets.sum() >= 30 and (d64[live] > 0).sum() >= 30
    assert err.max() <= MARGIN
    # crosses is the exact answer, and the winner of a crossing query the lowest triangle it meets
    assert np.array_equal(crosses[live] == 1, meets[live]) and np.array_equal(win[meets], first[meets])
    assert (dist[crosses == 1] == 0).all()
    # the outputs belong together: |x - y| = dist where the pair does not cross, x in the segment's bounding box, y in the winner's
    W = V[np.maximum(win, 0)]
    apart = live & (crosses == 0)
    assert np.all(np.abs(np.linalg.norm(x[apart].astype(np.float64) - y[apart], axis=1) - dist[apart]) <= 4 * MARGIN * scale[apart[live]])
    A, B = SX.split(segs)
    assert ((x[live] >= np.minimum(A, B)[live]) & (x[live] <= np.maximum(A, B)[live])).all()
    assert ((y[live] >= W[live].min(1)) & (y[live] <= W[live].max(1))).all()


@pytest.mark.parametrize("name", SS.NAMES)
def test_no_farther_than_sample_points(bunny_small, name):
    """independent of the truth above: the closest_point distance of 33 points along the segment bounds dist from above"""
    c = _case(name, bunny_small)
    pick = np.nonzero(SX.live(c["segs"]))[0][:120]
    A, B = SX.split(c["segs"][pick])
    u = (np.arange(33) / 32.0)[None, :, None]
    pts = (A[:, None].astype(np.float64) * (1 - u) + B[:, None].astype(np.float64) * u).astype(F).reshape(-1, 3)
    d = E.closest_point(pts, c["tri"])[2].reshape(-1, 33).min(1)
    scale = np.maximum(np.abs(c["segs"][pick]).max(1), float(np.abs(TE.vertices(c["tri"])[TE.live(TE.vertices(c["tri"]))]).max()))
    dist = c["free"][1][pick]
    assert (dist <= d + 2 * MARGIN * np.maximum(scale, d)).all()        # (the sample points themselves are rounded once: one MARGIN more)
    assert (dist < d).sum() >= 10                                      # ... and the samples do miss the nearest point between them


def test_a_point_against_the_exact_truth(bunny_small):
    """a == b: the six directions built from d = b - a are zero vectors and separate nothing; the normal and the nine g x axis_j of the
    triangle's edges decide.  Held against the exact point-in-triangle test on every zero-length live query of the three scenes x
    every live triangle whose bounding box holds the point (T1), and on grid points of the constructed triangle."""
    pairs = agree = inside = 0
    for name in SS.NAMES:
        c = _case(name, bunny_small)
        V = TE.vertices(c["tri"])
        segs = c["segs"]
        zero = SX.live(segs) & (segs[:, :3] == segs[:, 3:]).all(1)
        P = segs[zero, :3]
        i, k = np.nonzero(SX.t1(P[:, None], P[:, None], np.where(TE.live(V)[:, None, None], V, F(np.nan))[None]))
        got = SX.meets(P[i], P[i], V[k])
        pi, vi = TT.on_a_grid(P[i], V[k])
        want = np.array([TT.segment_meets_triangle(p, p, *v) for p, v in zip(pi, vi)], bool)
        pairs, agree, inside = pairs + i.size, agree + int((got == want).sum()), inside + int(want.sum())
    g = np.stack(np.meshgrid(np.arange(-2, 11), np.arange(-2, 11), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3).astype(F)
    tri = np.broadcast_to(F([[0, 0, 0], [8, 0, 0], [0, 8, 0]]), (g.shape[0], 3, 3))
    got = SX.t1(g, g, tri) & SX.meets(g, g, tri)
    want = (g[:, 2] == 0) & (g[:, 0] >= 0) & (g[:, 1] >= 0) & (g[:, 0] + g[:, 1] <= 8)
    print("a == b: %d point-triangle pairs inside T1, %d exactly on the triangle, %d agree" % (pairs, inside, agree))
    assert np.array_equal(got, want) and want.sum() == 45
    assert pairs >= 500 and inside >= 50 and agree == pairs


def test_constructed_pairs_d_max_and_radius():
    for leaf in (4, 8):
        tri, nodes, segs, where = SS.constructed(leaf)
        V = TE.vertices(tri)
        win, dist, x, y, cr, sub = SX.query(segs, tri)
        for i, (name, _, _, d2, crosses, cx, cy, csub) in enumerate(SS.CASES):
            shift = F([SS.SPACING * i, 0, 0])
            assert win[i] == where[i] and dist[i] == np.sqrt(F(d2)) and cr[i] == crosses, name
            assert cx is None or np.array_equal(x[i], F(cx) + shift), name
            assert cy is None or np.array_equal(y[i], F(cy) + shift), name
            assert csub is None or sub[i] == csub, name
    # the piercing pair: every one of the five sub-candidates is positive, and the points are those of their minimum
    A, B = SX.split(segs)
    d2s = np.array([d2 for _, _, d2 in SX.sub_candidates(A[SS.PIERCING], B[SS.PIERCING], V[where[SS.PIERCING]])])
    assert d2s.shape == (SX.N_SUB,) and (d2s > 0).all() and dist[SS.PIERCING] == 0 and cr[SS.PIERCING] == 1
    e = x[SS.PIERCING] - y[SS.PIERCING]
    assert (e * e).sum() == d2s.min()
    # nearest features of the others: |x - y|^2 is the pair's dist2, exactly
    e = (x - y).astype(np.float64)
    apart = cr == 0
    assert np.array_equal((e * e).sum(1)[apart], np.array([c[3] for c in SS.CASES], np.float64)[apart])
    # d_max and the radius at the winner's own distance keep it, one ulp below loses it, one above keeps it
    below, above = np.nextafter(dist, F(-np.inf)), np.nextafter(dist, F(np.inf))
    assert np.array_equal(SX.query(segs, tri, dist)[0], win) and np.array_equal(SX.query(segs, tri, above)[0], win)
    lost = SX.query(segs, tri, below)
    assert (lost[0] < 0).all() and np.isposinf(lost[1]).all() and not lost[2].any() and not lost[3].any() and not lost[4].any()
    r = np.arange(segs.shape[0])
    for radius, inside in ((dist, True), (above, True), (below, False)):
        rows, count = SX.capsule(segs, radius, tri, 8)
        assert np.array_equal((rows == win[:, None]).any(1), np.full(segs.shape[0], inside)), radius
        assert np.array_equal(count > 0, np.full(segs.shape[0], inside))
    for bad in (np.nan, -1.0, -0.5):
        assert (SX.query(segs, tri, np.full(segs.shape[0], bad, F))[0] < 0).all()
        assert not SX.capsule(segs, np.full(segs.shape[0], bad, F), tri, 8)[1].any()
    assert not SX.capsule(segs, np.full(segs.shape[0], np.inf, F), tri, 8)[1].any()            # the radius must be finite
    assert np.array_equal(SX.query(segs, tri, np.full(segs.shape[0], np.inf, F))[0], win)     # ... d_max need not be
    big = SX.capsule(segs, np.full(segs.shape[0], 3e19, F), tri, 8)                             # R2 = +inf admits every candidate
    assert (big[1] == TE.live(V).sum()).all() and np.array_equal(big[0], np.broadcast_to(np.nonzero(TE.live(V))[0][:8], big[0].shape))
    zero = SX.capsule(segs, np.zeros(segs.shape[0], F), tri, 8)                                 # r = 0: what is crossed or rounds to 0
    assert np.array_equal(zero[1] > 0, dist == 0) and np.array_equal(zero[0][:, 0], np.where(dist == 0, win, -1))
    # the _at form: the winners again, an id outside the scene misses
    at = SX.at(segs, tri, win)
    assert np.array_equal(at[0], dist) and np.array_equal(at[1], x) and np.array_equal(at[2], y) and np.array_equal(at[3], cr)
    for bad in (tri.shape[0], -1):
        miss = SX.at(segs, tri, np.full(segs.shape[0], bad))
        assert np.isposinf(miss[0]).all() and not miss[1].any() and not miss[2].any() and not miss[3].any()


def test_queries_and_triangles_that_are_not_live():
    tri, nodes, segs, where = SS.constructed(4)
    win = SX.query(segs, tri)[0]
    dead = segs.copy()
    for i, (j, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf))):
        dead[i, j] = v
    got = SX.query(dead, tri)
    assert (got[0][:6] < 0).all() and np.isposinf(got[1][:6]).all() and not got[2][:6].any() and not got[3][:6].any() and not got[4][:6].any()
    assert np.array_equal(got[0][6:], win[6:])
    rows, count = SX.capsule(dead, np.full(dead.shape[0], 100.0, F), tri, 4)
    assert not count[:6].any() and (rows[:6] == -1).all() and (count[6:] > 0).all()
    # a scene triangle that is not live is never a candidate: the winner of case 0 made degenerate, then given a NaN
    bad = tri.copy()
    bad[win[0], 3:6] = bad[win[0], 0:3]
    other = SX.query(segs[:1], bad)
    assert other[0][0] != win[0] and other[0][0] >= 0 and other[1][0] > 3
    bad[win[0], 3] = np.nan
    assert np.array_equal(SX.query(segs[:1], bad)[0], other[0])
    assert np.isposinf(SX.at(segs[:1], bad, win[:1])[0]).all()


def _reachable(nodes):
    """{node: triangle ids below it} of the nodes the root reaches, the root itself left out (its own box is never tested)"""
    below = {}
    TT._below(nodes, 1, below)
    below.pop(1, None)
    return below


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_the_pruning_inequality_on_the_bits(name):
    tri, nodes, expect = T.shape(name)
    V = TE.vertices(tri)
    segs, d_max, radius = SS.shape_queries(tri, expect, 300 + T.HOST_SHAPES.index(name))
    if name == "sah8":                                                 # queries whose lb, radius and dist2 are one float32
        grid, gd, gr = SS.queries_for(tri, 77, 600)
        on = np.all(grid * 8 == np.round(grid * 8), axis=1)
        segs, d_max, radius = np.concatenate([segs, grid[on]]), np.concatenate([d_max, gd[on]]), np.concatenate([radius, gr[on]])
    A, B = SX.split(segs)
    live = SX.live(segs)
    cand, d2, cross, _ = SX.dist2_all(segs, tri)
    with np.errstate(all="ignore"):
        qlo, qhi = np.minimum(A, B), np.maximum(A, B)
        own = SX.box_lb(qlo[:, None], qhi[:, None], V.min(1)[None], V.max(1)[None])
    assert cand.any() and (own[cand] <= d2[cand]).all() and (own[cross] == 0).all()
    facts = T.check_valid(tri, nodes)
    if facts["nested"] and facts["holds"]:                             # every box above a triangle, as the walk meets them
        key = np.where(cand, d2, F(np.inf))
        at_the_bound = 0
        for i, ids in _reachable(nodes).items():
            lb = SX.box_lb(qlo, qhi, nodes[i, 6:9][None], nodes[i, 9:12][None])
            nearest = key[:, ids].min(1)
            assert (lb[live] <= nearest[live]).all(), i
            at_the_bound += int((lb[live] == nearest[live]).sum())
        assert at_the_bound > 0 or len(_reachable(nodes)) == 0
    if name == "sah8":
        win, dist = SX.query(segs, tri, table=(cand, d2, cross))[:2]
        r = np.arange(segs.shape[0])
        tie = (win >= 0) & (dist > 0) & (own[r, np.maximum(win, 0)] == d2[r, np.maximum(win, 0)]) & (dist * dist == d2[r, np.maximum(win, 0)])
        print("sah8: %d queries whose winner's own lb, its dist2 > 0 and the radius dist * dist are one float32" % tie.sum())
        assert tie.sum() >= 8
        assert np.array_equal(SX.query(segs[tie], tri, dist[tie])[0], win[tie])
        assert (SX.capsule(segs[tie], dist[tie], tri, 0)[1] > 0).all()


@pytest.mark.parametrize("name", SS.NAMES)
def test_the_contracts_consequences(bunny_small, name):
    c = _case(name, bunny_small)
    segs, tri, radius, table = c["segs"], c["tri"], c["radius"], c["table"]
    rows, count = c["capsule"]
    win = SX.query(segs, tri, radius, table)[0]
    assert np.array_equal(win >= 0, count > 0)                         # d_max = r finds a triangle exactly where the capsule counts > 0
    fits = (count > 0) & (count <= SS.MAX_K)
    assert fits.sum() > 100 and (rows[fits] == win[fits][:, None]).any(1).all()                 # ... and that winner is in the row
    per = np.repeat(segs, SS.MAX_K, 0)
    d2 = SX.at(per, tri, rows.reshape(-1))[4].reshape(rows.shape)
    with np.errstate(all="ignore"):
        R2 = (radius * radius).astype(F)[:, None]
    assert ((d2 <= R2) == (rows >= 0)).all()                           # ... through dist2, not through dist
    # crosses: 1 exactly where the segment crosses some live triangle, and tri is then the lowest such id
    cross = table[2]
    free = c["free"]
    assert np.array_equal(free[4] == 1, cross.any(1)) and np.array_equal(free[0][cross.any(1)], np.argmax(cross, 1)[cross.any(1)])


def test_the_pruned_evaluation_equals_the_full_one(bunny_small):
    for name, n in (("voxel_solid", 2300), ("nasty", 300)):
        tri, nodes, segs, d_max, radius = SS.host_case(name, bunny_small)
        segs, d_max, radius = segs[:n], d_max[:n], radius[:n]
        full = SX.dist2_all(segs, tri)
        pruned = SX.dist2_all(segs, tri, prune=True, reach=np.maximum(d_max, radius))
        for dm in (None, d_max):
            for a, b in zip(SX.query(segs, tri, dm, full), SX.query(segs, tri, dm, pruned)):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        for a, b in zip(SX.capsule(segs, radius, tri, 64, full), SX.capsule(segs, radius, tri, 64, pruned)):
            assert np.array_equal(a, b), name


def test_t1_search(bunny_small):
    """T1 is in the rule so that a crossing pair has overlapping boxes whatever the rounded fp64 test says.  The search: over every
    pair of the three scenes whose boxes are DISJOINT but nearer than 1e-3 of the extent -- where a near miss would be -- does the
    segment test alone say "meets"?  None found (printed); T1 stays in the rule either way."""
    tested = found = 0
    for name in SS.NAMES:
        c = _case(name, bunny_small)
        V = TE.vertices(c["tri"])
        ok = TE.live(V)
        V = V[ok]
        segs = c["segs"][SX.live(c["segs"])]
        A, B = SX.split(segs)
        size = float(np.ptp(V.reshape(-1, 3), axis=0).max())
        qlo, qhi = np.minimum(A, B).astype(np.float64), np.maximum(A, B).astype(np.float64)
        gap = np.maximum(np.maximum(V.min(1)[None].astype(np.float64) - qhi[:, None], qlo[:, None] - V.max(1)[None]), 0.0).max(-1)
        i, k = np.nonzero((gap > 0) & (gap < 1e-3 * size))
        swap = TE._less(B[i], A[i])[:, None]
        got = SE.seg_meets(np.where(swap, B[i], A[i]), np.where(swap, A[i], B[i]), TE.sorted_vertices(V[k]))
        tested, found = tested + i.size, found + int(got.sum())
    print("T1 search: %d near pairs with disjoint boxes, %d that the segment test alone calls crossing" % (tested, found))
    assert tested > 10_000
    # a constructed near miss on huge coordinates, where fp64 products round: the boxes are disjoint by one ulp along x
    a, b = F([[3e37, 1, 1]]), F([[3e37, 2, 3]])
    V = np.nextafter(F([[[3e37, 0, 0], [3e37, 4, 0], [3e37, 0, 4]]]), F(0))
    V[0, :, 1:] = [[0, 0], [4, 0], [0, 4]]
    assert not SX.t1(a, b, V).any() and not SX.meets(a, b, V).any()


@pytest.mark.parametrize("name", SS.NAMES)
def test_sandwich_against_the_sphere_cast(bunny_small, name):
    """a contact at t <= 1 of the sphere of radius r - eps moving from a to b  =>  the capsule of radius r counts > 0  =>  a contact
    at t <= 1 for r + eps; eps = the sphere cast's measured tolerance (tests/test_sphere_cast_expected.py: TOL of the extent)"""
    c = _case(name, bunny_small)
    segs, radius, tri = c["segs"], c["radius"], c["tri"]
    V = TE.vertices(tri)
    size = float(np.ptp(V[TE.live(V)].reshape(-1, 3), axis=0).max())
    eps = F(TC.TOL * size)
    pick = np.nonzero(SX.live(segs) & (segs[:, :3] != segs[:, 3:]).any(1) & (radius > 2 * eps))[0][:600]
    A, B = SX.split(segs[pick])
    rays = np.concatenate([A, B - A], 1).astype(F)
    one = np.ones(pick.size, F)
    inner = CE.query(rays, radius[pick] - eps, tri, one)[0] >= 0
    outer = CE.query(rays, radius[pick] + eps, tri, one)[0] >= 0
    count = c["capsule"][1][pick] > 0
    print("%s: %d queries, %d / %d / %d contacts for r - eps / capsule r / r + eps" % (name, pick.size, inner.sum(), count.sum(), outer.sum()))
    assert inner.sum() >= 30 and (~outer).sum() >= 30
    assert (count[inner]).all() and (outer[count]).all()


@pytest.mark.parametrize("name", SS.NAMES)
def test_caps(bunny_small, name):
    c = _case(name, bunny_small)
    caps = SS.caps(c["segs"], c["free"], c["limited"], c["capsule"][1])
    print(name, {k: round(v, 3) for k, v in caps.items()})
    assert SS.caps_met(caps), caps
    A, B = SX.split(c["segs"][SX.live(c["segs"])])
    L = np.linalg.norm(B.astype(np.float64) - A, axis=1) / SS.leaf_size(c["tri"])
    assert (L[L > 0] < 0.2).sum() >= 20 and (L > 5).sum() >= 20          # lengths from 0.1 to 10 leaf sizes

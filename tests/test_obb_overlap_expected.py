"""The yardstick of the oriented-box tests pinned to true geometry before the device is compared with it (include/ezrt_obb_overlap.h).

tests/obb_overlap_expected.py restates the header in numpy.  Here it is held against a truth that shares nothing with it: the triangle
mapped into the box's own coordinates by Cramer's rule and clipped by the six half-spaces |s_j| <= 1, all in rational arithmetic
(fractions.Fraction) -- the triangle overlaps when a non-empty polygon remains.  On small integers the rule's fp64 numbers are exact
(the header's budget: a grid of 2^15 steps), so the two must agree on every pair, touching ones included.  Then: an axis-aligned box
gives box_overlap's rows, the orders of vertices and triangles change nothing, boxes that are not live and triangles that are not
finite overlap nothing, a row is a prefix of every longer one, the extremes of fp32 raise no numpy warning, and the two gates of a
walk never reject the box of a triangle that overlaps.  Needs no GPU."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_overlap_expected as BE  # noqa: E402
import inside_scenes as IS  # noqa: E402
import obb_overlap_expected as OE  # noqa: E402

F = np.float32


# ---- the truth
def _det(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def _box_coordinates(c, u, x):
    """s with x = c + s0 u0 + s1 u1 + s2 u2, by Cramer's rule (Fractions; u has volume)"""
    w = [x[i] - c[i] for i in range(3)]
    det = _det(u[0], u[1], u[2])
    return [Fraction(_det(w, u[1], u[2]), det), Fraction(_det(u[0], w, u[2]), det), Fraction(_det(u[0], u[1], w), det)]


def _clip(poly, axis, sign):
    """the part of the convex polygon `poly` (a list of points, repeated ones allowed) with sign * s[axis] <= 1, closed"""
    out = []
    for i, P in enumerate(poly):
        Q = poly[(i + 1) % len(poly)]
        fp, fq = sign * P[axis] - 1, sign * Q[axis] - 1
        if fp <= 0:
            out.append(P)
        if (fp < 0 < fq) or (fq < 0 < fp):
            t = fp / (fp - fq)
            out.append([P[k] + t * (Q[k] - P[k]) for k in range(3)])
    return out


def truth(c, u, tri):
    """does the closed triangle meet the closed box?  Integers in, exact."""
    poly = [_box_coordinates(c, u, x) for x in tri]
    for axis in range(3):
        for sign in (1, -1):
            poly = _clip(poly, axis, sign)
            if not poly:
                return False
    return True


# ---- the pairs: small integers
def _int_boxes(rng, n):
    """centres in -6..6, axes in -4..4, with volume"""
    c = rng.integers(-6, 7, (n, 3))
    u = rng.integers(-4, 5, (n, 3, 3))
    thin = rng.random(n) < 0.3                                        # many entries zero: axis-aligned and nearly so
    u[thin] = u[thin] * (rng.random((int(thin.sum()), 3, 3)) < 0.5)
    det = np.array([_det(*x.tolist()) for x in u])
    bad = det == 0
    u[bad] = np.eye(3, dtype=u.dtype) * rng.integers(1, 4, (int(bad.sum()), 1, 1))
    return c, u


def _int_pairs(rng):
    parts = []
    # generic triangles, two equal vertices, three equal vertices
    for n, kind in ((2400, "generic"), (700, "two"), (500, "one")):
        c, u = _int_boxes(rng, n)
        t = rng.integers(-8, 9, (n, 3, 3))
        if kind == "two":
            t[:, rng.integers(0, 3)] = t[:, 0] if rng.random() < 0.5 else t[:, 1]
            t[:, 1] = t[:, 0]
            t = t[:, rng.permutation(3)]
        if kind == "one":
            t[:, 1] = t[:, 0]
            t[:, 2] = t[:, 0]
        parts.append((c, u, t))
    # constructed touches: a vertex on a box corner, on an edge, in a face -- the rest of the triangle in the outward octant of the
    # box's own coordinates, or anywhere
    for n, free in ((500, 0), (500, 1), (500, 2)):
        c, u = _int_boxes(rng, n)
        s = rng.choice([-1, 1], (n, 3))
        on = s.copy()
        for f in range(free):                                          # `free` coordinates inside the face or along the edge
            on[np.arange(n), (rng.integers(0, 3, n) + f) % 3] = rng.integers(-1, 2, n)
        P = c + np.einsum("nj,njc->nc", on, u)
        out = lambda: np.einsum("nj,njc->nc", s * rng.integers(0, 3, (n, 3)), u)
        t = np.stack([P, P + out(), P + out()], 1)
        anywhere = rng.random(n) < 0.3
        t[anywhere, 1:] = rng.integers(-8, 9, (int(anywhere.sum()), 2, 3))
        parts.append((c, u, t[:, rng.permutation(3)]))
    # a box corner on the triangle's plane: inside the triangle, on its border, outside it
    n = 900
    c, u = _int_boxes(rng, n)
    P = c + np.einsum("nj,njc->nc", rng.choice([-1, 1], (n, 3)), u)
    a, b = rng.integers(-5, 6, (n, 3)), rng.integers(-5, 6, (n, 3))
    k = np.arange(n) % 3
    t = np.where((k == 0)[:, None, None], np.stack([P + a, P + b, P - a - b], 1),
                 np.where((k == 1)[:, None, None], np.stack([P + a, P - a, P + b], 1), np.stack([P + a, P + b, P + a + b], 1)))
    parts.append((c, u, t))
    return [np.concatenate([p[i] for p in parts]) for i in range(3)]


def test_the_rule_is_rational_clipping():
    c, u, t = _int_pairs(np.random.default_rng(2201))
    n = c.shape[0]
    assert n >= 4000
    got = OE.pairs(c.astype(F), u.astype(F), t.astype(F))
    want = np.array([truth(c[i].tolist(), u[i].tolist(), t[i].tolist()) for i in range(n)])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d of %d pairs differ from the rational truth, first: c %s u %s t %s (truth %s)" % (
        bad.size, n, c[bad[0]].tolist(), u[bad[0]].tolist(), t[bad[0]].tolist(), want[bad[0]])
    print("%d pairs, %d overlapping" % (n, int(want.sum())))
    assert n // 4 < want.sum() < 3 * n // 4                           # neither answer is rare
    # the touches touch and nothing more: a corner vertex with the rest of the triangle strictly outward overlaps, and moving the
    # triangle one step further out along that octant's diagonal does not
    cc, uu = np.zeros((1, 3), F), (np.eye(3) * 2).astype(F)[None]
    tt = np.array([[[2, 2, 2], [5, 2, 2], [2, 6, 3]]], F)
    assert OE.pairs(cc, uu, tt)[0] and not OE.pairs(cc, uu, tt + F(1))[0]


def _voxel():
    v = IS.voxel_solid()
    return v["tri"]


def test_an_axis_aligned_box_is_box_overlap():
    tri = _voxel()
    V = OE.vertices(tri)
    rng = np.random.default_rng(2202)
    lo_s, hi_s = np.floor(V.reshape(-1, 3).min(0)), np.ceil(V.reshape(-1, 3).max(0))
    n = 600
    c = rng.integers(lo_s - 1, hi_s + 2, (n, 3)).astype(F)
    h = rng.integers(1, 4, (n, 3)).astype(F)
    h[:20] = (hi_s - lo_s + 2).astype(F)                               # some hold everything
    u = np.zeros((n, 3, 3), F)
    perm = np.array([rng.permutation(3) for _ in range(n)])
    sign = rng.choice(F([-1, 1]), (n, 3))
    for j in range(3):                                                 # axis j along coordinate perm[j], either way
        u[np.arange(n), j, perm[:, j]] = h[np.arange(n), perm[:, j]] * sign[:, j]
    rows, count = OE.query(c, u, tri, 64)
    want = BE.query(c - h, c + h, tri, 64)
    assert np.array_equal(rows, want[0]) and np.array_equal(count, want[1])
    assert (count > 64).any() and (count == 0).any() and ((count > 0) & (count <= 64)).sum() > n // 4
    assert count.max() == V.shape[0]


def _float_pairs(rng, n, scale=1.0):
    c = (rng.normal(0, 1, (n, 3)) * scale).astype(F)
    u = (rng.normal(0, 0.6, (n, 3, 3)) * scale).astype(F)
    t = (c[:, None, :] + rng.normal(0, 1.2, (n, 3, 3)) * scale).astype(F)
    return c, u, t


def test_orders_do_not_matter():
    rng = np.random.default_rng(2203)
    ci, ui, ti = _int_pairs(rng)
    cf, uf, tf = _float_pairs(rng, 4000)
    for c, u, t in ((ci.astype(F), ui.astype(F), ti.astype(F)), (cf, uf, tf)):
        base = OE.pairs(c, u, t)
        assert 0.1 < base.mean() < 0.9
        for order in ((1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (2, 1, 0)):   # rotations keep the winding, exchanges turn it
            assert np.array_equal(OE.pairs(c, u, t[:, list(order)]), base), order
    # the order of the triangles: a permuted array gives the permuted columns, and the rows are its lowest ids
    tri = _voxel()
    V = OE.vertices(tri)
    c = V[rng.integers(0, V.shape[0], 80), 0] + F(0.25)
    u = rng.normal(0, 1.5, (80, 3, 3)).astype(F)
    over = OE.overlaps(c, u, tri)
    p = rng.permutation(V.shape[0])
    assert over.any() and np.array_equal(OE.overlaps(c, u, V[p]), over[:, p])


def test_boxes_that_are_not_live_overlap_nothing():
    tri = _voxel()
    V = OE.vertices(tri)
    mid = V.reshape(-1, 3).mean(0).astype(F)
    big = F(4) * (V.reshape(-1, 3).max(0) - V.reshape(-1, 3).min(0)).max()
    good = (np.eye(3) * big).astype(F)
    assert OE.live(mid, good)[0] and OE.overlaps(mid, good, tri).all()          # the control: this box holds everything
    dead = []
    z = good.copy(); z[1] = 0; dead.append((mid, z))                            # a zero axis
    z = good.copy(); z[2] = z[0] * F(-0.5); dead.append((mid, z))               # two parallel axes
    z = good.copy(); z[2] = z[0] + z[1]; dead.append((mid, z))                  # three coplanar axes
    z = good.copy(); z[0, 1] = np.nan; dead.append((mid, z))
    z = good.copy(); z[2, 2] = np.inf; dead.append((mid, z))
    z = mid.copy(); z[0] = np.nan; dead.append((z, good))
    z = mid.copy(); z[2] = -np.inf; dead.append((z, good))
    c, u = np.stack([d[0] for d in dead]), np.stack([d[1] for d in dead])
    assert not OE.live(c, u).any() and not OE.overlaps(c, u, tri).any()
    rows, count = OE.query(c, u, tri, 8)
    assert (rows == -1).all() and not count.any()
    assert not OE.slot_passes(c, u, np.tile(mid - big, (len(dead), 1)), np.tile(mid + big, (len(dead), 1))).any()


def test_a_triangle_that_is_not_finite_overlaps_nothing():
    c, u = np.zeros((1, 3), F), (np.eye(3) * 100).astype(F)[None]
    t = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    assert OE.pairs(c, u, t)[0]
    for v in range(3):
        for k in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                x = t.copy()
                x[0, v, k] = bad
                assert not OE.pairs(c, u, x)[0] and not OE.overlaps(c, u, x.reshape(1, 9))[0, 0]


def test_a_row_is_a_prefix_of_every_longer_one():
    tri = _voxel()
    V = OE.vertices(tri)
    rng = np.random.default_rng(2204)
    c = V[rng.integers(0, V.shape[0], 200), 0]
    u = rng.normal(0, 1.0, (200, 3, 3)).astype(F)
    rows, count = OE.query(c, u, tri, 64)
    for k in (0, 1, 5, 8, 63):
        r, n = OE.query(c, u, tri, k)
        assert np.array_equal(r, rows[:, :k]) and np.array_equal(n, count)
    assert (count > 8).any() and (count > 64).any()
    assert ((np.diff(rows, axis=1) > 0) | (rows[:, 1:] == -1)).all()   # ascending, then -1 to the end
    assert np.array_equal((rows >= 0).sum(1), np.minimum(count, 64))


def test_the_extremes_of_fp32_raise_nothing():
    """The header's bounds: from finite fp32 inputs nothing overflows, underflows to zero or is invalid -- the restatement raises on
    every numpy warning, so running it on the largest, the smallest and mixed magnitudes is the check."""
    rng = np.random.default_rng(2205)
    big, tiny = np.finfo(F).max, F(2.0) ** F(-149)
    n = 3000
    mags = np.array([big, big / F(3), F(1), F(1e-20), np.finfo(F).tiny, tiny, F(3) * tiny, F(0)], F)
    pick = lambda shape: (rng.choice(mags, shape) * rng.choice(F([-1, 1]), shape)).astype(F)
    c, u, t = pick((n, 3)), pick((n, 3, 3)), pick((n, 3, 3))
    same = rng.random(n) < 0.5                                         # one magnitude per pair, so that boxes are live and hulls pass
    m = rng.choice(mags[:-1], n)
    fit = lambda x: np.clip(x, -float(big), float(big)).astype(F)     # (twice the largest float stays the largest float)
    u[same] = fit((np.eye(3) + rng.integers(-1, 2, (n, 3, 3)))[same] * m[same, None, None].astype(np.float64))
    c[same] = fit(rng.integers(-1, 2, (n, 3))[same] * m[same, None].astype(np.float64))
    t[same] = fit(rng.integers(-2, 3, (n, 3, 3))[same] * m[same, None, None].astype(np.float64))
    got = OE.pairs(c, u, t)
    assert OE.live(c, u).sum() > n // 4 and got.sum() > n // 20 and (~got).sum() > n // 20
    lo, hi = t.min(1), t.max(1)
    assert OE.slot_passes(c, u, lo, hi)[got].all()


def test_the_gates_never_reject_an_overlapping_triangle():
    """Float inputs off the grid; half of the pairs have a vertex on a face of the box to within a rounding.  Whenever the rule says
    `overlaps`, the triangle's own bounding box and a larger box around it must pass both gates -- with no margin anywhere."""
    rng = np.random.default_rng(2206)
    n = 10000
    c1, u1, t1 = _float_pairs(rng, n)
    thin = rng.random(n) < 0.5                                         # thin boxes: their hulls are mostly empty
    u1[thin, 1:] *= F(0.05)
    # a vertex on a face to within a rounding: P = c + s0 u0 + s1 u1 + s2 u2 in fp32 with one |s_j| = 1, the rest of the triangle near P
    c2, u2, _ = _float_pairs(rng, n)
    u2[rng.random(n) < 0.5, 1:] *= F(0.05)
    s = rng.uniform(-1, 1, (n, 3)).astype(F)
    s[np.arange(n), rng.integers(0, 3, n)] = rng.choice(F([-1, 1]), n)
    corner = rng.random(n) < 0.2
    s[corner] = rng.choice(F([-1, 1]), (int(corner.sum()), 3))
    P = ((c2 + s[:, 0, None] * u2[:, 0]) + s[:, 1, None] * u2[:, 1]) + s[:, 2, None] * u2[:, 2]
    away = np.einsum("nj,njc->nc", s, u2).astype(F)                    # roughly outward
    t2 = np.stack([P, P + (away * rng.uniform(0, 1, (n, 1)) + rng.normal(0, 0.3, (n, 3))).astype(F),
                   P + (away * rng.uniform(0, 1, (n, 1)) + rng.normal(0, 0.3, (n, 3))).astype(F)], 1).astype(F)
    flat = rng.random(n) < 0.3                                         # ... or in the face's own plane
    j = np.argmax(np.abs(s) == 1, 1)
    e1, e2 = u2[np.arange(n), (j + 1) % 3], u2[np.arange(n), (j + 2) % 3]
    t2[flat, 1] = (P + e1 * rng.normal(0, 1, (n, 1)).astype(F))[flat]
    t2[flat, 2] = (P + e2 * rng.normal(0, 1, (n, 1)).astype(F))[flat]
    c, u, t = np.concatenate([c1, c2]), np.concatenate([u1, u2]), np.concatenate([t1, t2])
    t = t[:, rng.permutation(3)]
    assert c.shape[0] >= 20000
    over = OE.pairs(c, u, t)
    lo, hi = t.min(1), t.max(1)
    own = OE.slot_passes(c, u, lo, hi)
    grow_lo, grow_hi = lo - np.abs(rng.normal(0, 0.5, lo.shape)).astype(F), hi + np.abs(rng.normal(0, 0.5, hi.shape)).astype(F)
    exact = rng.random(c.shape[0]) < 0.3                               # some larger boxes share planes with the triangle's
    grow_lo[exact, 0], grow_hi[exact, 1] = lo[exact, 0], hi[exact, 1]
    larger = OE.slot_passes(c, u, grow_lo, grow_hi)
    B = OE.Boxes(c, u)
    hull = OE.hull_passes(B, lo, hi)
    print("%d pairs: %d overlap (%d of the near-face half), the gates reject %d, %d of them behind a hull that passes" % (
        c.shape[0], int(over.sum()), int(over[n:].sum()), int((~own).sum()), int((hull & ~own).sum())))
    assert over.sum() > c.shape[0] // 4 and (~over).sum() > c.shape[0] // 10
    assert 0.1 < over[n:].mean() < 0.98                                # the near-face half is decided both ways
    assert own[over].all(), "%d overlapping triangles whose own box is rejected" % int((over & ~own).sum())
    assert larger[over].all(), "%d overlapping triangles with a rejected box around them" % int((over & ~larger).sum())
    assert (~own | larger).all()                                       # a box that holds a passing box passes
    assert (hull & ~own).sum() > 100                                   # the face gate bites where the hull passes
    assert not own[~hull].any()

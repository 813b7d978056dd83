"""The yardstick of the triangle-overlap tests pinned before the device is compared with it, and the parts of the binding that need
no device (include/ezrt_tri_overlap.h, ezrt_amd/query.py: tri_overlap, tri_overlap_at).

tests/tri_overlap_expected.py restates the header's rule -- 29 separating directions -- in numpy over query triangles x all triangles.
Here it is held against a truth that owes nothing to it and is no separating-axis test: two proper triangles meet if and only if
some edge of one meets the other closed triangle, and a segment meets a triangle when the part of it in the triangle's plane (a
point, or the segment itself when it lies in the plane) clipped by the triangle's three in-plane half-planes is not empty -- in exact
arithmetic, Python ints and fractions.Fraction on small-integer pairs of every kind (generic, piercing, coplanar in axis planes and
in skew planes, parallel planes and coplanar triangles one step apart, constructed touches of every kind the header names), and in
int64 on the voxel solid of tests/inside_scenes.py against its own triangles.  Then the invariances the header promises (triangle
order, winding and vertex order of both sides, the swap of roles), the triangles that overlap nothing, the lowest-K list, and the
binding."""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


# ---- the truth, exact: Python ints and Fractions
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def segment_meets(P, Q, T):
    """the closed segment P Q meets the closed proper triangle T"""
    n = _cross(_sub(T[1], T[0]), _sub(T[2], T[0]))
    assert any(n)
    hP, hQ = _dot(n, _sub(P, T[0])), _dot(n, _sub(Q, T[0]))
    sides = []                                                      # g(X) = m . (X - a) >= 0: the in-plane half-plane of an edge
    for i in range(3):
        a, b, c = T[i], T[(i + 1) % 3], T[(i + 2) % 3]
        m = _cross(n, _sub(b, a))
        if _dot(m, _sub(c, a)) < 0:
            m = (-m[0], -m[1], -m[2])
        sides.append((m, a))
    if hP == 0 and hQ == 0:                                         # in the plane: P + t (Q - P), t in [0, 1], clipped
        t0, t1 = Fraction(0), Fraction(1)
        for m, a in sides:
            gP, gQ = _dot(m, _sub(P, a)), _dot(m, _sub(Q, a))
            if gQ == gP:
                if gP < 0:
                    return False
            elif gQ > gP:
                t0 = max(t0, Fraction(-gP, gQ - gP))
            else:
                t1 = min(t1, Fraction(gP, gP - gQ))
        return t0 <= t1
    if (hP > 0 and hQ > 0) or (hP < 0 and hQ < 0):
        return False
    t = Fraction(hP, hP - hQ)                                       # the one point of the segment in the plane
    X = tuple(p + t * (q - p) for p, q in zip(P, Q))
    return all(_dot(m, _sub(X, a)) >= 0 for m, a in sides)


def edges_meet(T, U):
    """some edge of T meets U"""
    return any(segment_meets(T[i], T[(i + 1) % 3], U) for i in range(3))


def truth(T, U):
    T, U = [tuple(int(x) for x in v) for v in T], [tuple(int(x) for x in v) for v in U]
    return edges_meet(T, U) or edges_meet(U, T)


def _proper(T):
    return np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]).any(1)


def _random_proper(rng, n, draw):
    T = draw(n)
    while not _proper(T).all():
        bad = ~_proper(T)
        T[bad] = draw(int(bad.sum()))
    return T


BASES = [((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0)),                       # axis planes
         ((1, 0, 1), (0, 1, -1)), ((1, 1, 0), (0, 1, 1)), ((1, -1, 0), (1, 0, 1)), ((1, 1, 1), (-1, 1, 0))]   # skew planes


def _in_plane(rng, st, base, origin):
    """integer points origin + s u + t v for st [..., 2]"""
    u, v = np.array(BASES[base][0]), np.array(BASES[base][1])
    return origin + st[..., :1] * u + st[..., 1:] * v


def _coplanar(rng, n, skew):
    """(Q, S, base, origin): random proper triangles in one plane, s and t in -2 .. 2"""
    base = rng.integers(3, 7, n) if skew else rng.integers(0, 3, n)
    origin = rng.integers(-1, 2, (n, 3)) * (0 if skew else 1)
    out = []
    for _ in range(2):
        T = np.zeros((n, 3, 3), int)
        for i in range(n):
            while True:
                t = _in_plane(rng, rng.integers(-2, 3, (3, 2)), base[i], origin[i])
                if _proper(t[None])[0]:
                    break
            T[i] = t
        out.append(T)
    return out[0], out[1], base, origin


def _normal_of(base):
    return np.cross(BASES[base][0], BASES[base][1])


def _kinds(rng, per):
    """{kind: (Q, S)} integer arrays [per, 3, 3]"""
    kinds = {}
    draw = lambda n: rng.integers(-4, 5, (n, 3, 3))
    kinds["generic"] = (_random_proper(rng, per, draw), _random_proper(rng, per, draw))
    # piercing: a large scene triangle in an axis plane and a small query near its middle, kept where no edge of the scene
    # triangle meets the query -- the query's edges alone decide
    Q, S = [], []
    while len(Q) < per:
        c = rng.integers(0, 3)
        big = np.array([[-4, -4, 0], [4, -4, 0], [0, 4, 0]])
        big = np.roll(big, c, axis=1)
        big[:, (2 + c) % 3] = rng.integers(-1, 2)                     # (the rolled zero column: the plane's own coordinate)
        q = _random_proper(rng, 1, lambda n: rng.integers(-2, 3, (n, 3, 3)))[0]
        if not edges_meet([tuple(map(int, v)) for v in big], [tuple(map(int, v)) for v in q]):
            Q.append(q)
            S.append(big)
    kinds["piercing"] = (np.stack(Q), np.stack(S))
    for name, skew in (("coplanar_axis", False), ("coplanar_skew", True)):
        Q, S, base, origin = _coplanar(rng, per, skew)
        kinds[name] = (Q, S)
        # the same pairs with the scene triangle moved one step off the plane: parallel planes, never an overlap
        step = np.stack([np.eye(3, dtype=int)[int(np.argmax(np.abs(_normal_of(b))))] for b in base])
        kinds["parallel_" + name] = (Q, S + step[:, None, :] * rng.choice([-1, 1], (per, 1, 1)))
    # nested, in every plane: (-2, -2) (2, -2) (-2, 2) holds (-1, -1) (0, -1) (-1, 0)
    base = rng.integers(0, 7, per)
    outer = np.stack([_in_plane(rng, np.array([[-2, -2], [2, -2], [-2, 2]]), b, 0) for b in base])
    inner = np.stack([_in_plane(rng, np.array([[-1, -1], [0, -1], [-1, 0]]), b, 0) for b in base])
    flip = rng.random(per) < 0.5
    kinds["nested"] = (np.where(flip[:, None, None], outer, inner), np.where(flip[:, None, None], inner, outer))
    # coplanar, one step apart: pairs that share an edge or a vertex, one of them moved by one in-plane step
    Q, S = [], []
    for i in range(per):
        b = rng.integers(0, 7)
        s = np.array([[0, 0], [2, 0], [0, 2]])
        q = np.array([[0, 0], [2, 0], [1, -2]]) if i % 2 else np.array([[0, 0], [-1, -2], [-2, -1]])
        move = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [1, -1], [-1, 1]])[rng.integers(0, 6)]
        Q.append(_in_plane(rng, q + move, b, 0))
        S.append(_in_plane(rng, s, b, 0))
    kinds["coplanar_step"] = (np.stack(Q), np.stack(S))
    for k, (Q, S) in kinds.items():                                   # any vertex order, any winding, on both sides
        kinds[k] = (np.stack([t[rng.permutation(3)] for t in Q]), np.stack([t[rng.permutation(3)] for t in S]))
    return kinds


BOTH = ("generic", "piercing", "coplanar_axis", "coplanar_skew", "coplanar_step")     # kinds where both answers can occur
ONLY = {"parallel_coplanar_axis": False, "parallel_coplanar_skew": False, "nested": True}


def _touching(rng, per):
    """{kind: (Q, S, away)}: pairs constructed to touch only; Q moved by `away` no longer meets S"""
    out = {}
    names = ("vertex_on_face", "vertex_on_edge", "vertex_on_vertex", "edges_cross", "coplanar_share_edge", "coplanar_share_point")
    for name in names:
        Q, S, W = [], [], []
        for _ in range(per):
            b = rng.integers(0, 7)
            u, v = np.array(BASES[b][0]), np.array(BASES[b][1])
            w = np.cross(u, v)
            o = rng.integers(-1, 2, 3)
            at = lambda s, t, h=0: o + s * u + t * v + h * w
            s_tri = [at(0, 0), at(3, 0), at(0, 3)]
            up = lambda: at(int(rng.integers(-1, 3)), int(rng.integers(-1, 3)), int(rng.integers(1, 3)))   # strictly above the plane
            if name == "vertex_on_face":
                q, away = [at(1, 1), up(), up()], w
            elif name == "vertex_on_edge":
                q, away = [at(2, 0), up(), up()], w
            elif name == "vertex_on_vertex":
                q, away = [at(3, 0), up(), up()], w
            elif name == "edges_cross":                               # the query's edge runs through (1, 0) on the edge t = 0: from above
                # the plane and outside to below it; its third vertex is outside too, so the point is all they share
                q, away = [at(1, -1, 1), at(1, 1, -1), at(2, -3, 1)], -v
            elif name == "coplanar_share_edge":
                q, away = [at(0, 0), at(3, 0), at(1, -2)], -v
            else:
                q, away = [at(0, 0), at(-1, -2), at(-2, -1)], -v
            while not _proper(np.array([q]))[0]:
                q[1], q[2] = up(), up()
            p1, p2 = rng.permutation(3), rng.permutation(3)
            Q.append(np.array(q)[p1])
            S.append(np.array(s_tri)[p2])
            W.append(away)
        out[name] = (np.stack(Q), np.stack(S), np.stack(W))
    return out


@pytest.fixture(scope="module")
def small_pairs():
    rng = np.random.default_rng(2017)
    kinds = _kinds(rng, 600)
    return {k: (Q, S, np.array([truth(q, s) for q, s in zip(Q, S)]), TE.pairs(Q.astype(np.float32), S.astype(np.float32)))
            for k, (Q, S) in kinds.items()}


def test_equals_exact_truth_on_small_integer_pairs(small_pairs):
    total = 0
    for kind, (Q, S, want, got) in small_pairs.items():
        assert _proper(Q).all() and _proper(S).all(), kind
        wrong = got != want
        assert not wrong.any(), "%s: %d of %d pairs differ from the exact truth, first: %s against %s (truth %s)" % (
            kind, int(wrong.sum()), wrong.size, Q[np.argmax(wrong)].tolist(), S[np.argmax(wrong)].tolist(), want[np.argmax(wrong)])
        total += want.size
        if kind in BOTH:
            assert want.sum() >= 30 and (~want).sum() >= 30, (kind, int(want.sum()))          # both answers occur
            gate = TE.t1(Q.astype(np.float32), S.astype(np.float32))
            assert (~want & gate).sum() >= 15, kind                                            # T2 decides, not T1 alone
        else:
            assert (want == ONLY[kind]).all(), kind                                            # the one answer this kind can have
    assert set(BOTH) | set(ONLY) == set(small_pairs) and total == 8 * 600     # eight kinds of 600 pairs
    Q, S, want, got = small_pairs["piercing"]                           # as labelled: no edge of the scene triangle meets the query
    assert not any(edges_meet([tuple(map(int, v)) for v in s], [tuple(map(int, v)) for v in q]) for q, s in zip(Q[:100], S[:100]))


def test_constructed_touches():
    rng = np.random.default_rng(2018)
    n = 0
    for kind, (Q, S, away) in _touching(rng, 50).items():
        want = np.array([truth(q, s) for q, s in zip(Q, S)])
        assert want.all(), kind                                                                 # constructed to touch, and they do
        moved = Q + away[:, None, :]
        assert not any(truth(q, s) for q, s in zip(moved, S)), kind                             # ... only: one step away they are apart
        assert TE.pairs(Q.astype(np.float32), S.astype(np.float32)).all(), kind
        assert not TE.pairs(moved.astype(np.float32), S.astype(np.float32)).any(), kind
        assert TE.pairs(S.astype(np.float32), Q.astype(np.float32)).all(), kind                 # roles swapped
        n += Q.shape[0]
    assert n >= 300


# ---- the truth again, vectorised in int64 for the voxel solid: the same edge-against-triangle test with the divisions multiplied
# out.  `peak` collects the largest magnitude of every intermediate.
def _vcross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _vdot(a, b):
    return (a * b).sum(1)


def _segment_meets_i64(P, Q, T, peak):
    def seen(x):
        peak.append(int(np.abs(x).max()) if x.size else 0)
        return x
    n = seen(_vcross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    hP, hQ = seen(_vdot(n, P - T[:, 0])), seen(_vdot(n, Q - T[:, 0]))
    flat = (hP == 0) & (hQ == 0)
    crossing = ~flat & ~((hP > 0) & (hQ > 0)) & ~((hP < 0) & (hQ < 0))
    s = np.sign(hP - hQ)
    one, nought = np.ones_like(hP), np.zeros_like(hP)
    lower, upper = [(nought, one)], [(one, one)]                      # t >= 0 / 1, t <= 1 / 1: (numerator, positive denominator)
    feasible = np.ones(hP.shape, bool)
    for i in range(3):
        a, b, c = T[:, i], T[:, (i + 1) % 3], T[:, (i + 2) % 3]
        m = _vcross(n, b - a)
        m = seen(m * np.sign(_vdot(m, c - a))[:, None])
        gP, gQ = seen(_vdot(m, P - a)), seen(_vdot(m, Q - a))
        crossing &= s * seen(hP * gQ - hQ * gP) >= 0                  # g at the point of the plane, times |hP - hQ|
        dg = gQ - gP
        feasible &= ~((dg == 0) & (gP < 0))
        lower.append((np.where(dg > 0, -gP, nought), np.where(dg > 0, dg, one)))
        upper.append((np.where(dg < 0, gP, one), np.where(dg < 0, -dg, one)))
    for ln, ld in lower:
        for un, ud in upper:
            feasible &= seen(ln * ud) <= seen(un * ld)
    return np.where(flat, feasible, crossing)


def truth_i64(T, U, peak):
    out = np.zeros(T.shape[0], bool)
    for X, Y in ((T, U), (U, T)):
        for i in range(3):
            out |= _segment_meets_i64(X[:, i], X[:, (i + 1) % 3], Y, peak)
    return out


def test_int64_truth_equals_the_fraction_truth(small_pairs):
    for kind, (Q, S, want, got) in small_pairs.items():
        assert np.array_equal(truth_i64(Q.astype(np.int64), S.astype(np.int64), []), want), kind


@pytest.fixture(scope="module")
def solid():
    v = IS.voxel_solid()
    P = TE.vertices(v["tri"])
    return dict(tri=v["tri"], P=P, over=TE.overlaps(P.reshape(-1, 9), v["tri"]))   # computed once


def test_voxel_solid_against_itself(solid):
    P, over = solid["P"], solid["over"]
    m = P.shape[0]
    assert over.shape == (m, m) and TE.live(P).all()
    I = P.astype(np.int64)
    assert np.array_equal(I.astype(np.float32), P)                  # integer coordinates
    # a triangle overlaps itself and every triangle that shares a vertex with it
    shares = (P[:, None, :, None, :] == P[None, :, None, :, :]).all(-1).any((2, 3))
    assert shares[np.arange(m), np.arange(m)].all() and over[shares].all() and shares.sum() > 8 * m
    # pairs whose closed integer bounding boxes are disjoint share no point (integer comparisons); the others: the int64 truth
    near = ((I.min(1)[:, None] <= I.max(1)[None]) & (I.min(1)[None] <= I.max(1)[:, None])).all(-1)
    assert not over[~near].any()
    i, k = np.nonzero(near)
    peak = []
    want = truth_i64(I[i], I[k], peak)
    # the magnitudes fit: coordinates 0 .. 7, so |n| <= 2 * 7^2, |h| and |m| <= 3 * 7 * |n|, |g| <= 3 * 7 * |m| and the products
    # of two of them stay below 2^40
    assert I.min() >= 0 and I.max() <= IS.G and max(peak) < 2 ** 40
    assert np.array_equal(over[i, k], want) and want.any() and not want.all()
    assert not (over & ~shares).any()                               # faces of a grid meet in grid points only: nothing else touches
    assert np.array_equal(over, over.T)


def _rotated(P):
    ang = 0.37
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.6), -np.sin(0.6)], [0, np.sin(0.6), np.cos(0.6)]])
    return (P.astype(np.float64) @ R.T).astype(np.float32)


def _shuffled(T, rng, how):
    if how == "winding":
        return T[:, ::-1]
    if how == "rolled":
        return np.stack([np.roll(t, int(r), axis=0) for t, r in zip(T, rng.integers(0, 3, T.shape[0]))])
    return np.stack([t[rng.permutation(3)] for t in T])


def test_order_winding_vertex_order_and_roles_do_not_matter(solid):
    rng = np.random.default_rng(7)
    P = solid["P"]
    m = P.shape[0]
    # queries: the scene's own triangles and copies moved a little, so that they cut their neighbours
    sel = rng.integers(0, m, 300)
    for name, S in (("grid", P), ("rotated", _rotated(P))):
        size = np.float32(1.0)
        Q = S[sel] + np.where(rng.random((300, 1, 1)) < 0.3, 0, rng.normal(0, 0.3 * size, (300, 1, 3))).astype(np.float32)
        if name == "grid":
            Q = np.round(Q * 2) / np.float32(2)                      # on the half grid: still exact
        base = TE.overlaps(Q.reshape(-1, 9), S)
        assert base.any(1).sum() > 100 and base.sum(1).max() > 8 and not base.all(), name
        perm = rng.permutation(m)
        assert np.array_equal(TE.overlaps(Q.reshape(-1, 9), S[perm])[:, np.argsort(perm)], base), name    # ids mapped back
        for how in ("winding", "rolled", "permuted"):
            assert np.array_equal(TE.overlaps(Q.reshape(-1, 9), _shuffled(S, rng, how)), base), (name, how)
            assert np.array_equal(TE.overlaps(_shuffled(Q, rng, how).reshape(-1, 9), S), base), (name, how)
        assert np.array_equal(TE.overlaps(S.reshape(-1, 9), Q).T, base), name                              # the roles swapped
    off = _rotated(P)
    assert np.array_equal(TE.overlaps(off.reshape(-1, 9), off), TE.overlaps(off.reshape(-1, 9), off).T)


def test_triangles_that_overlap_nothing():
    one = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[5, 5, 5], [6, 5, 5], [5, 6, 7]]])
    big = np.float32([[-2, -2, -3], [9, 9, -3], [4, 4, 20]])         # in the plane x = y: cuts both
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                 # no warning from numpy anywhere below
        assert TE.overlaps(big.reshape(1, 9), one).tolist() == [[True, True]]
        assert TE.overlaps(one.reshape(2, 9), big[None]).tolist() == [[True], [True]]
        for bad in (np.nan, np.inf, -np.inf):
            for v in range(3):
                for c in range(3):
                    q = big.copy()
                    q[v, c] = bad
                    assert not TE.overlaps(q.reshape(1, 9), one).any(), (bad, v, c)                  # in the query
                    assert not TE.live(q[None])[0]
                    t = one.copy()
                    t[0, v, c] = bad
                    assert TE.overlaps(big.reshape(1, 9), t).tolist() == [[False, True]], (bad, v, c)   # in the scene
        # collinear and repeated vertices, on either side: not a segment, not a point -- nothing
        a, b = np.float32([0, 0, 0]), np.float32([1, 0, 0])
        flat = [np.stack([a, b, b + b]), np.stack([a, a, b]), np.stack([b, a, b]), np.stack([a, b, b]), np.stack([a, a, a]),
                np.float32([[0.1, 0.2, 0.3], [0.2, 0.4, 0.6], [0.4, 0.8, 1.2]])]
        for t in flat:
            assert not TE.live(t[None])[0]
            assert not TE.overlaps(t.reshape(1, 9), one).any() and not TE.overlaps(t.reshape(1, 9), t[None]).any()
            assert TE.overlaps(one.reshape(2, 9), np.concatenate([t[None], one])).tolist() == [[False, True, False], [False, False, True]]
        # the largest and the smallest finite triangles take part, and nothing overflows or underflows to a wrong zero
        huge = np.float32([[FLT_MAX, -FLT_MAX, 0], [-FLT_MAX, FLT_MAX, FLT_MAX], [FLT_MAX, FLT_MAX, -FLT_MAX]])
        tiny = np.float32([[1e-45, 0, 0], [0, 1e-45, 0], [0, 0, -1e-45]])
        assert TE.live(np.stack([huge, tiny])).all()
        assert TE.overlaps(huge.reshape(1, 9), np.stack([huge, tiny])).tolist() == [[True, False]]
        assert TE.overlaps(tiny.reshape(1, 9), np.stack([huge, tiny])).tolist() == [[False, True]]
        through = np.float32([[-FLT_MAX, -FLT_MAX, 0], [FLT_MAX, -FLT_MAX, 0], [0, FLT_MAX, 0]])   # the plane z = 0, through `tiny`
        assert TE.overlaps(through.reshape(1, 9), np.stack([tiny, one[0], one[1]])).tolist() == [[True, True, False]]


def _rows(over):
    return [np.nonzero(r)[0] for r in over]


def test_lowest_k_list(solid):
    tri, P, over = solid["tri"], solid["P"], solid["over"]
    m = P.shape[0]
    G = IS.G
    cut = np.float32([[-1, -1, 3], [2 * G, -1, 3], [-1, 2 * G, 3]])   # the grid plane z = 3 through the whole solid
    far = np.float32([[20, 20, 20], [21, 20, 20], [20, 21, 20]])
    dead = np.float32([[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]])
    c = P[0].mean(0)                                                # a small triangle through the middle of triangle 0 alone
    nrm = np.cross(P[0, 1] - P[0, 0], P[0, 2] - P[0, 0])
    poke = np.float32([c - 0.1 * nrm, c + 0.1 * nrm, c + 0.05 * nrm[[1, 2, 0]]])
    Q = np.concatenate([P, poke[None], cut[None], far[None], dead[None]]).reshape(-1, 9)
    full, count = TE.query(Q, tri, 64)
    assert count[-3] > 64 and count[-2] == 0 and count[-1] == 0 and (full[-2:] == -1).all()
    assert np.array_equal(count[:m], over.sum(1)) and count[m] == 1 and full[m, 0] == 0 and (count > 8).any()
    for k in (1, 3, 8, 64):
        rows, cnt = TE.query(Q, tri, k)
        assert rows.shape == (Q.shape[0], k) and rows.dtype == np.int32 and np.array_equal(cnt, count)      # n_overlap independent of K
        assert np.array_equal(rows, full[:, :k])                                   # a K-row is a prefix of every longer one
        used = np.minimum(cnt, k)
        for r, u, o in zip(rows[:m], used[:m], _rows(over)):
            assert np.array_equal(r[:u], o[:u]) and (r[u:] == -1).all()            # the lowest ids, ascending, then -1
    assert (np.diff(full[-3]) > 0).all() and full[-3, 0] >= 0                      # count above K: 64 ids, ascending
    rows0, cnt0 = TE.query(Q, tri, 0)
    assert rows0.shape == (Q.shape[0], 0) and np.array_equal(cnt0, count)
    # the _at form: the pairs of the rows are overlaps, ids outside the scene are not
    ids = np.concatenate([full[:, 0], [m, -1, 2 ** 31 - 1]]).astype(np.int64)
    got = TE.at(np.concatenate([Q, np.repeat(cut.reshape(1, 9), 3, 0)]), tri, ids)
    assert np.array_equal(got[:-3].astype(bool), full[:, 0] >= 0) and not got[-3:].any()


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi, query
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ezrt_tri_overlap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.TRI_OVERLAP_ABI) == ["ezrt_query_tri_overlap_device", "ezrt_tri_overlap_at_device"]
    assert int(re.search(r"#define\s+EZRT_TRI_OVERLAP_MAX\s+(\d+)", src).group(1)) == _abi.TRI_OVERLAP_MAX == 64
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.TRI_OVERLAP_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "NEAREST_ABI", "INSIDE_ABI", "BOX_OVERLAP_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other
    assert callable(query.tri_overlap) and callable(query.tri_overlap_at)
    assert query.TriOverlap._fields == ("tri", "n_overlap")


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    tris = torch.zeros((4, 9), dtype=torch.float32)
    for k in (65, -1, 1.0, True, None, "8"):
        with pytest.raises(ValueError, match="max_k must be an int"):
            query.tri_overlap(None, tris, k)
    with pytest.raises(ValueError, match="count=True"):
        query.tri_overlap(None, tris, 0)
    for arg in (tris, np.zeros((4, 9), np.float32)):
        with pytest.raises(TypeError, match="GPU tensor"):
            query.tri_overlap(None, arg)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.tri_overlap(None, arg, max_k=0, count=True)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.tri_overlap_at(None, arg, torch.zeros(4, dtype=torch.int32))

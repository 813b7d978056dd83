"""The yardstick of the self-overlap tests pinned before the device is compared with it, and the parts of the binding that need no
device (include/ezrt_self_overlap.h, ezrt_amd/query.py: self_overlap, self_overlap_at).

tests/self_overlap_expected.py restates the header's rule -- the count s of vertices shared by value, then T2, two segment tests,
the fold test or true -- in numpy.  Here it is held against a truth that does not follow that case analysis and is no
separating-axis test: the intersection of two closed triangles is convex, and its extreme points are among the CANDIDATES -- every
vertex of one that lies in the other, every point where two edges that are not parallel cross, every point where an edge pierces
the other triangle's plane inside that triangle.  The triangles cross when some candidate lies outside the convex hull of the
vertices they share (nothing, a point, a segment; with three shared vertices they cross by definition).  All of it in exact
arithmetic, fractions.Fraction on the float32 values: small integer pairs of every kind, the voxel solid of tests/inside_scenes.py
(which crosses itself nowhere) and the same solid with constructed defects (tests/self_overlap_scenes.py).  Then the invariances the
header promises, the triangles that cross nothing, and the binding."""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import self_overlap_expected as SE  # noqa: E402
import self_overlap_scenes as SS  # noqa: E402
import test_tri_overlap_expected as TT  # noqa: E402  (its generators of pairs that share nothing)
import tri_overlap_expected as TE  # noqa: E402

SEED = 2031                # checked on the CPU: every kind where both answers can occur has both in at least a fifth of its pairs
PER = 300


# ---- the truth, exact
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _along(P, r, t):
    return (P[0] + t * r[0], P[1] + t * r[1], P[2] + t * r[2])


def in_triangle(X, T, n):
    """the point X lies in the closed proper triangle T with normal n"""
    if _dot(n, _sub(X, T[0])) != 0:
        return False
    return all(_dot(_cross(_sub(T[(i + 1) % 3], T[i]), _sub(X, T[i])), n) >= 0 for i in range(3))


def candidates(T, U):
    """points that hold every extreme point of the intersection of the closed proper triangles T and U"""
    nT, nU = _cross(_sub(T[1], T[0]), _sub(T[2], T[0])), _cross(_sub(U[1], U[0]), _sub(U[2], U[0]))
    assert any(nT) and any(nU)
    for A, B, nB in ((T, U, nU), (U, T, nT)):
        for X in A:                                                   # a vertex in the other triangle
            if in_triangle(X, B, nB):
                yield X
        for i in range(3):                                            # an edge through the other triangle's plane
            P, Q = A[i], A[(i + 1) % 3]
            hP, hQ = _dot(nB, _sub(P, B[0])), _dot(nB, _sub(Q, B[0]))
            if hP != hQ:
                t = Fraction(hP) / Fraction(hP - hQ)
                if 0 <= t <= 1:
                    X = _along(P, _sub(Q, P), t)
                    if in_triangle(X, B, nB):
                        yield X
    for i in range(3):                                                # two edges that are not parallel and cross
        P, r = T[i], _sub(T[(i + 1) % 3], T[i])
        for j in range(3):
            Q, s = U[j], _sub(U[(j + 1) % 3], U[j])
            x = _cross(r, s)
            w = _sub(Q, P)
            if not any(x) or _dot(w, x) != 0:
                continue
            xx = Fraction(_dot(x, x))
            t, u = _dot(_cross(w, s), x) / xx, _dot(_cross(w, r), x) / xx
            if 0 <= t <= 1 and 0 <= u <= 1:
                yield _along(P, r, t)


def truth(T, U):
    """the proper triangles T, U [3][3] (numbers that Fraction takes exactly) share a point outside the hull of their shared vertices"""
    T, U = [tuple(Fraction(float(x)) for x in v) for v in T], [tuple(Fraction(float(x)) for x in v) for v in U]
    both = [v for v in T if v in U]
    if len(both) == 3:
        return True
    for X in candidates(T, U):
        if not both:
            return True
        if len(both) == 1:
            if X != both[0]:
                return True
        else:
            e, d = _sub(both[1], both[0]), _sub(X, both[0])
            if any(_cross(d, e)) or not 0 <= _dot(d, e) <= _dot(e, e):
                return True
    return False


# ---- pairs by kind
def _proper(T):
    return TT._proper(T)


def _plane_points(base, st, origin=0):
    u, v = np.array(TT.BASES[base][0]), np.array(TT.BASES[base][1])
    st = np.asarray(st)
    return origin + st[..., :1] * u + st[..., 1:] * v


def _shares(I, J):
    return int(sum(any((v == w).all() for w in J) for v in I))


def _draw(rng, per, make, s):
    """per pairs from make() that are proper and share exactly s vertices"""
    I, J = [], []
    while len(I) < per:
        i, j = make()
        i, j = np.asarray(i), np.asarray(j)
        if _proper(i[None])[0] and _proper(j[None])[0] and _shares(i, j) == s:
            I.append(i)
            J.append(j)
    return np.stack(I), np.stack(J)


RING = np.array([[4, 0, 0], [3, 3, 0], [0, 4, 0], [-3, 3, 0], [-4, 0, 0], [-3, -3, 0], [0, -4, 0], [3, -3, 0]])


def _kinds(rng, per):
    """{kind: (I, J)} integer arrays [per, 3, 3]"""
    kinds = {}
    old = TT._kinds(rng, per)
    for name, src in (("s0_generic", "generic"), ("s0_coplanar_axis", "coplanar_axis"), ("s0_coplanar_skew", "coplanar_skew")):
        I, J = old[src]
        keep = np.array([_shares(i, j) == 0 for i, j in zip(I, J)])
        kinds[name] = (I[keep], J[keep])

    def umbrella():                                                   # two sectors of a fan about v that are not neighbours
        ring = RING + np.concatenate([np.zeros((8, 2), int), rng.integers(-1, 2, (8, 1))], 1)
        v = np.array([0, 0, int(rng.integers(1, 3))])
        i = int(rng.integers(0, 8))
        j = (i + int(rng.integers(2, 7))) % 8
        roll, off = int(rng.integers(0, 3)), rng.integers(-1, 2, 3)
        f = lambda t: np.roll(np.array(t), roll, axis=1) + off
        return f([v, ring[i], ring[(i + 1) % 8]]), f([v, ring[j], ring[(j + 1) % 8]])
    kinds["s1_umbrella"] = _draw(rng, per, umbrella, 1)

    def piercing():
        v = rng.integers(-2, 3, 3)
        a, b = rng.integers(-4, 5, (2, 3))
        if rng.random() < 0.5:
            return [v, a, b], [v, *rng.integers(-4, 5, (2, 3))]
        mid, w = (v + a + b) // 3, rng.integers(-2, 3, 3)               # J's far edge runs through the middle of I, or near it
        return [v, a, b], [v, mid + w, mid - w + rng.integers(-1, 2, 3)]
    kinds["s1_piercing"] = _draw(rng, per, piercing, 1)

    def fan():                                                        # coplanar, about a shared vertex
        b, o = int(rng.integers(0, 7)), rng.integers(-1, 2, 3)
        v = rng.integers(-1, 2, 2)
        i, j = rng.integers(-3, 4, (2, 2)), rng.integers(-3, 4, (2, 2))
        return _plane_points(b, [v, *i], o), _plane_points(b, [v, *j], o)
    kinds["s1_coplanar_fan"] = _draw(rng, per, fan, 1)

    def touch():                                                      # J's vertex on, or J's edge through, the edge of I opposite v
        v = rng.integers(-2, 3, 3)
        a = rng.integers(-3, 4, 3)
        b = a + 2 * rng.integers(-2, 3, 3)
        mid = (a + b) // 2
        if rng.random() < 0.5:
            return [v, a, b], [v, mid, rng.integers(-5, 6, 3)]
        w = rng.integers(-2, 3, 3)
        return [v, a, b], [v, mid + w, mid - w]
    kinds["s1_touch"] = _draw(rng, per, touch, 1)

    def dihedral():
        u, v = rng.integers(-3, 4, 3), rng.integers(-3, 4, 3)
        a, b = rng.integers(-4, 5, 3), rng.integers(-4, 5, 3)
        if np.dot(np.cross(v - u, a - u), b - u) == 0:
            b = u                                                     # (coplanar: rejected as improper)
        return [u, v, a], [b, u, v]
    kinds["s2_dihedral"] = _draw(rng, per, dihedral, 2)

    def flat(same):
        def make():
            bse, o = int(rng.integers(0, 7)), rng.integers(-1, 2, 3)
            u, v = rng.integers(-2, 3, 2), rng.integers(-2, 3, 2)
            a, b = rng.integers(-3, 4, 2), rng.integers(-3, 4, 2)
            side = lambda x: np.sign((v[0] - u[0]) * (x[1] - u[1]) - (v[1] - u[1]) * (x[0] - u[0]))
            if side(a) * side(b) != (1 if same else -1):
                b = u
            return _plane_points(bse, [u, v, a], o), _plane_points(bse, [v, b, u], o)
        return make
    kinds["s2_opposite"] = _draw(rng, per, flat(False), 2)
    kinds["s2_folded"] = _draw(rng, per, flat(True), 2)

    def twin():
        t = rng.integers(-6, 7, (3, 3))
        return t, t[rng.permutation(3)]
    kinds["s3"] = _draw(rng, per, twin, 3)
    for k, (I, J) in kinds.items():                                   # any vertex order, any winding, on both sides
        kinds[k] = (np.stack([t[rng.permutation(3)] for t in I]), np.stack([t[rng.permutation(3)] for t in J]))
    return kinds


BOTH = ("s0_generic", "s0_coplanar_axis", "s0_coplanar_skew", "s1_piercing", "s1_coplanar_fan")     # both answers can occur
ONLY = {"s1_umbrella": False, "s1_touch": True, "s2_dihedral": False, "s2_opposite": False, "s2_folded": True, "s3": True}
SHARED = {"s0": 0, "s1": 1, "s2": 2, "s3": 3}


@pytest.fixture(scope="module")
def small_pairs():
    rng = np.random.default_rng(SEED)
    return {k: (I, J, np.array([truth(i, j) for i, j in zip(I, J)]), SE.pairs(I.astype(np.float32), J.astype(np.float32)))
            for k, (I, J) in _kinds(rng, PER).items()}


def test_equals_exact_truth_on_small_integer_pairs(small_pairs):
    assert set(BOTH) | set(ONLY) == set(small_pairs)
    for kind, (I, J, want, got) in small_pairs.items():
        assert _proper(I).all() and _proper(J).all() and np.abs(I).max() <= 8 and np.abs(J).max() <= 8, kind
        assert (SE.shared_count(I.astype(np.float32), J.astype(np.float32)) == SHARED[kind[:2]]).all(), kind
        wrong = got != want
        assert not wrong.any(), "%s: %d of %d pairs differ from the exact truth, first: %s against %s (truth %s)" % (
            kind, int(wrong.sum()), wrong.size, I[np.argmax(wrong)].tolist(), J[np.argmax(wrong)].tolist(), want[np.argmax(wrong)])
        if kind in BOTH:
            assert want.size >= 200 and min(want.sum(), (~want).sum()) * 5 >= want.size, (kind, int(want.sum()), want.size)
        else:
            assert want.size == PER and (want == ONLY[kind]).all(), kind
        # the roles swapped: the same answer
        assert np.array_equal(SE.pairs(J.astype(np.float32), I.astype(np.float32)), got), kind
    # the triangle rule says "overlap" for every pair that shares a vertex: what the new rule is for
    for kind in ONLY:
        I, J = small_pairs[kind][:2]
        assert TE.pairs(I.astype(np.float32), J.astype(np.float32)).all(), kind


def test_truth_agrees_with_the_triangle_tests_truth_where_nothing_is_shared(small_pairs):
    for kind in ("s0_generic", "s0_coplanar_axis", "s0_coplanar_skew"):
        I, J, want, got = small_pairs[kind]
        assert np.array_equal(np.array([TT.truth(i, j) for i, j in zip(I, J)]), want), kind


# ---- the voxel solid, and the solid with defects
def _near(P):
    lo, hi = P.min(1), P.max(1)
    return ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all(-1)


def _truth_matrix(P):
    """bool [m, m]: the Fraction truth of every pair whose closed bounding boxes meet (the others share no point), each pair once"""
    m = P.shape[0]
    out = np.zeros((m, m), bool)
    T = [[tuple(Fraction(float(x)) for x in v) for v in t] for t in P]
    i, k = np.nonzero(np.triu(_near(P), 1))
    for a, b in zip(i.tolist(), k.tolist()):
        out[a, b] = out[b, a] = truth(T[a], T[b])
    return out


@pytest.fixture(scope="module")
def solid():
    v = IS.voxel_solid()
    return dict(tri=v["tri"], P=TE.vertices(v["tri"]), cross=SE.crosses(v["tri"]))


@pytest.fixture(scope="module")
def defects():
    s = SS.defect_scene()
    return dict(s, cross=SE.crosses(s["tri"]))


def test_voxel_solid_crosses_itself_nowhere(solid):
    P, cross = solid["P"], solid["cross"]
    m = P.shape[0]
    assert TE.live(P).all() and cross.shape == (m, m)
    assert not cross.any()                                            # count 0 for every triangle
    over = TE.overlaps(P.reshape(-1, 9), solid["tri"])
    over[np.arange(m), np.arange(m)] = False
    assert (over.sum(1) > 0).all() and over.sum(1).min() >= 8        # the triangle rule, own id dropped: neighbours in every row
    s = SE.shared_count(np.repeat(P, m, 0), np.tile(P, (m, 1, 1))).reshape(m, m)
    assert (s[over] >= 1).all() and {1, 2} <= set(s[over].tolist())   # ... all of them shared by value
    near = _near(P)                                                   # the Fraction truth on a fifth of the rows
    assert not any(truth(P[i], P[k]) for i in range(0, m, 5) for k in np.nonzero(near[i])[0] if k != i)


def test_defect_scene_equals_the_exact_truth(defects):
    P, cross, copy, m = defects["P"], defects["cross"], defects["copy"], defects["m"]
    n = P.shape[0]
    assert n == 2 * m + 9 and n < 1000 and TE.live(P).all()
    want = _truth_matrix(P)
    assert np.array_equal(cross, want)
    assert np.array_equal(cross, cross.T) and not cross.diagonal().any()
    count = cross.sum(1)
    assert (count > 64).sum() >= 2 and (count == 0).any() and ((count > 0) & (count <= 64)).sum() > n // 4
    i, k = np.nonzero(cross)
    s = SE.shared_count(P[i], P[k])
    assert set(s.tolist()) == {0, 1, 2, 3}                            # every case contributes a crossing
    plain = defects["plain"]
    assert not cross[np.ix_(plain, plain)].any() and not cross[np.ix_(copy, copy)].any()     # each solid alone: nothing
    assert cross[np.ix_(plain, copy)].any()
    moved = TE.vertices(SS.moved_clear())
    clear = SE.crosses(SS.moved_clear())
    assert not clear[np.ix_(plain, copy)].any() and clear[~copy][:, ~copy].sum() == cross[~copy][:, ~copy].sum()
    sub = np.nonzero(copy)[0][::7]                                    # the truth of the moved scene on some rows of the copy
    assert all(clear[a, b] == (a != b and bool(_near(moved[[a, b]])[0, 1]) and truth(moved[a], moved[b])) for a in sub for b in range(n))


def test_lowest_k_list(defects):
    tri, cross = defects["tri"], defects["cross"]
    n = cross.shape[0]
    full, count = SE.rows_of(cross, None, 64)
    assert np.array_equal(count, cross.sum(1)) and (count > 64).any()
    for k in (1, 3, 8, 64):
        rows, cnt = SE.rows_of(cross, None, k)
        assert rows.shape == (n, k) and rows.dtype == np.int32 and np.array_equal(cnt, count)
        assert np.array_equal(rows, full[:, :k])                      # a K-row is a prefix of every longer one
        for r, u, o in zip(rows, np.minimum(cnt, k), cross):
            ids = np.nonzero(o)[0]
            assert np.array_equal(r[:u], ids[:u]) and (r[u:] == -1).all()
    rows0, cnt0 = SE.rows_of(cross, None, 0)
    assert rows0.shape == (n, 0) and np.array_equal(cnt0, count)
    ids = np.int32([5, n, -1, 5, n - 1, 2 ** 31 - 1])
    rows, cnt = SE.rows_of(cross, ids, 8)
    assert np.array_equal(rows[0], full[5, :8]) and np.array_equal(rows[3], rows[0]) and np.array_equal(rows[4], full[n - 1, :8])
    assert (rows[[1, 2, 5]] == -1).all() and not cnt[[1, 2, 5]].any()
    a = np.repeat(np.arange(n), 8)
    assert np.array_equal(SE.at(tri, a, full[:, :8].reshape(-1)).astype(bool), full[:, :8].reshape(-1) >= 0)   # a -1 slot: false
    assert not SE.at(tri, [3, n, 3, -1], [3, 3, n, 2]).any()


def test_order_winding_vertex_order_and_roles_do_not_matter(defects):
    rng = np.random.default_rng(11)
    tri, cross = defects["tri"], defects["cross"]
    n = cross.shape[0]
    for name, T in (("grid", tri), ("rotated", None)):
        if T is None:
            T = tri.copy()
            T[:, :9] = TT._rotated(TE.vertices(tri)).reshape(-1, 9)   # off the grid: rounded, and still pinned
            base = SE.crosses(T)
            assert base.sum() > cross.sum() // 2
        else:
            base = cross
        assert np.array_equal(base, base.T), name                     # crosses(I, J) == crosses(J, I)
        P = TE.vertices(T)
        perm = rng.permutation(n)
        assert np.array_equal(SE.crosses(P[perm])[np.ix_(np.argsort(perm), np.argsort(perm))], base), name      # ids mapped back
        for how in ("winding", "rolled", "permuted"):
            assert np.array_equal(SE.crosses(TT._shuffled(P, rng, how)), base), (name, how)


def test_triangles_that_cross_nothing():
    one = np.float32([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[1, 1, -1], [1, 1, 1], [5, 5, 0]]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert SE.crosses(one).tolist() == [[False, True], [True, False]]                    # I == J crosses nothing
        assert not SE.at(one, [0, 1], [0, 1]).any() and SE.at(one, [0, 1], [1, 0]).all()
        for bad in (np.nan, np.inf, -np.inf):
            for v in range(3):
                for c in range(3):
                    t = one.copy()
                    t[1, v, c] = bad
                    assert not SE.crosses(t).any(), (bad, v, c)
        a, b = np.float32([1, 1, 0]), np.float32([2, 2, 0])
        flat = [np.stack([a, b, b + b - a]), np.stack([a, a, b]), np.stack([b, a, b]), np.stack([a, a, a]),
                np.stack([one[0, 0], one[0, 1], one[0, 1]])]                                   # the last shares two values with one[0]
        for t in flat:
            assert not TE.live(t[None])[0]
            assert not SE.crosses(np.concatenate([one[:1], t[None], t[None]])).any()
        twin = np.stack([one[0], one[0][[2, 0, 1]], -one[0]])                                 # -0 == +0: the twin and its mirror image
        assert SE.crosses(twin)[0].tolist() == [False, True, False]


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi, query
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ezrt_self_overlap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.SELF_OVERLAP_ABI) == ["ezrt_query_self_overlap_device", "ezrt_self_overlap_at_device"]
    assert int(re.search(r"#define\s+EZRT_SELF_OVERLAP_MAX\s+(\d+)", src).group(1)) == _abi.SELF_OVERLAP_MAX == 64
    for name, params in protos.items():
        res, args = _abi.SELF_OVERLAP_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "NEAREST_ABI", "INSIDE_ABI", "BOX_OVERLAP_ABI", "TRI_OVERLAP_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other
    assert callable(query.self_overlap) and callable(query.self_overlap_at)
    assert query.SelfOverlap._fields == ("tri", "n_overlap")


def test_entry_points_are_exported():
    from ezrt_amd import _abi
    hip = _abi.load_hip()                                                      # dlopen only
    for name, (res, args) in _abi.SELF_OVERLAP_ABI.items():
        assert getattr(hip, name).argtypes == args and getattr(hip, name).restype is res


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    ids = torch.zeros(4, dtype=torch.int32)
    for k in (65, -1, 1.0, True, None, "8"):
        with pytest.raises(ValueError, match="max_k must be an int"):
            query.self_overlap(None, ids, k)
    with pytest.raises(ValueError, match="count=True"):
        query.self_overlap(None, ids, 0)
    with pytest.raises(ValueError, match="count=True"):
        query.self_overlap(None, None, 0)
    for arg in (ids, np.zeros(4, np.int32)):
        with pytest.raises(TypeError, match="GPU tensor"):
            query.self_overlap(None, arg)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.self_overlap(None, arg, max_k=0, count=True)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.self_overlap_at(None, arg, ids)
    with pytest.raises(TypeError, match="open trace.Scene"):
        query.self_overlap(None)

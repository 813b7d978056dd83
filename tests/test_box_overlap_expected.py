"""The yardstick of the box-overlap tests pinned before the device is compared with it, and the parts of the binding that need no
device (include/ezrt_box_overlap.h, ezrt_amd/query.py: box_overlap, box_overlap_at).

tests/box_overlap_expected.py restates the header's rule in numpy over boxes x all triangles.  Here it is held against a truth that
owes nothing to it: the triangle clipped by the box's six closed half-spaces in rational arithmetic (fractions.Fraction) -- a
non-empty result is an overlap -- on small-integer pairs (generic, collinear and repeated-vertex triangles, boxes of thickness zero,
pairs constructed to touch only) and on the voxel solid of tests/inside_scenes.py against every unit cell of its grid.  Then the
invariances the header promises (triangle order, winding, vertex order), the boxes and triangles that overlap nothing, the
lowest-K list, and the binding."""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_overlap_expected as BE  # noqa: E402
import inside_scenes as IS  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


# ---- the truth: Sutherland-Hodgman clipping of the triangle, as a closed polygon, by the six closed half-spaces, in Fractions.  A
# vertex on a plane is kept; an edge that crosses a plane gives its exact crossing point.  The clipped vertex list is empty exactly
# when the convex hull of the input misses the closed half-space, degenerate polygons (segments, points) included.
def clip(poly, axis, bound, keep_below):
    inside = (lambda p: p[axis] <= bound) if keep_below else (lambda p: p[axis] >= bound)
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        if inside(p):
            out.append(p)
        if inside(p) != inside(q):
            s = (bound - p[axis]) / (q[axis] - p[axis])
            out.append(tuple(a + s * (b - a) for a, b in zip(p, q)))
    return out


def clipped(lo, hi, tri):
    """the vertices of (triangle) intersected with (closed box), exact"""
    poly = [tuple(Fraction(int(x)) for x in v) for v in tri]
    for c in range(3):
        for bound, below in ((lo[c], False), (hi[c], True)):
            if poly:
                poly = clip(poly, c, Fraction(int(bound)), below)
    return poly


def truth(lo, hi, tri):
    return len(clipped(lo, hi, tri)) > 0


def touches_only(lo, hi, tri):
    """the triangle meets the closed box but not its interior: the intersection lies in one face plane (or the box has no interior)"""
    q = clipped(lo, hi, tri)
    if not q:
        return False
    return any(all(p[c] == b for p in q) for c in range(3) for b in (lo[c], hi[c]))


def _triangles(rng, n, kind):
    a = rng.integers(0, 8, (n, 3))
    if kind == "generic":
        return np.stack([a, rng.integers(0, 8, (n, 3)), rng.integers(0, 8, (n, 3))], 1)
    if kind == "collinear":                                       # three different points on one line, in any order
        step = rng.integers(-2, 3, (n, 3))
        step[(step == 0).all(1)] = (1, 0, 0)
        a = rng.integers(2, 6, (n, 3))
        m = np.where(np.abs(step).max(1) == 2, 1, rng.integers(1, 3, n))[:, None]
        T = np.stack([a - step, a, a + m * step], 1)               # every coordinate in 0 .. 7
        return np.stack([t[rng.permutation(3)] for t in T])
    if kind == "two_equal":
        b = rng.integers(0, 8, (n, 3))
        T = np.stack([a, a, b], 1)
        return np.stack([t[rng.permutation(3)] for t in T])
    assert kind == "three_equal"
    return np.stack([a, a, a], 1)


def _boxes(rng, n):
    lo = rng.integers(0, 7, (n, 3))
    return lo, lo + rng.integers(0, 3, (n, 3))                    # thickness 0 .. 2 per axis, independently


def _touching(rng):
    """pairs constructed to touch only: (lo, hi, tri) integer arrays"""
    out = []
    for _ in range(40):
        # a box corner on an interior point of an edge: the edge runs through the corner M along (1, -1, 0) (any axes), the box
        # extends from M into the positive octant, the third vertex lies on the far side
        ax = rng.permutation(3)
        M = rng.integers(2, 5, 3)
        d = np.zeros(3, int)
        d[ax[0]], d[ax[1]] = 1, -1
        third = M.copy()
        third[ax[0]] -= 2
        third[ax[1]] -= 2
        size = rng.integers(1, 3, 3)
        out.append((M, M + size, [M - 2 * d, M + d, third]))
        # a vertex on a box face, the rest of the triangle beyond it
        lo = rng.integers(1, 4, 3)
        hi = lo + 2
        c = rng.integers(0, 3)
        v = lo + 1
        v[c] = hi[c]
        w1, w2 = v + rng.integers(-1, 2, 3), v + rng.integers(-1, 2, 3)
        w1[c], w2[c] = hi[c] + rng.integers(1, 3), hi[c] + rng.integers(0, 3)
        out.append((lo, hi, [v, w1, w2]))
        # a triangle in the plane of a box face, over the face
        c = rng.integers(0, 3)
        T = np.stack([lo + rng.integers(-1, 4, 3) for _ in range(3)])
        T[:, c] = lo[c]
        T[0] = lo + 1
        T[0, c] = lo[c]                                           # one vertex inside the face's rectangle
        out.append((lo, hi, list(T)))
        # point boxes: on a vertex, on an edge's midpoint, in the face
        a = rng.integers(0, 3, 3) * 2
        b, cc = a + 2 * rng.integers(1, 3, 3), a + 2 * np.array([rng.integers(1, 3), 0, rng.integers(-1, 2)])
        out.append((a, a, [a, b, cc]))
        mid = (a + b) // 2
        out.append((mid, mid, [a, b, cc]))
        a0 = rng.integers(0, 4, 3)
        e1, e2 = np.roll([4, 0, 0], rng.integers(0, 3)), np.roll([0, 4, 0], rng.integers(0, 3))
        if not np.cross(e1, e2).any():
            e2 = np.roll(e2, 1)
        inner = a0 + (e1 + e2) // 4                               # a0 + e1 / 4 + e2 / 4: strictly inside the triangle
        out.append((inner, inner, [a0, a0 + e1, a0 + e2]))
    return out


@pytest.fixture(scope="module")
def small_pairs():
    """(lo [n, 3], hi [n, 3], V [n, 3, 3]) float32, the truth bool [n], touch-only bool [n], the restatement bool [n]"""
    rng = np.random.default_rng(2015)
    per = 1100
    V = np.concatenate([_triangles(rng, per, k) for k in ("generic", "collinear", "two_equal", "three_equal")])
    lo, hi = _boxes(rng, V.shape[0])
    made = _touching(rng)
    lo = np.concatenate([lo, np.stack([m[0] for m in made])])
    hi = np.concatenate([hi, np.stack([m[1] for m in made])])
    V = np.concatenate([V, np.stack([np.stack(m[2]) for m in made])])
    want = np.array([truth(l, h, t) for l, h, t in zip(lo, hi, V)])
    touch = np.array([w and touches_only(l, h, t) for w, l, h, t in zip(want, lo, hi, V)])
    lo, hi, V = lo.astype(np.float32), hi.astype(np.float32), V.astype(np.float32)
    return lo, hi, V, want, touch, BE.pairs(lo, hi, V), 4 * per


def test_equals_rational_clipping_on_small_integer_pairs(small_pairs):
    lo, hi, V, want, touch, got, n_random = small_pairs
    assert lo.shape[0] >= 4000 and n_random >= 4000
    wrong = got != want
    assert not wrong.any(), "%d of %d pairs differ from the clipped truth, first: box %s %s triangle %s" % (
        int(wrong.sum()), wrong.size, lo[np.argmax(wrong)], hi[np.argmax(wrong)], V[np.argmax(wrong)].tolist())
    passes_h1 = BE.h1(lo, hi, V)
    assert want.sum() >= 200 and (~want & passes_h1).sum() >= 200                  # H2 / H3 decide, not H1 alone
    assert (~want[:n_random] & passes_h1[:n_random]).sum() >= 200
    made = np.arange(lo.shape[0]) >= n_random
    assert (touch & made).sum() >= 50 and want[made].all()                         # constructed to touch, and they do
    thick = ((hi - lo) > 0).all(1)
    assert (touch & thick).sum() >= 50                                             # ... a box with an interior that is not entered
    kinds = np.arange(n_random) // (n_random // 4)
    for k in range(4):                                                             # every kind of triangle has both answers
        assert want[:n_random][kinds == k].any() and not want[:n_random][kinds == k].all(), k
    assert ((hi - lo) == 0).any(1).sum() >= 1000 and ((hi - lo) == 0).all(1).sum() >= 30


@pytest.fixture(scope="module")
def solid():
    v = IS.voxel_solid()
    G = IS.G
    cells = np.stack(np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij"), -1).reshape(-1, 3)
    lo, hi = cells.astype(np.float32), (cells + 1).astype(np.float32)
    return dict(tri=v["tri"], occ=v["occ"], cells=cells, lo=lo, hi=hi, over=BE.overlaps(lo, hi, v["tri"]))   # computed once


def test_voxel_solid_every_unit_cell(solid):
    tri, cells, lo, hi, over = solid["tri"], solid["cells"], solid["lo"], solid["hi"], solid["over"]
    V = BE.vertices(tri)
    assert over.shape == (IS.G ** 3, V.shape[0])
    # the truth for all cells x triangles: pairs whose closed integer bounding boxes are disjoint have an empty intersection (no
    # arithmetic: integer comparisons), the others are clipped
    tlo, thi = V.min(1), V.max(1)
    near = ((tlo[None] <= hi[:, None]) & (thi[None] >= lo[:, None])).all(-1)
    assert not over[~near].any()
    i, k = np.nonzero(near)
    want = np.array([truth(lo[a], hi[a], V[b]) for a, b in zip(i, k)])
    assert np.array_equal(over[i, k], want) and want.any() and not want.all()
    # a cell whose 3 x 3 x 3 neighbourhood is all solid or all empty is not adjacent to the surface: nothing overlaps it
    occ = solid["occ"]
    pad = np.zeros(tuple(n + 2 for n in occ.shape), bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    away = np.array([len({bool(x) for x in pad[a:a + 3, b:b + 3, c:c + 3].reshape(-1)}) == 1 for a, b, c in cells])
    assert away.sum() >= 8 and not over[away].any()                                # (the grid's corners at least)
    # ... and a cell with a boundary face has that face's two triangles at least
    assert (over.sum(1)[~away] >= 2).all() and over.sum(1).max() > 8


def _rows(over):
    return [np.nonzero(r)[0] for r in over]


def test_order_winding_and_vertex_order_do_not_matter(solid):
    lo, hi, over = solid["lo"], solid["hi"], solid["over"]
    P = BE.vertices(solid["tri"])
    rng = np.random.default_rng(7)
    perm = rng.permutation(P.shape[0])
    got = BE.overlaps(lo, hi, P[perm])
    assert np.array_equal(got[:, np.argsort(perm)], over)                          # ids mapped back
    assert np.array_equal(BE.overlaps(lo, hi, P[:, ::-1]), over)                   # winding
    rolled = np.stack([np.roll(t, int(r), axis=0) for t, r in zip(P, rng.integers(0, 3, P.shape[0]))])
    assert np.array_equal(BE.overlaps(lo, hi, rolled), over)                       # vertex rotation
    # ... and on a rotated, off-grid copy, where every product rounds; boxes around its vertices and across it
    ang = 0.37
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.6), -np.sin(0.6)], [0, np.sin(0.6), np.cos(0.6)]])
    Q = (P.astype(np.float64) @ R.T).astype(np.float32)
    c = Q.reshape(-1, 3)[rng.integers(0, Q.shape[0] * 3, 300)]
    half = rng.uniform(0.0, 0.8, (300, 3)).astype(np.float32) * (rng.random((300, 3)) > 0.2)
    qlo, qhi = c - half, c + half
    base = BE.overlaps(qlo, qhi, Q)
    assert base.any(1).all() and base.sum(1).max() > 8 and not base.all()          # (a box around a vertex holds it)
    perm = rng.permutation(Q.shape[0])
    assert np.array_equal(BE.overlaps(qlo, qhi, Q[perm])[:, np.argsort(perm)], base)
    assert np.array_equal(BE.overlaps(qlo, qhi, Q[:, ::-1]), base)
    assert np.array_equal(BE.overlaps(qlo, qhi, np.stack([t[rng.permutation(3)] for t in Q])), base)
    assert np.array_equal(BE.overlaps(qlo, qhi, np.stack([np.roll(t, 1, axis=0) for t in Q])), base)


def test_boxes_and_triangles_that_overlap_nothing():
    one = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[5, 5, 5], [6, 5, 5], [5, 6, 7]]])
    lo, hi = np.float32([-1, -1, -1]), np.float32([8, 8, 8])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                             # no warning from numpy anywhere below
        assert BE.overlaps(lo[None], hi[None], one).tolist() == [[True, True]]
        for c in range(3):
            l, h = lo.copy(), hi.copy()
            l[c], h[c] = 8, -1                                                     # lo > hi on one axis
            assert not BE.overlaps(l[None], h[None], one).any()
            for bad in (np.nan, np.inf, -np.inf):
                for which in (0, 1):
                    l, h = lo.copy(), hi.copy()
                    (l, h)[which][c] = bad
                    assert not BE.overlaps(l[None], h[None], one).any(), (c, bad, which)
        assert BE.live(np.float32([[1, 2, 3]]), np.float32([[1, 2, 3]]))[0]        # a point box is live
        assert BE.overlaps(np.float32([[1, 0, 0]]), np.float32([[1, 0, 0]]), one).tolist() == [[True, False]]
        huge_lo, huge_hi = np.float32([[-FLT_MAX] * 3]), np.float32([[FLT_MAX] * 3])
        for bad in (np.nan, np.inf, -np.inf):
            for v in range(3):
                for c in range(3):
                    t = one.copy()
                    t[0, v, c] = bad
                    assert BE.overlaps(huge_lo, huge_hi, t).tolist() == [[False, True]], (bad, v, c)
                    assert BE.overlaps(lo[None], hi[None], t).tolist() == [[False, True]]
        # a +-FLT_MAX box overlaps every finite triangle, the largest ones included
        big = np.float32([[[FLT_MAX, -FLT_MAX, 0], [-FLT_MAX, FLT_MAX, FLT_MAX], [FLT_MAX, FLT_MAX, -FLT_MAX]],
                          [[FLT_MAX, FLT_MAX, FLT_MAX]] * 3, [[1e-45, 0, 0], [0, 1e-45, 0], [0, 0, -1e-45]]])
        assert BE.overlaps(huge_lo, huge_hi, np.concatenate([one, big])).all()
        assert BE.overlaps(huge_lo, huge_hi, IS.voxel_solid()["tri"]).all()
        # ... and a huge triangle against a small box far from its plane does not
        assert BE.overlaps(np.float32([[1, 1, 1]]), np.float32([[2, 2, 2]]), big).tolist() == [[False, False, False]]


def test_lowest_k_list(solid):
    lo, hi, tri, over = solid["lo"], solid["hi"], solid["tri"], solid["over"]
    whole_lo, whole_hi = np.float32([[0, 0, 0]]), np.float32([[IS.G] * 3])
    L = np.concatenate([lo, whole_lo, np.float32([[np.nan, 0, 0]])])
    H = np.concatenate([hi, whole_hi, np.float32([[1, 1, 1]])])
    full, count = BE.query(L, H, tri, 64)
    m = BE.vertices(tri).shape[0]
    assert count[-2] == m > 64 and count[-1] == 0 and (full[-1] == -1).all()       # the whole scene; a box that is not live
    assert np.array_equal(count[:-2], over.sum(1)) and (count == 0).any() and ((count > 0) & (count < 8)).any() and (count > 8).any()
    for k in (1, 3, 8, 64):
        rows, cnt = BE.query(L, H, tri, k)
        assert rows.shape == (L.shape[0], k) and rows.dtype == np.int32 and np.array_equal(cnt, count)      # n_overlap independent of K
        assert np.array_equal(rows, full[:, :k])                                   # a K-row is a prefix of every longer one
        used = np.minimum(cnt, k)
        for r, u, o in zip(rows[:-2], used[:-2], _rows(over)):
            assert np.array_equal(r[:u], o[:u]) and (r[u:] == -1).all()            # the lowest ids, ascending, then -1
    assert np.array_equal(full[-2], np.arange(64))
    rows0, cnt0 = BE.query(L, H, tri, 0)
    assert rows0.shape == (L.shape[0], 0) and np.array_equal(cnt0, count)
    # the _at form: the pairs of the rows are overlaps, ids outside the scene are not
    ids = np.concatenate([full[:, 0], [m, -1, 2 ** 31 - 1]]).astype(np.int64)
    bl = np.concatenate([L, np.repeat(whole_lo, 3, 0)])
    bh = np.concatenate([H, np.repeat(whole_hi, 3, 0)])
    got = BE.at(bl, bh, tri, ids)
    assert np.array_equal(got[:-3].astype(bool), full[:, 0] >= 0) and not got[-3:].any()


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi, query
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ezrt_box_overlap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.BOX_OVERLAP_ABI) == ["ezrt_box_overlap_at_device", "ezrt_query_box_overlap_device"]
    assert int(re.search(r"#define\s+EZRT_BOX_OVERLAP_MAX\s+(\d+)", src).group(1)) == _abi.BOX_OVERLAP_MAX == 64
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.BOX_OVERLAP_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "NEAREST_ABI", "INSIDE_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other
    assert callable(query.box_overlap) and callable(query.box_overlap_at)
    assert query.BoxOverlap._fields == ("tri", "n_overlap")


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    lo, hi = torch.zeros((4, 3), dtype=torch.float32), torch.ones((4, 3), dtype=torch.float32)
    for k in (65, -1, 1.0, True, None, "8"):
        with pytest.raises(ValueError, match="max_k must be an int"):
            query.box_overlap(None, lo, hi, k)
    with pytest.raises(ValueError, match="count=True"):
        query.box_overlap(None, lo, hi, 0)
    for args in ((lo, hi), (np.zeros((4, 3), np.float32), hi), (lo, np.ones((4, 3), np.float32))):
        with pytest.raises(TypeError, match="GPU tensor"):
            query.box_overlap(None, *args)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.box_overlap(None, *args, max_k=0, count=True)
        with pytest.raises(TypeError, match="GPU tensor"):
            query.box_overlap_at(None, *args, torch.zeros(4, dtype=torch.int32))

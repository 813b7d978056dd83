"""The definition of include/ezrt_self_overlap.h restated in numpy (a helper, no test): the number of vertices two triangles of the
scene share by value, and per case the rule of the header -- T2 of the triangle rule (s = 0), the two segment tests of 16
directions each (s = 1), the fold test (s = 2), true (s = 3) -- over triangles x ALL triangles, and the lowest-K list and the count.

Written from the header's comment, not from the kernel.  The sorts, the equalities of vertices and the order of the two triangles
are float32 comparisons; everything else is float64 on the float32 values converted exactly, one numpy operation (one rounding)
per written operation, the sums left to right and the zero component of a direction g x axis_j multiplied and added like the
others.  Liveness, the sorting, T1 and T2 are those of tests/tri_overlap_expected.py, imported, not restated."""
import numpy as np

import tri_overlap_expected as TE

F = np.float32
D = np.float64
PAIRS = TE.PAIRS
REST = np.array([[1, 2], [0, 2], [0, 1]])       # the two other vertices of a sorted triangle, still in the order of their values


def shared(IS, JS):
    """(s int [p], eq bool [p, 3, 3]): eq[p, i, j] is vertex i of IS[p] == vertex j of JS[p] on all three coordinates, s the number
    of vertices of I that equal a vertex of J -- IS, JS sorted float32 [p, 3, 3] of live triangles"""
    eq = (IS[:, :, None, :] == JS[:, None, :, :]).all(-1)
    return eq.any(2).sum(1), eq


def _first(IS, JS):
    """bool [p]: J comes first in the order of the values, (A, B) = (J, I) -- the choice of T2"""
    return TE._less(JS[:, 0], IS[:, 0]) | (TE._same(JS[:, 0], IS[:, 0]) & (
        TE._less(JS[:, 1], IS[:, 1]) | (TE._same(JS[:, 1], IS[:, 1]) & TE._less(JS[:, 2], IS[:, 2]))))


def _p(x, d):
    return (x[:, 0] * d[:, 0] + x[:, 1] * d[:, 1]) + x[:, 2] * d[:, 2]


def seg_meets(a, b, T):
    """bool [p]: the closed segment a b (float32 [p, 3], a before b in the order of the values) against the closed live sorted
    triangle T [p, 3, 3]: none of the 16 directions separates"""
    with np.errstate(all="raise"):
        t0 = T[:, 0]
        Ds = [TE._d3(T[:, 1], t0), TE._d3(T[:, 2], t0), TE._d3(a, t0), TE._d3(b, t0)]
        zero = np.zeros(T.shape[0], D)
        ok = np.ones(T.shape[0], bool)

        def direction(x):
            nonlocal ok
            p = [_p(x, d) for d in Ds]
            tmax, tmin = np.maximum(np.maximum(zero, p[0]), p[1]), np.minimum(np.minimum(zero, p[0]), p[1])
            smax, smin = np.maximum(p[2], p[3]), np.minimum(p[2], p[3])
            ok &= ~((tmax < smin) | (smax < tmin))

        d = TE._d3(b, a)
        f = TE._edges(T)
        direction(TE.normal(T))
        for j in range(3):
            direction(TE._cross(d, f[j]))
        for g in [d] + f:
            for j in range(3):
                u, w = (j + 1) % 3, (j + 2) % 3
                x = np.zeros((T.shape[0], 3), D)
                x[:, u], x[:, w] = -g[:, w], g[:, u]
                direction(x)
    return ok


def _take(S, idx):
    return S[np.arange(S.shape[0]), idx]


def one_shared(IS, JS, eq):
    """bool [p]: s = 1 -- seg_meets(a, b; J) || seg_meets(c, d; I)"""
    iv, jv = eq.any(2).argmax(1), eq.any(1).argmax(1)
    a, b = _take(IS, REST[iv, 0]), _take(IS, REST[iv, 1])
    c, d = _take(JS, REST[jv, 0]), _take(JS, REST[jv, 1])
    return seg_meets(a, b, JS) | seg_meets(c, d, IS)


def two_shared(IS, JS, eq):
    """bool [p]: s = 2 -- coplanar && same_side, with the triangle that comes first by value in the role of I"""
    first = _first(IS, JS)[:, None, None]
    A, B = np.where(first, JS, IS), np.where(first, IS, JS)
    eqA = np.where(first, eq.transpose(0, 2, 1), eq)                  # [p, vertex of A, vertex of B]
    ia, ib = eqA.any(2).argmin(1), eqA.any(1).argmin(1)             # the apexes: the one vertex that is not shared
    u, v = _take(A, REST[ia, 0]), _take(A, REST[ia, 1])
    a, b = _take(A, ia), _take(B, ib)
    with np.errstate(all="raise"):
        e = TE._d3(v, u)
        da, db = TE._d3(a, u), TE._d3(b, u)
        Xa, Xb = TE._cross(e, da), TE._cross(e, db)
        coplanar = _p(Xa, db) == 0
        same_side = (((Xa > 0) & (Xb > 0)) | ((Xa < 0) & (Xb < 0))).any(1)
    return coplanar & same_side


def crosses_sorted(IS, JS):
    """bool [p]: crosses for live sorted triangles of different ids whose bounding boxes meet (T1 holds)"""
    s, eq = shared(IS, JS)
    out = np.zeros(IS.shape[0], bool)
    i = np.nonzero(s == 0)[0]
    out[i] = TE.t2(IS[i], JS[i])
    i = np.nonzero(s == 1)[0]
    out[i] = one_shared(IS[i], JS[i], eq[i])
    i = np.nonzero(s == 2)[0]
    out[i] = two_shared(IS[i], JS[i], eq[i])
    out[s == 3] = True
    return out


def pairs(I, J):
    """bool [p]: crosses(I[p], J[p]) for triangles float32 [p, 3, 3] taken to have different ids"""
    (il, IS), (jl, JS) = TE.prepare(I), TE.prepare(J)
    out = il & jl
    i = np.nonzero(out)[0]
    out[i] = TE.t1(IS[i], JS[i])
    i = np.nonzero(out)[0]
    out[i] = crosses_sorted(IS[i], JS[i])
    return out


def shared_count(I, J):
    """int [p]: s of live triangles I, J float32 [p, 3, 3]"""
    return shared(TE.prepare(I)[1], TE.prepare(J)[1])[0]


def crosses(tri):
    """bool [m, m]: every triangle of `tri` against every other"""
    live, S = TE.prepare(TE.vertices(tri))
    m = S.shape[0]
    out = np.zeros((m, m), bool)
    bc = max(1, PAIRS // max(1, m))
    for i0 in range(0, m, bc):
        s = slice(i0, min(m, i0 + bc))
        out[s] = live[s, None] & live[None, :] & TE.t1(S[s, None], S[None])
    out[np.arange(m), np.arange(m)] = False
    i, k = np.nonzero(out)
    for p0 in range(0, i.size, PAIRS):
        s = slice(p0, p0 + PAIRS)
        out[i[s], k[s]] = crosses_sorted(S[i[s]], S[k[s]])
    return out


def at(tri, a, b):
    """uint8 [n]: crosses(a[i], b[i]); an id outside the scene and equal ids give 0"""
    V = TE.vertices(tri)
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    m = V.shape[0]
    ok = (a >= 0) & (a < m) & (b >= 0) & (b < m) & (a != b)
    out = np.zeros(a.shape[0], np.uint8)
    out[ok] = pairs(V[a[ok]], V[b[ok]])
    return out


def rows_of(cross, ids, k):
    """(tri int32 [n, k], n_overlap int32 [n]) of the matrix `cross` for the queries `ids` (None: every triangle); an id outside
    the scene has an empty row"""
    m = cross.shape[0]
    ids = np.arange(m) if ids is None else np.asarray(ids).reshape(-1).astype(np.int64)
    ok = (ids >= 0) & (ids < m)
    over = np.zeros((ids.shape[0], m), bool)
    over[ok] = cross[ids[ok]]
    return TE.lowest(over, k)


def query(tri, ids, k):
    """what ezrt_query_self_overlap_device writes"""
    return rows_of(crosses(tri), ids, k)

"""The definition of include/ezrt_tri_distance.h restated in numpy float32 (a helper, no test): the 15 sub-candidates of a pair in the
header's order, the first smallest finite d2, the crossing step, and the answer over query triangles x ALL triangles -- there is no
tree here.

Written from the header's comment, not from the kernel: every operation is one numpy float32 operation (one rounding each, numpy does
not contract), dot is x*x' + y*y' + z*z' left to right, the cases are selected with np.where.  The vertex sub-candidates are
closest_point_expected.per_triangle as it stands (the header: "closest_point_triangle as it stands"), liveness and the crossing step
are tri_overlap_expected's.  Both triangles' vertices are taken in the order given.  Chunked over queries x triangles."""
import numpy as np

import closest_point_expected as E
import tri_overlap_expected as TE

F = np.float32
PAIRS = 1 << 17            # query-triangle pairs evaluated at a time
N_SUB = 15

_dot, _min, _max = E._dot, E._min, E._max


def _clamp01(v):           # min(max(v, 0), 1) with ez_max, ez_min: a NaN stays a NaN
    return _min(_max(v, F(0)), F(1))


def _into_box(r, P, Q):
    lo, hi = _min(P, Q), _max(P, Q)
    return np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(F)


def seg_seg(P1, Q1, P2, Q2):
    """(x, y, d2) of the closed segments [P1, Q1] and [P2, Q2], float32 [..., 3] that broadcast against each other"""
    with np.errstate(all="ignore"):
        d1, d2, r = Q1 - P1, Q2 - P2, P1 - P2
        a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
        den = a * e - b * b
        s = np.where(den > 0, _clamp01((b * f - c * e) / den), F(0)).astype(F)
        t = ((b * s + f) / e).astype(F)
        below, above = t < 0, t > 1
        s = np.where(below, _clamp01(-c / a), np.where(above, _clamp01((b - c) / a), s)).astype(F)
        t = np.where(below, F(0), np.where(above, F(1), t)).astype(F)
        x = _into_box(P1 + d1 * s[..., None], P1, Q1)
        y = _into_box(P2 + d2 * t[..., None], P2, Q2)
        g = x - y
        return x, y, _dot(g, g)


def sub_candidates(Q, V):
    """yields (x, y, d2) of the 15 sub-candidates in the header's order; Q, V float32 [..., 3, 3] that broadcast against each other"""
    q = [Q[..., i, :] for i in range(3)]
    v = [V[..., i, :] for i in range(3)]
    shape = np.broadcast_shapes(Q.shape, V.shape)[:-2]
    for i in range(3):                                                 # a vertex of Q against the scene triangle
        y, _, _, d2 = E.per_triangle(q[i], v[0], v[1], v[2])
        yield np.broadcast_to(q[i], shape + (3,)), y, d2
    for j in range(3):                                                 # a vertex of the scene triangle against Q
        x, _, _, d2 = E.per_triangle(v[j], q[0], q[1], q[2])
        yield x, np.broadcast_to(v[j], shape + (3,)), d2
    for i in range(3):
        for j in range(3):
            yield seg_seg(q[i], q[(i + 1) % 3], v[j], v[(j + 1) % 3])


def all_d2(Q, V):
    """float32 [15, ...]: the d2 of every sub-candidate"""
    return np.stack([np.broadcast_to(d2, np.broadcast_shapes(Q.shape, V.shape)[:-2]) for _, _, d2 in sub_candidates(Q, V)])


def pair_min(Q, V, points=True):
    """(found bool, best float32, x, y): the first smallest finite d2 of the 15 and its points (zeros where nothing is finite, or
    None without `points`)"""
    shape = np.broadcast_shapes(Q.shape, V.shape)[:-2]
    found = np.zeros(shape, bool)
    best = np.full(shape, np.inf, F)
    bx = np.zeros(shape + (3,), F) if points else None
    by = np.zeros(shape + (3,), F) if points else None
    for x, y, d2 in sub_candidates(Q, V):
        with np.errstate(all="ignore"):
            take = np.isfinite(d2) & (~found | (d2 < best))
        best = np.where(take, d2, best).astype(F)
        found |= take
        if points:
            bx, by = np.where(take[..., None], x, bx).astype(F), np.where(take[..., None], y, by).astype(F)
    return found, best, bx, by


def pairs(Q, V):
    """(candidate bool [p], dist2 [p], x [p, 3], y [p, 3], crosses uint8 [p]) of query triangle i against triangle i -- Q, V float32
    [p, 3, 3]; where the pair is no candidate: (False, +inf, zeros, zeros, 0)"""
    Q, V = np.ascontiguousarray(Q, F).reshape(-1, 3, 3), np.ascontiguousarray(V, F).reshape(-1, 3, 3)
    found, best, x, y = pair_min(Q, V)
    cand = TE.live(Q) & TE.live(V) & found
    cross = TE.pairs(Q, V) & cand
    d2 = np.where(cross, F(0), np.where(cand, best, F(np.inf))).astype(F)
    return cand, d2, np.where(cand[:, None], x, F(0)).astype(F), np.where(cand[:, None], y, F(0)).astype(F), cross.astype(np.uint8)


# With `prune` the pairs that cannot hold a winner or a tie are left out BEFORE the restatement is evaluated, by an argument that is
# not the kernel's: in float64, the gap between the two bounding boxes is a lower bound of the true distance of the pair, U = the
# restated dist2 of the query against the SEEDS triangles with the smallest gaps is an upper bound of the winner's, and a pair is
# kept when gap <= sqrt(U) * (1 + 1e-3) + 1e-4 * (largest |coordinate| of the two) -- a thousand times what fp32 rounding can move a
# distance (about 1e-6 relative to the coordinates).  A pair left out is reported as no candidate; the winner, its ties and every
# output of query() are those of the full evaluation (tests/test_tri_distance_expected.py holds the two against each other).
SEEDS = 8
SLACK_REL, SLACK_ABS = 1e-3, 1e-4


def _kept(Q, V, live):
    """bool [n, m]: the pairs the pruned evaluation keeps"""
    n, m = Q.shape[0], V.shape[0]
    Qd, Vd = Q.astype(np.float64), V.astype(np.float64)
    with np.errstate(all="ignore"):
        qlo, qhi, lo, hi = Qd.min(1)[:, None], Qd.max(1)[:, None], Vd.min(1)[None], Vd.max(1)[None]
        gap = np.sqrt((np.maximum(np.maximum(lo - qhi, qlo - hi), 0.0) ** 2).sum(-1))
    gap = np.where(live, gap, np.inf)
    k = min(SEEDS, m)
    seeds = np.argpartition(gap, k - 1, axis=1)[:, :k]
    cand, d2, _, _, _ = pairs(np.repeat(Q, k, 0), V[seeds.reshape(-1)])
    U = np.where(cand, d2, F(np.inf)).reshape(n, k).min(1).astype(np.float64)
    scale = np.maximum(np.abs(Qd).max((1, 2))[:, None], np.abs(Vd).max((1, 2))[None])
    with np.errstate(all="ignore"):
        return live & ~(gap > np.sqrt(U)[:, None] * (1 + SLACK_REL) + SLACK_ABS * scale)      # (a NaN or infinite bound keeps the pair)


def dist2_all(tris, tri, cross=None, prune=False):
    """(candidate bool [n, m], dist2 float32 [n, m], crosses bool [n, m]) over query triangles x ALL triangles"""
    Q = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    V = TE.vertices(tri)
    n, m = Q.shape[0], V.shape[0]
    live = TE.live(Q)[:, None] & TE.live(V)[None, :]
    cross = TE.overlaps(Q.reshape(-1, 9), V) if cross is None else cross
    cand = np.zeros((n, m), bool)
    d2 = np.full((n, m), np.inf, F)
    if prune:
        i, k = np.nonzero(_kept(Q, V, live))
        for p0 in range(0, i.size, PAIRS):
            s = slice(p0, p0 + PAIRS)
            found, best, _, _ = pair_min(Q[i[s]], V[k[s]], points=False)
            cand[i[s], k[s]] = found
            d2[i[s], k[s]] = best
    else:
        bc = max(1, PAIRS // max(1, m))
        for i0 in range(0, n, bc):
            s = slice(i0, min(n, i0 + bc))
            found, best, _, _ = pair_min(Q[s, None], V[None], points=False)
            cand[s] = found & live[s]
            d2[s] = best
    cross = cross & cand
    return cand, np.where(cross, F(0), np.where(cand, d2, F(np.inf))).astype(F), cross


def bound(d_max, n):
    """(B float32 [n], allowed bool [n])"""
    if d_max is None:
        return np.full(n, np.inf, F), np.ones(n, bool)
    d_max = np.ascontiguousarray(d_max, F).reshape(n)
    with np.errstate(all="ignore"):
        return (d_max * d_max).astype(F), d_max >= 0                   # (false for a NaN)


def query(tris, tri, d_max=None, table=None, prune=False):
    """(tri_id int32 [n], dist [n], point_query [n, 3], point_scene [n, 3], crosses uint8 [n]): what ezrt_query_tri_distance_device
    writes; `table` = dist2_all(tris, tri), when the caller holds it"""
    Q = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    V = TE.vertices(tri)
    n = Q.shape[0]
    cand, d2, cross = dist2_all(Q, tri, prune=prune) if table is None else table
    B, allowed = bound(d_max, n)
    with np.errstate(all="ignore"):
        ok = cand & allowed[:, None] & (d2 <= B[:, None])
    key = np.where(ok, d2, F(np.inf))
    tie = ok & (key == key.min(1, keepdims=True))                      # the pairs at the smallest dist2 ...
    first = tie & cross                                                # ... of which one that crosses comes before one that does not
    win = np.argmax(np.where(first.any(1, keepdims=True), first, tie), axis=1)   # ... and then the lowest k (the FIRST True)
    r = np.arange(n)
    has = ok[r, win] if V.shape[0] else np.zeros(n, bool)
    tri_id = np.where(has, win, -1).astype(np.int32)
    _, _, x, y, _ = pairs(Q, V[np.where(has, win, 0)])
    with np.errstate(all="ignore"):
        dist = np.where(has, np.sqrt(np.where(has, key[r, win], F(0))), F(np.inf)).astype(F)
    return (tri_id, dist, np.where(has[:, None], x, F(0)).astype(F), np.where(has[:, None], y, F(0)).astype(F),
            (has & cross[r, win]).astype(np.uint8))


def at(tris, tri, ids):
    """(dist [n], point_query [n, 3], point_scene [n, 3], crosses uint8 [n]): what ezrt_tri_distance_at_device writes for query
    triangle i against triangle ids[i]"""
    Q = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    V = TE.vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    inside = (ids >= 0) & (ids < V.shape[0])
    cand, d2, x, y, cross = pairs(Q, V[np.where(inside, ids, 0)])
    cand &= inside
    with np.errstate(all="ignore"):
        dist = np.where(cand, np.sqrt(np.where(cand, d2, F(0))), F(np.inf)).astype(F)
    return dist, np.where(cand[:, None], x, F(0)).astype(F), np.where(cand[:, None], y, F(0)).astype(F), (cross & cand).astype(np.uint8)


def box_lb(qlo, qhi, lo, hi):
    """float32: tri_distance_box -- g = max(lo - qhi, 0, qlo - hi) per axis, lb = dot(g, g), in the kernel's order of operations"""
    with np.errstate(all="ignore"):
        g = np.fmax(np.fmax(lo - qhi, F(0)), qlo - hi).astype(F)
        return _dot(g, g).astype(F)

"""The definition of include/ezrt_sphere_cast.h restated in numpy float32 (a helper, no test): liveness, the touching step on
closest_point_expected as it stands, the gate, the seven sub-candidates of a pair in the header's order, the first smallest finite t
clamped up to tnear, and the answer over queries x ALL triangles -- there is no tree here.  It also says which sub-candidate won.

Written from the header's comment, not from the kernel: every operation is one numpy float32 operation (one rounding each, numpy does
not contract), dot is x*x' + y*y' + z*z' left to right, the cases are selected with np.where.  The gate is part of the rule, so the
seven sub-candidates are evaluated for the pairs that pass it alone; a pair that fails it is no candidate by definition."""
import numpy as np

import closest_point_expected as E

F = np.float32
PAIRS = 1 << 18            # pairs evaluated at a time
INF = F(np.inf)

_dot, _min, _max = E._dot, E._min, E._max


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def vertices(tri):
    return np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)


def split(rays, radius):
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    return rays[:, :3], rays[:, 3:], np.ascontiguousarray(radius, F).reshape(-1)


def inverse(d):
    with np.errstate(all="ignore"):
        return (F(1) / d).astype(F)


def live(rays, radius):
    """bool [n]: step 1 for the query"""
    o, d, r = split(rays, radius)
    with np.errstate(all="ignore"):
        dd = _dot(d, d)
        inv = inverse(d)
        return (np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(r) & (r >= 0) & np.isfinite(dd) & (dd > 0) &
                ((d == 0) | np.isfinite(inv)).all(1))


def tri_live(V):
    return np.isfinite(V).all((-1, -2))


def slab(o, d, r, lo, hi):
    """(passes bool, tnear float32) of the ray against the box [lo, hi] inflated by r; o, d, lo, hi [..., 3] and r [...] broadcast"""
    with np.errstate(all="ignore"):
        inv = inverse(d)
        L, H = lo - r[..., None], hi + r[..., None]
        x, y = (L - o) * inv, (H - o) * inv
        flat = d == 0
        near, far = np.where(d < 0, y, x), np.where(d < 0, x, y)
        ok = ~(flat & ((o < L) | (o > H))).any(-1)
        tn = np.zeros(ok.shape, F)
        tf = np.full(ok.shape, INF, F)
        for k in range(3):
            tn = np.where(~flat[..., k] & (tn < near[..., k]), near[..., k], tn)        # max(tn, near): a NaN bounds nothing
            tf = np.where(~flat[..., k] & (far[..., k] < tf), far[..., k], tf)          # min(tf, far)
        return ok & (tn <= tf), tn.astype(F)


def box_bound(o, d, r, lo, hi):
    """float32: sphere_cast_box -- tnear where the gate passes, else +inf"""
    ok, tn = slab(o, d, r, lo, hi)
    return np.where(ok, tn, INF).astype(F)


def _root(B, C, disc):
    with np.errstate(all="ignore"):
        t = C / (np.sqrt(disc) - B)
        return np.where(C <= 0, F(0), np.where((B < 0) & (disc >= 0), t, F(np.nan))).astype(F)


def _into(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(F)


def sub_candidates(o, d, r, V):
    """yields (valid, tt, x) of the seven sub-candidates in the header's order; o, d [p, 3], r [p], V [p, 3, 3]"""
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all="ignore"):
        rr = r * r
        dd = _dot(d, d)
        lo, hi = _min(_min(a, b), c), _max(_max(a, b), c)
        ab, ac, m = b - a, c - a, o - a
        n0 = _cross(ab, ac)
        h0 = _dot(n0, m)
        flip = h0 < 0
        n = np.where(flip[:, None], -n0, n0)
        h = np.where(flip, -h0, h0)
        nd = _dot(n, d)
        ln = np.sqrt(_dot(n, n))
        g = h - r * ln
        tt = np.where(g <= 0, F(0), g / (-nd)).astype(F)
        x = (o + d * tt[:, None]) - n * (r / ln)[:, None]
        e0, e1, e2 = _dot(_cross(ab, x - a), n0), _dot(_cross(c - b, x - b), n0), _dot(_cross(a - c, x - c), n0)
        yield (nd < 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0), tt, _into(x, lo, hi)
        for u, v in ((a, b), (b, c), (c, a)):
            e, m = v - u, o - u
            ee = _dot(e, e)
            sd, sm = _dot(e, d) / ee, _dot(e, m) / ee
            dp, mp = d - e * sd[:, None], m - e * sm[:, None]
            k = _cross(mp, dp)
            tt = _root(_dot(mp, dp), _dot(mp, mp) - rr, _dot(dp, dp) * rr - _dot(k, k))
            s = sm + sd * tt
            yield (s >= 0) & (s <= 1), tt, _into(u + e * s[:, None], _min(u, v), _max(u, v))
        for p in (a, b, c):
            m = o - p
            k = _cross(m, d)
            tt = _root(_dot(m, d), _dot(m, m) - rr, dd * rr - _dot(k, k))
            yield np.ones(tt.shape, bool), tt, p


def pairs(o, d, r, V):
    """(candidate bool [p], t float32 [p] (+inf), sub int8 [p] (-1), point [p, 3] (zeros), gate bool [p], tnear [p]) of the swept rule
    for LIVE queries o, d, r against triangles V [p, 3, 3], pair by pair"""
    p = o.shape[0]
    ok = tri_live(V)
    Vz = np.where(ok[:, None, None], V, F(0))
    gate, tnear = slab(o, d, r, Vz.min(1), Vz.max(1))
    gate &= ok
    best = np.full(p, INF, F)
    sub = np.full(p, -1, np.int8)
    point = np.zeros((p, 3), F)
    for j, (valid, tt, x) in enumerate(sub_candidates(o, d, r, Vz)):
        with np.errstate(all="ignore"):
            take = valid & (tt < best)                                  # false for a NaN or infinite tt; the first wins on equality
        best = np.where(take, tt, best).astype(F)
        sub = np.where(take, np.int8(j), sub)
        point = np.where(take[:, None], x, point).astype(F)
    t = np.where(best < tnear, tnear, best).astype(F)
    cand = gate & (best < INF) & (t < INF)
    return (cand, np.where(cand, t, INF).astype(F), np.where(cand, sub, np.int8(-1)), np.where(cand[:, None], point, F(0)).astype(F), gate,
            tnear)


def swept_all(rays, radius, tri, points=False):
    """(candidate bool [n, m], t float32 [n, m], sub int8 [n, m], gate bool [n, m], tnear float32 [n, m]) of step 3 over queries x ALL
    triangles; a query that is not live has no candidates.  With `points`, a sixth entry: the pairs' contact points float32 [n, m, 3]
    (zeros where the pair is no candidate)."""
    o, d, r = split(rays, radius)
    V = vertices(tri)
    n, m = o.shape[0], V.shape[0]
    alive = live(rays, radius)
    ok = tri_live(V)
    Vz = np.where(ok[:, None, None], V, F(0))
    lo, hi = Vz.min(1), Vz.max(1)
    gate = np.zeros((n, m), bool)
    tnear = np.zeros((n, m), F)
    bc = max(1, PAIRS // max(1, m))
    for i0 in range(0, n, bc):
        s = slice(i0, min(n, i0 + bc))
        g, tn = slab(o[s, None], d[s, None], r[s, None], lo[None], hi[None])
        gate[s] = g & ok[None] & alive[s, None]
        tnear[s] = tn
    cand = np.zeros((n, m), bool)
    t = np.full((n, m), INF, F)
    sub = np.full((n, m), -1, np.int8)
    x = np.zeros((n, m, 3), F) if points else None
    i, k = np.nonzero(gate)
    for p0 in range(0, i.size, PAIRS):
        s = slice(p0, p0 + PAIRS)
        c, tt, sb, px, _, _ = pairs(o[i[s]], d[i[s]], r[i[s]], V[k[s]])
        cand[i[s], k[s]], t[i[s], k[s]], sub[i[s], k[s]] = c, tt, sb
        if points:
            x[i[s], k[s]] = px
    return (cand, t, sub, gate, tnear, x) if points else (cand, t, sub, gate, tnear)


def touch(rays, radius, tri, prune=False):
    """(tri_id int32 [n] (-1), point [n, 3]): step 2 -- closest_point for o with d_max = r, for the live queries.  With `prune` the
    queries that cannot touch are left out before closest_point_expected is asked, by an argument that is not the kernel's: in
    float64, a query whose o is farther than r * (1 + 1e-3) + 1e-4 * (largest |coordinate| of the two) from every triangle's
    bounding box -- a thousand times what fp32 rounding can move a distance -- has no triangle with dist2 <= r * r
    (tests/test_sphere_cast_expected.py holds the two against each other)."""
    o, d, r = split(rays, radius)
    alive = live(rays, radius)
    ask = alive
    if prune:
        V = vertices(tri)
        V = V[tri_live(V)].astype(np.float64)
        lo, hi = V.min(1), V.max(1)
        big = np.abs(V).max((1, 2))
        can = np.zeros(o.shape[0], bool)
        od, rd = np.where(alive[:, None], o, F(0)).astype(np.float64), np.where(alive, r, F(0)).astype(np.float64)
        bc = max(1, PAIRS // max(1, V.shape[0]))
        for i0 in range(0, o.shape[0], bc):
            s = slice(i0, i0 + bc)
            gap = np.sqrt((np.maximum(np.maximum(lo[None] - od[s, None], od[s, None] - hi[None]), 0.0) ** 2).sum(-1))
            can[s] = (gap <= rd[s, None] * (1 + 1e-3) + 1e-4 * np.maximum(big[None], np.abs(od[s]).max(1)[:, None])).any(1)
        ask = alive & can
    win, point = np.full(o.shape[0], -1, np.int32), np.zeros((o.shape[0], 3), F)
    w = np.nonzero(ask)[0]
    if w.size:
        win[w], point[w] = E.closest_point(o[w], tri, r[w])[:2]
    return win, point


def limit(t_max, n):
    """(t_max float32 [n], allowed bool [n])"""
    if t_max is None:
        return np.full(n, INF, F), np.ones(n, bool)
    t_max = np.ascontiguousarray(t_max, F).reshape(n)
    with np.errstate(all="ignore"):
        return t_max, t_max >= 0


def query(rays, radius, tri, t_max=None, table=None, touching=None):
    """(tri_id int32 [n], t [n], point [n, 3], touching uint8 [n], sub int8 [n]): what ezrt_query_sphere_cast_device writes, and the
    sub-candidate that supplied a swept winner (-1 else); `table` = swept_all(...) and `touching` = touch(...), when the caller holds
    them"""
    o, d, r = split(rays, radius)
    V = vertices(tri)
    n = o.shape[0]
    cand, t, sub = (swept_all(rays, radius, tri) if table is None else table)[:3]
    tw, tp = touch(rays, radius, tri) if touching is None else touching
    tm, allowed = limit(t_max, n)
    with np.errstate(all="ignore"):
        ok = cand & allowed[:, None] & (t <= tm[:, None])
    key = np.where(ok, t, INF)
    rows = np.arange(n)
    if V.shape[0]:
        win = np.argmax(ok & (key == key.min(1, keepdims=True)), axis=1)    # the FIRST True: the lowest k at the smallest t
        has = ok[rows, win]
    else:
        win, has = np.zeros(n, np.int64), np.zeros(n, bool)
    is_touch = tw >= 0
    has &= ~is_touch
    point = np.zeros((n, 3), F)
    w = np.nonzero(has)[0]
    if w.size:
        point[w] = pairs(o[w], d[w], r[w], V[win[w]])[3]
    tri_id = np.where(is_touch, tw, np.where(has, win, -1)).astype(np.int32)
    tt = np.where(is_touch, F(0), np.where(has, key[rows, win] if V.shape[0] else INF, INF)).astype(F)
    point = np.where(is_touch[:, None], tp, point).astype(F)
    return tri_id, tt, point, is_touch.astype(np.uint8), np.where(has, sub[rows, win] if V.shape[0] else -1, -1).astype(np.int8)


def at(rays, radius, tri, ids):
    """(t [n], point [n, 3], touching uint8 [n]): what ezrt_sphere_cast_at_device writes for query i against triangle ids[i]"""
    o, d, r = split(rays, radius)
    V = vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    n = ids.size
    good = (ids >= 0) & (ids < V.shape[0]) & live(rays, radius)
    W = V[np.where(good, ids, 0)] if V.shape[0] else np.zeros((n, 3, 3), F)
    oz, dz, rz = np.where(good[:, None], o, F(0)), np.where(good[:, None], d, F(1)), np.where(good, r, F(0))
    q, _, _, d2 = E.per_triangle(oz, W[:, 0], W[:, 1], W[:, 2])
    with np.errstate(all="ignore"):
        is_touch = good & np.isfinite(d2) & (d2 <= rz * rz)
    cand, t, _, point, _, _ = pairs(oz, dz, rz, W)
    cand &= good & ~is_touch
    tt = np.where(is_touch, F(0), np.where(cand, t, INF)).astype(F)
    point = np.where(is_touch[:, None], q, np.where(cand[:, None], point, F(0))).astype(F)
    return tt, point, is_touch.astype(np.uint8)

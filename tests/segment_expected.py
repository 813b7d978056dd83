"""The definition of include/ezrt_segment.h restated in numpy float32 (a helper, no test): the five sub-candidates of a pair in the
header's order, the first smallest finite d2, the crossing step (T1 and the segment test), and the answers of the three calls over
query segments x ALL triangles -- there is no tree here.

Written from the header's comment, not from the kernel: every operation is one numpy float32 operation (one rounding each, numpy does
not contract).  The end points go through closest_point_expected.per_triangle as it stands, the edge pairs through
tri_distance_expected.seg_seg (the header: "the closest points of two closed segments of ezrt_tri_distance.h as they stand"),
liveness of a triangle and the sorting are tri_overlap_expected's, the segment test is self_overlap_expected.seg_meets.  A query is
[a, b]: TWO END POINTS.  Chunked over queries x triangles."""
import numpy as np

import closest_point_expected as E
import self_overlap_expected as SE
import tri_distance_expected as TD
import tri_overlap_expected as TE

F = np.float32
PAIRS = 1 << 18            # segment-triangle pairs evaluated at a time
N_SUB = 5

box_lb = TD.box_lb         # tri_distance_box: the walk's bound and the pair gate


def split(segs):
    """(a, b) float32 [n, 3] of segs [n, 6]"""
    S = np.ascontiguousarray(segs, F).reshape(-1, 6)
    return S[:, :3], S[:, 3:]


def live(segs):
    """bool [n]: six finite numbers"""
    return np.isfinite(np.ascontiguousarray(segs, F).reshape(-1, 6)).all(1)


def sub_candidates(A, B, V):
    """yields (x, y, d2) of the five sub-candidates in the header's order; A, B float32 [..., 3] and V [..., 3, 3] that broadcast"""
    v = [V[..., i, :] for i in range(3)]
    shape = np.broadcast_shapes(A.shape[:-1], V.shape[:-2])
    for e in (A, B):                                                   # an end point against the triangle
        y, _, _, d2 = E.per_triangle(e, v[0], v[1], v[2])
        yield np.broadcast_to(e, shape + (3,)), y, d2
    for j in range(3):                                                 # the segment, FIRST, against an edge
        yield TD.seg_seg(A, B, v[j], v[(j + 1) % 3])


def pair_min(A, B, V, points=True):
    """(found bool, best float32, x, y, sub int8): the first smallest finite d2 of the five, its points (zeros where nothing is finite,
    or None without `points`) and its index (-1)"""
    shape = np.broadcast_shapes(A.shape[:-1], V.shape[:-2])
    found = np.zeros(shape, bool)
    best = np.full(shape, np.inf, F)
    sub = np.full(shape, -1, np.int8)
    bx = np.zeros(shape + (3,), F) if points else None
    by = np.zeros(shape + (3,), F) if points else None
    for i, (x, y, d2) in enumerate(sub_candidates(A, B, V)):
        with np.errstate(all="ignore"):
            take = np.isfinite(d2) & (~found | (d2 < best))
        best = np.where(take, d2, best).astype(F)
        sub = np.where(take, np.int8(i), sub)
        found |= take
        if points:
            bx, by = np.where(take[..., None], x, bx).astype(F), np.where(take[..., None], y, by).astype(F)
    return found, best, bx, by, sub


def t1(A, B, V):
    """bool: the closed fp32 comparison of the segment's bounding box with the triangle's (finite inputs)"""
    qlo, qhi = np.minimum(A, B), np.maximum(A, B)
    return ((qlo <= V.max(-2)) & (V.min(-2) <= qhi)).all(-1)


def meets(A, B, V):
    """bool [p]: T1 && seg_meets(lo, hi; S) for LIVE segments and LIVE triangles, A, B [p, 3], V [p, 3, 3]"""
    out = t1(A, B, V)
    i = np.nonzero(out)[0]
    for p0 in range(0, i.size, TE.PAIRS):
        s = i[p0:p0 + TE.PAIRS]
        a, b = A[s], B[s]
        swap = TE._less(b, a)[:, None]
        out[s] = SE.seg_meets(np.where(swap, b, a), np.where(swap, a, b), TE.sorted_vertices(V[s]))
    return out


def crossing(segs, V, keep=None):
    """bool [n, m]: the crossing step over segments x triangles (False where either is not live); `keep` [n, m] limits the pairs"""
    A, B = split(segs)
    n, m = A.shape[0], V.shape[0]
    ok = live(segs)[:, None] & TE.live(V)[None, :]
    if keep is not None:
        ok &= keep
    with np.errstate(all="ignore"):
        ok &= t1(A[:, None], B[:, None], V[None])                      # (T1 first: the rule is a conjunction)
    out = np.zeros((n, m), bool)
    i, k = np.nonzero(ok)
    out[i, k] = meets(A[i], B[i], V[k])
    return out


def pairs(segs, V):
    """(candidate bool [p], dist2 [p], x [p, 3], y [p, 3], crosses uint8 [p], sub int8 [p]) of segment i against triangle i -- segs
    [p, 6], V float32 [p, 3, 3]; where the pair is no candidate: (False, +inf, zeros, zeros, 0, -1)"""
    A, B = split(segs)
    V = np.ascontiguousarray(V, F).reshape(-1, 3, 3)
    found, best, x, y, sub = pair_min(A, B, V)
    ok = live(segs) & TE.live(V)
    cand = ok & found
    cross = np.zeros(cand.shape, bool)
    i = np.nonzero(cand)[0]
    cross[i] = meets(A[i], B[i], V[i])
    d2 = np.where(cross, F(0), np.where(cand, best, F(np.inf))).astype(F)
    return (cand, d2, np.where(cand[:, None], x, F(0)).astype(F), np.where(cand[:, None], y, F(0)).astype(F), cross.astype(np.uint8),
            np.where(cand, sub, np.int8(-1)))


# With `prune` the pairs that cannot hold a winner, a tie or a member of the capsule are left out BEFORE the restatement is evaluated, by
# tri_distance_expected's argument, which is not the kernel's: in float64 the gap between the two bounding boxes is a lower bound of
# the true distance of the pair, U = the restated dist2 of the query against the SEEDS triangles with the smallest gaps is an upper
# bound of the winner's, and a pair is kept when gap <= max(sqrt(U), reach) * (1 + 1e-3) + 1e-4 * (largest |coordinate| of the two) --
# `reach` the largest d_max or radius the caller will ask about.  A pair left out is reported as no candidate
# (tests/test_segment_expected.py holds the pruned evaluation against the full one).
SEEDS = TD.SEEDS
SLACK_REL, SLACK_ABS = TD.SLACK_REL, TD.SLACK_ABS


def _kept(segs, V, ok, reach):
    A, B = split(segs)
    n, m = A.shape[0], V.shape[0]
    Ad, Bd, Vd = A.astype(np.float64), B.astype(np.float64), V.astype(np.float64)
    with np.errstate(all="ignore"):
        qlo, qhi, lo, hi = np.minimum(Ad, Bd)[:, None], np.maximum(Ad, Bd)[:, None], Vd.min(1)[None], Vd.max(1)[None]
        gap = np.sqrt((np.maximum(np.maximum(lo - qhi, qlo - hi), 0.0) ** 2).sum(-1))
    gap = np.where(ok, gap, np.inf)
    k = min(SEEDS, m)
    seeds = np.argpartition(gap, k - 1, axis=1)[:, :k]
    cand, d2 = pairs(np.repeat(np.ascontiguousarray(segs, F).reshape(-1, 6), k, 0), V[seeds.reshape(-1)])[:2]
    U = np.where(cand, d2, F(np.inf)).reshape(n, k).min(1).astype(np.float64)
    if reach is not None:
        with np.errstate(all="ignore"):
            r = np.asarray(reach, np.float64).reshape(n)
            U = np.maximum(U, np.where(r >= 0, r * r, 0.0))
    scale = np.maximum(np.maximum(np.abs(Ad).max(1), np.abs(Bd).max(1))[:, None], np.abs(Vd).max((1, 2))[None])
    with np.errstate(all="ignore"):
        return ok & ~(gap > np.sqrt(U)[:, None] * (1 + SLACK_REL) + SLACK_ABS * scale)        # (a NaN or infinite bound keeps the pair)


def dist2_all(segs, tri, prune=False, reach=None):
    """(candidate bool [n, m], dist2 float32 [n, m], crosses bool [n, m], sub int8 [n, m]) over segments x ALL triangles"""
    A, B = split(segs)
    V = TE.vertices(tri)
    n, m = A.shape[0], V.shape[0]
    ok = live(segs)[:, None] & TE.live(V)[None, :]
    cand = np.zeros((n, m), bool)
    d2 = np.full((n, m), np.inf, F)
    sub = np.full((n, m), -1, np.int8)
    keep = None
    if prune and m:
        keep = _kept(segs, V, ok, reach)
        i, k = np.nonzero(keep)
        for p0 in range(0, i.size, PAIRS):
            s = slice(p0, p0 + PAIRS)
            found, best, _, _, sb = pair_min(A[i[s]], B[i[s]], V[k[s]], points=False)
            cand[i[s], k[s]] = found
            d2[i[s], k[s]] = best
            sub[i[s], k[s]] = sb
    else:
        bc = max(1, PAIRS // max(1, m))
        for i0 in range(0, n, bc):
            s = slice(i0, min(n, i0 + bc))
            found, best, _, _, sb = pair_min(A[s, None], B[s, None], V[None], points=False)
            cand[s] = found & ok[s]
            d2[s] = best
            sub[s] = sb
    cross = crossing(segs, V, keep) & cand
    return cand, np.where(cross, F(0), np.where(cand, d2, F(np.inf))).astype(F), cross, np.where(cand, sub, np.int8(-1))


bound = TD.bound


def query(segs, tri, d_max=None, table=None, prune=False):
    """(tri_id int32 [n], dist [n], point_query [n, 3], point_scene [n, 3], crosses uint8 [n], sub int8 [n]): what
    ezrt_query_segment_distance_device writes, and the winning sub-candidate's index (-1 for a miss); `table` = dist2_all(segs, tri),
    when the caller holds it"""
    S = np.ascontiguousarray(segs, F).reshape(-1, 6)
    V = TE.vertices(tri)
    n = S.shape[0]
    cand, d2, cross = (dist2_all(S, tri, prune=prune, reach=d_max) if table is None else table)[:3]
    B, allowed = bound(d_max, n)
    with np.errstate(all="ignore"):
        ok = cand & allowed[:, None] & (d2 <= B[:, None])
    key = np.where(ok, d2, F(np.inf))
    tie = ok & (key == key.min(1, keepdims=True)) if V.shape[0] else ok   # the pairs at the smallest dist2 ...
    first = tie & cross                                                # ... of which one that crosses comes before one that does not
    win = np.argmax(np.where(first.any(1, keepdims=True), first, tie), axis=1) if V.shape[0] else np.zeros(n, np.int64)
    r = np.arange(n)
    has = ok[r, win] if V.shape[0] else np.zeros(n, bool)
    tri_id = np.where(has, win, -1).astype(np.int32)
    if V.shape[0]:
        _, _, x, y, _, sub = pairs(S, V[np.where(has, win, 0)])
    else:
        x = y = np.zeros((n, 3), F)
        sub = np.full(n, -1, np.int8)
    with np.errstate(all="ignore"):
        dist = np.where(has, np.sqrt(np.where(has, key[r, win] if V.shape[0] else F(0), F(0))), F(np.inf)).astype(F)
    return (tri_id, dist, np.where(has[:, None], x, F(0)).astype(F), np.where(has[:, None], y, F(0)).astype(F),
            (has & (cross[r, win] if V.shape[0] else False)).astype(np.uint8), np.where(has, sub, np.int8(-1)))


def at(segs, tri, ids):
    """(dist [n], point_query [n, 3], point_scene [n, 3], crosses uint8 [n], dist2 [n]): what ezrt_segment_distance_at_device writes
    for segment i against triangle ids[i], and the pair's dist2 (+inf where it writes the miss)"""
    S = np.ascontiguousarray(segs, F).reshape(-1, 6)
    V = TE.vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    inside = (ids >= 0) & (ids < V.shape[0])
    cand, d2, x, y, cross, _ = pairs(S, V[np.where(inside, ids, 0)])
    cand &= inside
    with np.errstate(all="ignore"):
        dist = np.where(cand, np.sqrt(np.where(cand, d2, F(0))), F(np.inf)).astype(F)
    return (dist, np.where(cand[:, None], x, F(0)).astype(F), np.where(cand[:, None], y, F(0)).astype(F), (cross & cand).astype(np.uint8),
            np.where(cand, d2, F(np.inf)).astype(F))


def capsule_live(segs, radius):
    """bool [n]: a live segment and a finite radius >= 0"""
    r = np.ascontiguousarray(radius, F).reshape(-1)
    with np.errstate(all="ignore"):
        return live(segs) & np.isfinite(r) & (r >= 0)


def within(segs, radius, tri, table=None, prune=False):
    """bool [n, m]: triangle k is in the capsule of query i -- a candidate with dist2 <= R2 = radius*radius in float32"""
    S = np.ascontiguousarray(segs, F).reshape(-1, 6)
    r = np.ascontiguousarray(radius, F).reshape(-1)
    cand, d2 = (dist2_all(S, tri, prune=prune, reach=r) if table is None else table)[:2]
    with np.errstate(all="ignore"):
        R2 = (r * r).astype(F)
        return cand & capsule_live(S, r)[:, None] & (d2 <= R2[:, None])


def capsule(segs, radius, tri, k, table=None, prune=False):
    """(rows int32 [n, k], count int32 [n]): what ezrt_query_capsule_overlap_device writes"""
    return TE.lowest(within(segs, radius, tri, table, prune), k)

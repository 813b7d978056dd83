"""The rule of the plane queries (include/ezrt_plane.h: P1 .. P6) restated in numpy, operation by operation, over ALL triangles -- no
tree, no kernel (a helper, no test).  float64 and float32 numpy arithmetic is IEEE and never contracted, so every line below is one
rounding, as in the header.  tests/test_plane_expected.py holds it against exact rational arithmetic within the header's derived
bound."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 20            # plane-triangle pairs classified at a time


def vertices(tri):
    """float32 [m, 3, 3]: p1 p2 p3 of the scene's triangle rows [m, 36] (or of vertices given as [m, 3, 3] / [m, 9])"""
    T = np.ascontiguousarray(tri, F)
    T = T.reshape(T.shape[0], -1)
    return np.ascontiguousarray(T[:, :9]).reshape(-1, 3, 3)


def live(planes):
    """P1: bool [n]"""
    p = np.ascontiguousarray(planes, F).reshape(-1, 4)
    return np.isfinite(p).all(1) & ~(p[:, :3] == 0).all(1)


def sides(planes, V):
    """P2: s float64 [n, m, 3] of planes [n, 4] against vertices V [m, 3, 3] (whatever the plane: the caller applies P1)"""
    p = np.ascontiguousarray(planes, F).reshape(-1, 4).astype(D)
    V = V.astype(D)
    a, b, c, d = (p[:, k, None, None] for k in range(4))
    with np.errstate(all="ignore"):
        return ((a * V[None, :, :, 0] + b * V[None, :, :, 1]) + c * V[None, :, :, 2]) - d


def crossed_of(s, plane_live, tri_finite):
    """P3: bool [n, m] from s [n, m, 3]"""
    with np.errstate(invalid="ignore"):
        up = s >= 0.0
    return plane_live[:, None] & tri_finite[None, :] & ~up.all(2) & up.any(2)


def _less(x, y):
    return (x[:, 0] < y[:, 0]) | ((x[:, 0] == y[:, 0]) & ((x[:, 1] < y[:, 1]) | ((x[:, 1] == y[:, 1]) & (x[:, 2] < y[:, 2]))))


def edge_point(X, sx, Y, sy):
    """P4: float32 [r, 3], the points of the edges with the ends X, Y (float32 [r, 3]) and their sides (float64 [r]), one UP one DOWN"""
    sw = _less(Y, X)
    A = np.where(sw[:, None], Y, X)
    B = np.where(sw[:, None], X, Y)
    sa = np.where(sw, sy, sx)
    sb = np.where(sw, sx, sy)
    with np.errstate(all="ignore"):
        t = sa / (sa - sb)
        P = (A.astype(D) + t[:, None] * (B.astype(D) - A.astype(D))).astype(F)
    lo = np.where(B < A, B, A)
    hi = np.where(B < A, A, B)
    P = np.where(P < lo, lo, np.where(P > hi, hi, P))
    P = np.where((sa == 0.0)[:, None], A, np.where((sb == 0.0)[:, None], B, P))
    assert P.dtype == F
    return P


def segments(V, s):
    """P5: seg float32 [r, 2, 3] of CROSSED triangles V [r, 3, 3] with the sides s [r, 3]"""
    up = s >= 0.0
    r = np.arange(V.shape[0])
    out = np.zeros((V.shape[0], 2, 3), F)
    for q, want_from_up in ((0, True), (1, False)):
        frm = up if want_from_up else ~up
        e = np.where(frm[:, 0] & ~frm[:, 1], 0, np.where(frm[:, 1] & ~frm[:, 2], 1, 2))   # the directed edge p[e] -> p[e + 1]
        f = (e + 1) % 3
        assert np.all(frm[r, e] & ~frm[r, f])
        out[:, q] = edge_point(V[r, e], s[r, e], V[r, f], s[r, f])
    return out


def classify(planes, tri):
    """crossed bool [n, m], evaluated in blocks of planes"""
    p = np.ascontiguousarray(planes, F).reshape(-1, 4)
    V = vertices(tri)
    lv, fin = live(p), np.isfinite(V).all(axis=(1, 2))
    out = np.zeros((p.shape[0], V.shape[0]), bool)
    step = max(1, PAIRS // max(V.shape[0], 1))
    for i in range(0, p.shape[0], step):
        out[i:i + step] = crossed_of(sides(p[i:i + step], V), lv[i:i + step], fin)
    return out


def section(planes, tri):
    """P6: (offsets int64 [n + 1], tri_id int32 [rows], seg float32 [rows, 2, 3], crossed bool [n, m]) of planes [..., 4], flattened
    row-major"""
    p = np.ascontiguousarray(planes, F).reshape(-1, 4)
    V = vertices(tri)
    cr = classify(p, V)
    i, k = np.nonzero(cr)                                          # row-major: by plane, then by ascending id
    offsets = np.zeros(p.shape[0] + 1, np.int64)
    offsets[1:] = np.cumsum(cr.sum(1))
    pd = p[i].astype(D)
    Vk = V[k]
    Vd = Vk.astype(D)
    s = ((pd[:, 0, None] * Vd[:, :, 0] + pd[:, 1, None] * Vd[:, :, 1]) + pd[:, 2, None] * Vd[:, :, 2]) - pd[:, 3, None]
    return offsets, k.astype(np.int32), segments(Vk, s), cr


def part_of(crossed, S):
    """int32 [n, S]: the crossed triangles per slice j = [j L, (j + 1) L) with L = 64 ceil(ceil(m / S) / 64)"""
    n, m = crossed.shape
    per = -(-m // S)                                               # ceil(m / S)
    L = max(64, 64 * -(-per // 64))
    out = np.zeros((n, S), np.int32)
    for j in range(S):
        out[:, j] = crossed[:, j * L:(j + 1) * L].sum(1)
    return out


def slices_of(n, n_tri, slices):
    """ezrt_plane_slices for slices >= 1: clamped to ceil(n_tri / 64) and 4096, at least 1"""
    return max(1, min(slices, -(-n_tri // 64), 4096))


def section_at(planes, tri, ids):
    """(crosses bool ids.shape, side int8 ids.shape + (3,), seg float32 ids.shape + (2, 3)): plane i against triangle ids[i] (ids [n],
    or [n, K]: a row per plane); an id outside the scene, a plane that is not live, a non-finite triangle: zeros"""
    p = np.ascontiguousarray(planes, F).reshape(-1, 4)
    ids = np.asarray(ids)
    rows = ids.reshape(p.shape[0], -1)
    V = vertices(tri)
    pp = np.repeat(p, rows.shape[1], axis=0)
    kk = rows.reshape(-1).astype(np.int64)
    ok = (kk >= 0) & (kk < V.shape[0])
    Vk = V[np.where(ok, kk, 0)]
    ok &= live(pp) & np.isfinite(Vk).all(axis=(1, 2))
    pd, Vd = pp.astype(D), Vk.astype(D)
    with np.errstate(all="ignore"):
        s = ((pd[:, 0, None] * Vd[:, :, 0] + pd[:, 1, None] * Vd[:, :, 1]) + pd[:, 2, None] * Vd[:, :, 2]) - pd[:, 3, None]
        s = np.where(ok[:, None], s, 0.0)
        up = s >= 0.0
    cr = ok & ~up.all(1) & up.any(1)
    side = np.where(ok[:, None], np.sign(s), 0).astype(np.int8)
    seg = np.zeros((kk.shape[0], 2, 3), F)
    seg[cr] = segments(Vk[cr], s[cr])
    return cr.reshape(ids.shape), side.reshape(ids.shape + (3,)), seg.reshape(ids.shape + (2, 3))


def flipped(tri):
    """the scene's rows with every triangle's winding flipped (p2 and p3 exchanged, their normals too)"""
    T = np.array(tri, F).reshape(-1, 36)
    T[:, 3:6], T[:, 6:9] = T[:, 6:9].copy(), T[:, 3:6].copy()
    T[:, 12:15], T[:, 15:18] = T[:, 15:18].copy(), T[:, 12:15].copy()
    return T


def loop_balance(seg):
    """(the sorted 12-byte patterns of all q0, of all q1): equal on a closed, consistently wound manifold"""
    b = np.ascontiguousarray(seg, F).reshape(-1, 2, 3).view(np.uint32)
    rows = lambda x: x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))]
    return rows(b[:, 0]), rows(b[:, 1])


def signed_area(seg, plane):
    """the area enclosed by the segments of one section about the plane's unit normal: 1/2 sum n . (q0 x q1), float64"""
    s = np.asarray(seg, D).reshape(-1, 2, 3)
    n = np.asarray(plane, D)[:3]
    return 0.5 * float((np.cross(s[:, 0], s[:, 1]) @ n).sum()) / float(np.linalg.norm(n))

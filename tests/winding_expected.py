"""The rule of the winding-number queries (include/ezrt_winding.h: W1 .. W5) restated in numpy, operation by operation, over ALL
triangles -- no tree, no kernel (a helper, no test).  float64 and float32 numpy arithmetic is IEEE and never contracted, so every
line below is one rounding, as in the header; ez_atan2 is include/ezrt_detmath.h's, built from float32 operations.
tests/test_winding_expected.py holds it against a float64 evaluation within the header's derived bound."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 18            # point-triangle pairs evaluated at a time
SCALE = D(2.0 ** 36)
INV_2PI = float.fromhex("0x1.45f306dc9c883p-3")
Q_MAX = 1 << 38            # |q_k| < 2^38
N_TRI_MAX = 1 << 24        # a leaf reference holds 24 bits


def ez_atan_pos(x):
    """ez_atan_pos of include/ezrt_detmath.h on a float32 array x >= 0"""
    x = np.asarray(x, F)
    big = x > F(2.414213562373095)
    mid = ~big & (x > F(0.4142135623730950))
    with np.errstate(all="ignore"):
        y = np.where(big, F(1.5707963267948966), np.where(mid, F(0.7853981633974483), F(0.0))).astype(F)
        x = np.where(big, -(F(1.0) / x), np.where(mid, (x - F(1.0)) / (x + F(1.0)), x)).astype(F)
    z = x * x
    p = F(8.05374449538e-2)
    p = p * z - F(1.38776856032e-1)
    p = p * z + F(1.99777106478e-1)
    p = p * z - F(3.33329491539e-1)
    y = y + (p * z * x + x)
    assert y.dtype == F
    return y


def ez_atan(x):
    x = np.asarray(x, F)
    neg = x < F(0.0)
    y = ez_atan_pos(np.where(neg, -x, x))
    return np.where(neg, -y, y)


def ez_atan2(y, x):
    """ez_atan2 of include/ezrt_detmath.h on float32 arrays"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    PI_F, PIO2_F = F(3.14159265358979323846), F(1.5707963267948966)
    zero = x == F(0.0)
    with np.errstate(all="ignore"):
        a = ez_atan(y / np.where(zero, F(1.0), x))
    a = np.where(x < F(0.0), np.where(y < F(0.0), a - PI_F, a + PI_F), a)
    a = np.where(zero, np.where(y > F(0.0), PIO2_F, np.where(y < F(0.0), -PIO2_F, F(0.0))), a)
    assert a.dtype == F
    return a


def vertices(tri):
    """float32 [m, 3, 3]: p1 p2 p3 of the scene's triangle rows [m, 36] (or of vertices given as [m, 3, 3] / [m, 9])"""
    T = np.ascontiguousarray(tri, F)
    T = T.reshape(T.shape[0], -1)
    return np.ascontiguousarray(T[:, :9]).reshape(-1, 3, 3)


def _less(x, y):
    return (x[:, 0] < y[:, 0]) | ((x[:, 0] == y[:, 0]) & ((x[:, 1] < y[:, 1]) | ((x[:, 1] == y[:, 1]) & (x[:, 2] < y[:, 2]))))


def sorted_vertices(P):
    """W1: (V float32 [m, 3, 3] in the order of the values, sgn float32 [m], live bool [m])"""
    P = np.array(P, F).reshape(-1, 3, 3)
    v = [P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()]
    sgn = np.ones(P.shape[0], F)
    with np.errstate(invalid="ignore"):
        for i, j in ((0, 1), (1, 2), (0, 1)):
            sw = _less(v[j], v[i])
            v[i][sw], v[j][sw] = v[j][sw].copy(), v[i][sw].copy()
            sgn[sw] = -sgn[sw]
        live = np.isfinite(P).all(axis=(1, 2)) & ~(v[0] == v[1]).all(1) & ~(v[1] == v[2]).all(1)
    return np.stack(v, 1), sgn, live


def _block(p, V, sgn, live):
    """(q int64 [n, m], t float32 [n, m]) of points p [n, 3] against sorted triangles"""
    with np.errstate(all="ignore"):
        pd = p.astype(D)[:, None, :]
        a, b, c = (V[None, :, k, :].astype(D) - pd for k in range(3))
        ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
        bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
        cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
        nx = by * cz - bz * cy
        ny = bz * cx - bx * cz
        nz = bx * cy - by * cx
        det = (ax * nx + ay * ny) + az * nz
        la = np.sqrt((ax * ax + ay * ay) + az * az)
        lb = np.sqrt((bx * bx + by * by) + bz * bz)
        lc = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ab = (ax * bx + ay * by) + az * bz
        bc = (bx * cx + by * cy) + bz * cz
        ca = (cx * ax + cy * ay) + cz * az
        den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
        m = np.maximum(np.abs(det), np.abs(den))
        ok = live[None, :] & np.isfinite(p).all(1)[:, None] & (det != 0.0) & np.isfinite(det) & np.isfinite(den) & (m != 0.0)
        ms = np.where(ok, m, 1.0)
        t = ez_atan2((np.where(ok, det, 0.0) / ms).astype(F), (np.where(ok, den, 1.0) / ms).astype(F))
        t = np.where(ok, sgn[None, :] * t, F(0.0)).astype(F)
        q = np.rint(t.astype(D) * SCALE).astype(np.int64)
    return q, t


def terms(points, tri, want_t=False):
    """q_k int64 [n, m] of every point against every triangle (and t float32 [n, m])"""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    V, sgn, live = sorted_vertices(vertices(tri))
    n, m = p.shape[0], V.shape[0]
    q, t = np.zeros((n, m), np.int64), (np.zeros((n, m), F) if want_t else None)
    step = max(1, PAIRS // max(m, 1))
    for i in range(0, n, step):
        q[i:i + step], tt = _block(p[i:i + step], V, sgn, live)
        if want_t:
            t[i:i + step] = tt
    return (q, t) if want_t else q


def winding_of(S):
    """W5: the float32 winding of the int64 sum"""
    return ((np.asarray(S, np.int64).astype(D) * D(2.0 ** -36)) * D(INV_2PI)).astype(F)


def fixed(points, tri, abs_t=False):
    """S int64 [n] (and sum_k |t_k| float64 [n]) without holding the n x m terms"""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    V, sgn, live = sorted_vertices(vertices(tri))
    n, m = p.shape[0], V.shape[0]
    S, A = np.zeros(n, np.int64), np.zeros(n, D)
    step = max(1, PAIRS // max(m, 1))
    for i in range(0, n, step):
        q, t = _block(p[i:i + step], V, sgn, live)
        S[i:i + step] = q.sum(1)
        A[i:i + step] = np.abs(t.astype(D)).sum(1)
    return (S, A) if abs_t else S


def terms_at(points, tri, ids):
    """q int64 ids.shape: the term of point i and triangle ids[i] (ids [n], or [n, K]: a row per point); an id outside the scene gives 0"""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    ids = np.asarray(ids)
    rows = ids.reshape(p.shape[0], -1)
    V, sgn, live = sorted_vertices(vertices(tri))
    out = np.zeros(rows.shape, np.int64)
    for j in range(rows.shape[1]):
        ok = (rows[:, j] >= 0) & (rows[:, j] < V.shape[0])
        k = np.where(ok, rows[:, j], 0)
        for i in range(0, p.shape[0], 512):                         # point i against triangle k[i]: the diagonal of small blocks
            s = slice(i, i + 512)
            q, _ = _block(p[s], V[k[s]], sgn[k[s]], live[k[s]])
            out[s, j] = np.where(ok[s], np.diagonal(q), 0)
    return out.reshape(ids.shape)


def truth(points, tri):
    """(w float64 [n], sum_k |t_k| float64 [n], err float64 [n]): the real-number value as float64 arithmetic gives it -- W2's det
    and den, np.arctan2, the terms summed in float64 -- with W3's convention that a triangle whose plane holds the point (det == 0)
    contributes nothing, and W1's that a triangle with two equal or non-finite vertices does not either.  No sort, no float32, no
    fixed point.  `err` bounds this evaluation's own error as a winding number: det and den are sums of at most 16 products of
    magnitude |a||b||c|, each rounded to 2^-53, and atan2 moves by at most delta / hypot(det, den) for a change delta of its
    arguments -- so err = sum_k 2^-48 |a||b||c| / hypot(det, den) / (2 pi): large where p lies on an edge or a vertex of a triangle
    (the real-number value jumps there, and a float64 evaluation cannot say which side it is on), negligible elsewhere -- and
    infinite where p lies on the face of a triangle to within that rounding (den < 0 and |det| < 2^-44 |a||b||c|: atan2's cut)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3).astype(D)
    P0 = vertices(tri)
    P = P0.astype(D)
    live = np.isfinite(P0).all(axis=(1, 2)) & ~(P0[:, 0] == P0[:, 1]).all(1) & ~(P0[:, 1] == P0[:, 2]).all(1) & ~(P0[:, 0] == P0[:, 2]).all(1)
    n, m = p.shape[0], P.shape[0]
    w, A, err = np.zeros(n, D), np.zeros(n, D), np.zeros(n, D)
    step = max(1, PAIRS // max(m, 1))
    with np.errstate(all="ignore"):
        for i in range(0, n, step):
            a, b, c = (P[None, :, k, :] - p[i:i + step, None, :] for k in range(3))
            det = (a * np.cross(b, c)).sum(-1)
            la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
            ok = live[None, :] & (det != 0.0) & np.isfinite(det) & np.isfinite(den) & np.isfinite(p[i:i + step]).all(1)[:, None]
            t = np.where(ok, np.arctan2(det, den), 0.0)
            e = np.where(live[None, :], 2.0 ** -48 * (la * lb * lc) / np.hypot(det, den), 0.0)
            e = np.where(live[None, :] & (den < 0.0) & (np.abs(det) < 2.0 ** -44 * (la * lb * lc)), np.inf, e)   # (det == 0 included)
            w[i:i + step] = t.sum(1) / (2.0 * np.pi)
            A[i:i + step] = np.abs(t).sum(1)
            err[i:i + step] = e.sum(1) / (2.0 * np.pi)
    return w, A, err


def bound(abs_t, n_tri, w):
    """the header's derived bound on |winding - exact|"""
    return (2.0 ** -22 * np.asarray(abs_t, D) + n_tri * 2.0 ** -37) / (2.0 * np.pi) + 2.0 ** -24 * np.abs(np.asarray(w, D))

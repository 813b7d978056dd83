"""The definition of include/ezrt_inside.h restated in numpy (a helper, no test): G1 .. G6 of the header, in its order, over ALL
triangles -- there is no tree here.

Written from the header's comment, not from the kernel.  The frame of an axis is a permutation of the columns and an exact product
with +-1; G1 - G3 and the sort of the vertices are float32 comparisons; everything after the sort is float64 on the float32 values
converted exactly, one numpy operation (one rounding, numpy does not contract) per written operation.  Chunked over points x
triangles."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 20            # point-triangle pairs evaluated at a time


def frame(x, axis):
    """(s, t, u) of float32 vectors x [..., 3] in the frame of `axis`"""
    x = np.asarray(x, F)
    c = axis >> 1
    g = F(-1.0) if axis & 1 else F(1.0)
    return x[..., (c + 1) % 3], x[..., (c + 2) % 3], g * x[..., c]


def _less(x, y):
    return (x[0] < y[0]) | ((x[0] == y[0]) & ((x[1] < y[1]) | ((x[1] == y[1]) & (x[2] < y[2]))))


def _swap(x, y):
    m = _less(y, x)
    return tuple(np.where(m, b, a) for a, b in zip(x, y)), tuple(np.where(m, a, b) for a, b in zip(x, y))


def sorted_vertices(P, axis):
    """v0, v1, v2 (each a tuple s, t, u of float32 [m]) of triangles P [m, 3, 3] in the frame of `axis`, by the header's three swaps"""
    a, b, c = (frame(P[:, k], axis) for k in range(3))
    with np.errstate(invalid="ignore"):
        a, b = _swap(a, b)
        b, c = _swap(b, c)
        a, b = _swap(a, b)
    return a, b, c


def crossed(ps, pt, pu, P, axis):
    """bool [n, m]: G1 .. G6 for points in the frame (float32 [n] each) against triangles P [m, 3, 3] (float32, not yet in the frame).
    G1 - G3 are evaluated for every pair, G4 - G6 for the pairs that pass them (the same operations on the same values)."""
    with np.errstate(all="ignore"):
        fa, fb, fc = (frame(P[:, k], axis) for k in range(3))
        S, T, U = ps[:, None], pt[:, None], pu[:, None]
        ks = [v[0][None, :] <= S for v in (fa, fb, fc)]
        g1 = (ks[0] | ks[1] | ks[2]) & ~(ks[0] & ks[1] & ks[2])
        g2 = ((fa[1][None] <= T) | (fb[1][None] <= T) | (fc[1][None] <= T)) & ((fa[1][None] >= T) | (fb[1][None] >= T) | (fc[1][None] >= T))
        g3 = (fa[2][None] > U) | (fb[2][None] > U) | (fc[2][None] > U)
        out = g1 & g2 & g3
        i, k = np.nonzero(out)
        v0, v1, v2 = sorted_vertices(P, axis)
        d = lambda x, y: x.astype(D) - y.astype(D)
        ps, pt, pu = ps[i], pt[i], pu[i]
        v0, v1, v2 = (tuple(x[k] for x in v) for v in (v0, v1, v2))
        s1, t1, u1 = (d(v1[j], v0[j]) for j in range(3))
        s2, t2, u2 = (d(v2[j], v0[j]) for j in range(3))
        A = s1 * t2 - t1 * s2
        g4 = np.isfinite(A) & (A != 0)
        qs, qt, qu = d(ps, v0[0]), d(pt, v0[1]), d(pu, v0[2])
        E02 = s2 * qt - t2 * qs
        s12, t12 = d(v2[0], v1[0]), d(v2[1], v1[1])
        rs, rt = d(ps, v1[0]), d(pt, v1[1])
        E = np.where(v1[0] <= ps, s12 * rt - t12 * rs, s1 * qt - t1 * qs)
        g5 = (E02 < 0) != (E < 0)
        Ns = t1 * u2 - u1 * t2
        Nt = u1 * s2 - s1 * u2
        Dp = (Ns * qs + Nt * qt) + A * qu
        g6 = np.isfinite(Dp) & (((Dp < 0) & (A > 0)) | ((Dp > 0) & (A < 0)))
        out[i, k] = g4 & g5 & g6
    return out


def crossings(points, tri, axis):
    """(crossings int32 [n], inside uint8 [n]) of float32 `points` [n, 3] against the scene's triangle array `tri` [m, 36] (p1 p2 p3 in
    floats 0-8; an [m, 9] or [m, 3, 3] array of the vertices alone will do) along `axis` (0..5)"""
    assert 0 <= axis <= 5
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    T = np.ascontiguousarray(tri, F)
    P = (T.reshape(-1, 36)[:, :9] if T.ndim == 2 and T.shape[1] == 36 else T.reshape(-1, 9)).reshape(-1, 3, 3)
    n, m = points.shape[0], P.shape[0]
    count = np.zeros(n, np.int32)
    ps, pt, pu = frame(points, axis)
    finite = np.isfinite(points).all(1)
    pc = max(1, PAIRS // max(1, m))
    for i0 in range(0, n, pc):
        pi = slice(i0, min(n, i0 + pc))
        count[pi] = crossed(ps[pi], pt[pi], pu[pi], P, axis).sum(1)
    count[~finite] = 0
    return count, (count & 1).astype(np.uint8)


def all_axes(points, tri):
    """(crossings int32 [6, n], inside uint8 [6, n])"""
    both = [crossings(points, tri, axis) for axis in range(6)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])

"""The definition of include/ezrt_obb_overlap.h restated in numpy (a helper, no test): the per-box numbers and the live-box rule, H0 ..
H3 of the header, in its order, over boxes x ALL triangles -- there is no tree here --, the lowest-K list and the count, and the two
gates a walk may prune a slot's box on.

Written from the header's comment, not from the kernel.  Everything is float64 on the float32 values converted exactly, one numpy
operation (one rounding, numpy does not contract) per written operation, dot and cross in the header's order; the sort of the vertices
is float32 comparisons.  H0 is the float64 comparison the header states, not the rounded hull of the kernel.  Pairs that the
comparisons reject (a box that is not live, a non-finite vertex, H0) never reach the arithmetic, so nothing here overflows, underflows
or is invalid: the module runs with every numpy warning raised as an error.  Chunked over boxes x triangles."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 20            # box-triangle pairs compared at a time


def vertices(tri):
    """float32 [m, 3, 3] of the scene's triangle array [m, 36] (p1 p2 p3 in floats 0-8; [m, 9] or [m, 3, 3] will do)"""
    T = np.ascontiguousarray(tri, F)
    return (T.reshape(-1, 36)[:, :9] if T.ndim == 2 and T.shape[1] == 36 else T.reshape(-1, 9)).reshape(-1, 3, 3)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _d(x, y):
    return x.astype(D) - y.astype(D)


class Boxes:
    """The numbers of n boxes: c float32 [n, 3], U float64 [n, 3, 3], n float64 [n, 3 (j), 3], r float64 [n, 3], hull_lo and hull_hi
    float64 [n, 3], live bool [n].  The rows of a box with a non-finite number are zeros (it is not live, and never used)."""

    def __init__(self, centre, axes):
        c = np.ascontiguousarray(centre, F).reshape(-1, 3)
        u = np.ascontiguousarray(axes, F).reshape(-1, 3, 3)
        assert c.shape[0] == u.shape[0]
        finite = np.isfinite(c).all(-1) & np.isfinite(u).all((1, 2))
        self.c = np.where(finite[:, None], c, F(0))
        U = np.where(finite[:, None, None], u, F(0)).astype(D)
        with np.errstate(all="raise"):
            self.U = U
            self.n = np.stack([_cross(U[:, (j + 1) % 3], U[:, (j + 2) % 3]) for j in range(3)], 1)
            self.r = np.abs(np.stack([_dot(self.n[:, j], U[:, j]) for j in range(3)], 1))
            h = (np.abs(U[:, 0]) + np.abs(U[:, 1])) + np.abs(U[:, 2])
            self.hull_lo, self.hull_hi = self.c.astype(D) - h, self.c.astype(D) + h
        self.live = finite & (self.r > 0).all(-1)

    def take(self, i):
        b = object.__new__(Boxes)
        for k in ("c", "U", "n", "r", "hull_lo", "hull_hi", "live"):
            setattr(b, k, getattr(self, k)[i])
        return b


def live(centre, axes):
    """bool [n]: twelve finite numbers and r_0, r_1, r_2 > 0"""
    return Boxes(centre, axes).live


def _less(x, y):
    return (x[:, 0] < y[:, 0]) | ((x[:, 0] == y[:, 0]) & ((x[:, 1] < y[:, 1]) | ((x[:, 1] == y[:, 1]) & (x[:, 2] < y[:, 2]))))


def _swap(x, y):
    m = _less(y, x)[:, None]
    return np.where(m, y, x), np.where(m, x, y)


def sorted_vertices(V):
    """v0, v1, v2 (float32 [p, 3] each) of finite triangles V [p, 3, 3], by the header's three swaps"""
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    a, b = _swap(a, b)
    b, c = _swap(b, c)
    a, b = _swap(a, b)
    return a, b, c


def h0(B, V):
    """bool: on every axis some vertex has x <= hull_hi and some vertex has x >= hull_lo; B's rows against V [..., 3 vertices, 3]
    (broadcast: B [p] against V [p, 3, 3], or B [n, 1] rows against V [1, m, 3, 3])"""
    X = V.astype(D)
    return ((X <= B.hull_hi[..., None, :]).any(-2) & (X >= B.hull_lo[..., None, :]).any(-2)).all(-1)


def h1(B, V):
    """bool [p]: H1 for live boxes B [p] against finite triangles V [p, 3, 3]"""
    with np.errstate(all="raise"):
        dv = V.astype(D) - B.c.astype(D)[:, None, :]
        ok = np.ones(V.shape[0], bool)
        for j in range(3):
            p = _dot(B.n[:, None, j, :], dv)                                            # [p, 3 vertices]
            r = B.r[:, j, None]
            ok &= (p <= r).any(1) & (p >= -r).any(1)
    return ok


def h2_h3(B, V):
    """bool [p]: H2 and H3 for live boxes B [p] against finite triangles V [p, 3, 3]"""
    with np.errstate(all="raise"):
        v0, v1, v2 = sorted_vertices(V)
        U = B.U
        N = _cross(_d(v1, v0), _d(v2, v0))
        s = _dot(N, _d(B.c, v0))
        R = (np.abs(_dot(N, U[:, 0])) + np.abs(_dot(N, U[:, 1]))) + np.abs(_dot(N, U[:, 2]))
        ok = np.abs(s) <= R                                                             # H2
        zero = np.zeros(V.shape[0], D)
        for A, Bv, C in ((v0, v1, v2), (v1, v2, v0), (v0, v2, v1)):
            e, q, g = _d(Bv, A), _d(C, A), _d(B.c, A)
            for j in range(3):
                a = _cross(U[:, j], e)
                t, s = _dot(a, q), _dot(a, g)
                R = np.abs(_dot(a, U[:, (j + 1) % 3])) + np.abs(_dot(a, U[:, (j + 2) % 3]))
                ok &= ~((s - R > np.maximum(zero, t)) | (s + R < np.minimum(zero, t)))  # H3: this direction does not separate
    return ok


def _rule(B, V):
    """bool [p] for live boxes B [p] against finite triangles V [p, 3, 3] that pass H0"""
    out = h1(B, V)
    i = np.nonzero(out)[0]
    out[i] = h2_h3(B.take(i), V[i])
    return out


def pairs(centre, axes, V):
    """bool [p]: box i against triangle i -- centre float32 [p, 3], axes float32 [p, 3, 3], V float32 [p, 3, 3]"""
    B, V = Boxes(centre, axes), np.ascontiguousarray(V, F).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):                                                 # (comparisons with a NaN are false)
        out = B.live & np.isfinite(V).all((1, 2)) & h0(B, V)
    i = np.nonzero(out)[0]
    out[i] = _rule(B.take(i), V[i])
    return out


def overlaps(centre, axes, tri):
    """bool [n, m]: every box against every triangle of `tri`"""
    B, V = Boxes(centre, axes), vertices(tri)
    n, m = B.c.shape[0], V.shape[0]
    out = np.zeros((n, m), bool)
    finite = np.isfinite(V).all((1, 2))
    bc = max(1, PAIRS // max(1, m))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, n, bc):
            s = np.arange(i0, min(n, i0 + bc))
            Bs = B.take(s)
            Bs.hull_lo, Bs.hull_hi = Bs.hull_lo[:, None], Bs.hull_hi[:, None]
            out[s] = B.live[s, None] & finite[None, :] & h0(Bs, V[None])
    i, k = np.nonzero(out)
    for p0 in range(0, i.size, PAIRS):
        s = slice(p0, p0 + PAIRS)
        out[i[s], k[s]] = _rule(B.take(i[s]), V[k[s]])
    return out


def at(centre, axes, tri, ids):
    """uint8 [n]: box i against triangle ids[i]; an id outside the scene gives 0"""
    c = np.ascontiguousarray(centre, F).reshape(-1, 3)
    u = np.ascontiguousarray(axes, F).reshape(-1, 3, 3)
    V = vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    ok = (ids >= 0) & (ids < V.shape[0])
    out = np.zeros(ids.shape[0], np.uint8)
    out[ok] = pairs(c[ok], u[ok], V[ids[ok]])
    return out


def lowest(over, k):
    """(tri int32 [n, k], n_overlap int32 [n]) of bool [n, m]: the k lowest overlapping indices of each row, ascending, then -1"""
    n, m = over.shape
    count = over.sum(1).astype(np.int32)
    rows = np.full((n, k), -1, np.int32)
    rank = np.cumsum(over, 1) - 1                                   # the position of an overlapping triangle in its row's list
    i, t = np.nonzero(over & (rank < k))
    rows[i, rank[i, t]] = t
    return rows, count


def query(centre, axes, tri, k):
    """(tri int32 [n, k], n_overlap int32 [n]): what ezrt_query_obb_overlap_device writes"""
    return lowest(overlaps(centre, axes, tri), k)


def hull_passes(B, lo, hi):
    """bool [p]: the first gate -- H0 on the box [lo, hi] (float32 [p, 3]); false for an all-NaN box"""
    with np.errstate(invalid="ignore"):
        return B.live & ((lo.astype(D) <= B.hull_hi) & (hi.astype(D) >= B.hull_lo)).all(-1)


def face_passes(B, lo, hi):
    """bool [p]: the second gate -- for no j is pmin_j > r_j or pmax_j < -r_j, with p_j by the rule's own expression at the corner
    chosen per component by the sign of n_j[c].  A NaN (0 times an infinite bound) fails both comparisons: the box passes."""
    ok = np.ones(lo.shape[0], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        dl, dh = lo.astype(D) - B.c.astype(D), hi.astype(D) - B.c.astype(D)
        for j in range(3):
            n = B.n[:, j]
            pl, ph = n * dl, n * dh
            up = n >= 0
            tmin, tmax = np.where(up, pl, ph), np.where(up, ph, pl)
            pmin, pmax = (tmin[:, 0] + tmin[:, 1]) + tmin[:, 2], (tmax[:, 0] + tmax[:, 1]) + tmax[:, 2]
            ok &= ~((pmin > B.r[:, j]) | (pmax < -B.r[:, j]))
    return ok


def slot_passes(centre, axes, lo, hi):
    """bool [p]: does a walk descend the box [lo[i], hi[i]] for box i -- the hull gate and, behind it, the face gate"""
    B = Boxes(centre, axes)
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    return hull_passes(B, lo, hi) & face_passes(B, lo, hi)

"""The definition of include/ezrt_box_overlap.h restated in numpy (a helper, no test): the live-box rule, H1 .. H3 of the header, in
its order, over boxes x ALL triangles -- there is no tree here -- and the lowest-K list and the count.

Written from the header's comment, not from the kernel.  H1 and the sort of the vertices are float32 comparisons; everything after
the sort is float64 on the float32 values converted exactly, one numpy operation (one rounding, numpy does not contract) per written
operation, the sums left to right and the zero component of an edge axis multiplied and added like the others.  Pairs that the
comparisons reject (a box that is not live, a non-finite vertex, H1) never reach the arithmetic, so nothing here overflows or is
invalid: the module runs with every numpy warning raised as an error.  Chunked over boxes x triangles."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 21            # box-triangle pairs compared at a time


def vertices(tri):
    """float32 [m, 3, 3] of the scene's triangle array [m, 36] (p1 p2 p3 in floats 0-8; [m, 9] or [m, 3, 3] will do)"""
    T = np.ascontiguousarray(tri, F)
    return (T.reshape(-1, 36)[:, :9] if T.ndim == 2 and T.shape[1] == 36 else T.reshape(-1, 9)).reshape(-1, 3, 3)


def live(lo, hi):
    """bool [n]: six finite numbers and lo <= hi on every axis"""
    return np.isfinite(lo).all(-1) & np.isfinite(hi).all(-1) & (lo <= hi).all(-1)


def h1(lo, hi, V):
    """bool: on every axis some vertex has x <= hi and some vertex has x >= lo; lo, hi [..., 3] against V [..., 3 vertices, 3]"""
    return ((V <= hi[..., None, :]).any(-2) & (V >= lo[..., None, :]).any(-2)).all(-1)


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


def _d(x, y):
    return x.astype(D) - y.astype(D)


def _interval(a, lo, hi, A):
    """bmin(a, A), bmax(a, A): a float64 [p, 3]; lo, hi, A float32 [p, 3]"""
    dl, dh = _d(lo, A), _d(hi, A)
    pl, ph = a * dl, a * dh
    up = a >= 0
    tmin, tmax = np.where(up, pl, ph), np.where(up, ph, pl)
    return (tmin[:, 0] + tmin[:, 1]) + tmin[:, 2], (tmax[:, 0] + tmax[:, 1]) + tmax[:, 2]


def h2_h3(lo, hi, V):
    """bool [p]: H2 and H3 for live boxes lo, hi [p, 3] against finite triangles V [p, 3, 3]"""
    with np.errstate(all="raise"):
        v0, v1, v2 = sorted_vertices(V)
        e1, e2 = _d(v1, v0), _d(v2, v0)
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        bmin, bmax = _interval(N, lo, hi, v0)
        ok = (bmin <= 0) & (bmax >= 0)                                                  # H2
        zero = np.zeros(V.shape[0], D)
        for A, B, C in ((v0, v1, v2), (v1, v2, v0), (v0, v2, v1)):
            e, q = _d(B, A), _d(C, A)
            for j in range(3):
                u, w = (j + 1) % 3, (j + 2) % 3
                a = np.zeros((V.shape[0], 3), D)
                a[:, u], a[:, w] = -e[:, w], e[:, u]
                t = (a[:, 0] * q[:, 0] + a[:, 1] * q[:, 1]) + a[:, 2] * q[:, 2]
                bmin, bmax = _interval(a, lo, hi, A)
                ok &= ~((bmin > np.maximum(zero, t)) | (bmax < np.minimum(zero, t)))    # H3: this axis does not separate
    return ok


def pairs(lo, hi, V):
    """bool [p]: box i against triangle i -- lo, hi float32 [p, 3], V float32 [p, 3, 3]"""
    lo, hi, V = np.ascontiguousarray(lo, F), np.ascontiguousarray(hi, F), np.ascontiguousarray(V, F)
    with np.errstate(invalid="ignore"):                                                 # (comparisons with a NaN are false)
        out = live(lo, hi) & np.isfinite(V).all((1, 2)) & h1(lo, hi, V)
    i = np.nonzero(out)[0]
    out[i] = h2_h3(lo[i], hi[i], V[i])
    return out


def overlaps(lo, hi, tri):
    """bool [n, m]: every box of lo, hi (float32 [n, 3]) against every triangle of `tri`"""
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    V = vertices(tri)
    n, m = lo.shape[0], V.shape[0]
    out = np.zeros((n, m), bool)
    finite = np.isfinite(V).all((1, 2))
    with np.errstate(invalid="ignore"):
        alive = live(lo, hi)
        bc = max(1, PAIRS // max(1, m))
        for i0 in range(0, n, bc):
            s = slice(i0, min(n, i0 + bc))
            out[s] = alive[s, None] & finite[None, :] & h1(lo[s, None], hi[s, None], V[None])
    i, k = np.nonzero(out)
    for p0 in range(0, i.size, PAIRS):
        s = slice(p0, p0 + PAIRS)
        out[i[s], k[s]] = h2_h3(lo[i[s]], hi[i[s]], V[k[s]])
    return out


def at(lo, hi, tri, ids):
    """uint8 [n]: box i against triangle ids[i]; an id outside the scene gives 0"""
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    V = vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    ok = (ids >= 0) & (ids < V.shape[0])
    out = np.zeros(ids.shape[0], np.uint8)
    out[ok] = pairs(lo[ok], hi[ok], V[ids[ok]])
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


def query(lo, hi, tri, k):
    """(tri int32 [n, k], n_overlap int32 [n]): what ezrt_query_box_overlap_device writes"""
    return lowest(overlaps(lo, hi, tri), k)

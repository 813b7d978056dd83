"""The definition of include/ezrt_tri_overlap.h restated in numpy (a helper, no test): the live rule, T1 and the 29 directions of T2,
in the header's order, over query triangles x ALL triangles -- there is no tree here -- and the lowest-K list and the count.

Written from the header's comment, not from the kernel.  T1, the sorts of the vertices and the order of the two triangles are float32
comparisons; everything else is float64 on the float32 values converted exactly, one numpy operation (one rounding, numpy does not
contract) per written operation, the sums left to right and the zero component of a direction g x axis_j multiplied and added like
the others.  Triangles with a non-finite coordinate never reach the arithmetic, so nothing here overflows or is invalid: the module
runs with every numpy warning raised as an error.  Chunked over queries x triangles."""
import numpy as np

F = np.float32
D = np.float64
PAIRS = 1 << 20            # query-triangle pairs compared at a time


def vertices(tri):
    """float32 [m, 3, 3] of the scene's triangle array [m, 36] (p1 p2 p3 in floats 0-8; [m, 9] or [m, 3, 3] will do)"""
    T = np.ascontiguousarray(tri, F)
    return (T.reshape(-1, 36)[:, :9] if T.ndim == 2 and T.shape[1] == 36 else T.reshape(-1, 9)).reshape(-1, 3, 3)


def _less(x, y):
    return (x[:, 0] < y[:, 0]) | ((x[:, 0] == y[:, 0]) & ((x[:, 1] < y[:, 1]) | ((x[:, 1] == y[:, 1]) & (x[:, 2] < y[:, 2]))))


def _same(x, y):
    return (x == y).all(1)


def _swap(x, y):
    m = _less(y, x)[:, None]
    return np.where(m, y, x), np.where(m, x, y)


def sorted_vertices(V):
    """float32 [p, 3, 3]: v0 v1 v2 of finite triangles V [p, 3, 3], by the header's three swaps"""
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    a, b = _swap(a, b)
    b, c = _swap(b, c)
    a, b = _swap(a, b)
    return np.stack([a, b, c], 1)


def _d3(x, y):
    return x.astype(D) - y.astype(D)


def _cross(e, f):
    return np.stack([e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1], e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2],
                     e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]], 1)


def normal(S):
    """float64 [p, 3]: N of sorted finite triangles S [p, 3, 3]"""
    return _cross(_d3(S[:, 1], S[:, 0]), _d3(S[:, 2], S[:, 0]))


def prepare(V):
    """(live bool [m], sorted float32 [m, 3, 3]) of triangles V [m, 3, 3]; the sorted vertices of a triangle that is not finite are
    zeros and never used"""
    V = np.ascontiguousarray(V, F).reshape(-1, 3, 3)
    finite = np.isfinite(V).all((1, 2))
    S = np.zeros_like(V)
    alive = finite.copy()
    i = np.nonzero(finite)[0]
    with np.errstate(all="raise"):
        S[i] = sorted_vertices(V[i])
        alive[i] = (normal(S[i]) != 0).any(1)
    return alive, S


def live(V):
    """bool [m]: nine finite numbers and N != (0, 0, 0)"""
    return prepare(V)[0]


def t1(QS, SS):
    """bool: closed overlap of the bounding boxes, QS [..., 3, 3] against SS [..., 3, 3] (finite)"""
    return ((QS.min(-2) <= SS.max(-2)) & (SS.min(-2) <= QS.max(-2))).all(-1)


def _edges(S):
    return [_d3(S[:, 1], S[:, 0]), _d3(S[:, 2], S[:, 1]), _d3(S[:, 2], S[:, 0])]


def t2(QS, SS):
    """bool [p]: T2 for live sorted triangles QS, SS [p, 3, 3]"""
    with np.errstate(all="raise"):
        first = _less(SS[:, 0], QS[:, 0]) | (_same(SS[:, 0], QS[:, 0]) & (
            _less(SS[:, 1], QS[:, 1]) | (_same(SS[:, 1], QS[:, 1]) & _less(SS[:, 2], QS[:, 2]))))
        A = np.where(first[:, None, None], SS, QS)
        B = np.where(first[:, None, None], QS, SS)
        a0 = A[:, 0]
        Ds = [_d3(A[:, 1], a0), _d3(A[:, 2], a0), _d3(B[:, 0], a0), _d3(B[:, 1], a0), _d3(B[:, 2], a0)]
        zero = np.zeros(A.shape[0], D)
        ok = np.ones(A.shape[0], bool)

        def direction(x):
            nonlocal ok
            p = [(x[:, 0] * d[:, 0] + x[:, 1] * d[:, 1]) + x[:, 2] * d[:, 2] for d in Ds]
            amax, amin = np.maximum(np.maximum(zero, p[0]), p[1]), np.minimum(np.minimum(zero, p[0]), p[1])
            bmax, bmin = np.maximum(np.maximum(p[2], p[3]), p[4]), np.minimum(np.minimum(p[2], p[3]), p[4])
            ok &= ~((amax < bmin) | (bmax < amin))

        direction(normal(A))
        direction(normal(B))
        e, f = _edges(A), _edges(B)
        for i in range(3):
            for j in range(3):
                direction(_cross(e[i], f[j]))
        for g in e + f:
            for j in range(3):
                u, w = (j + 1) % 3, (j + 2) % 3
                x = np.zeros((A.shape[0], 3), D)
                x[:, u], x[:, w] = -g[:, w], g[:, u]
                direction(x)
    return ok


def pairs(Q, V):
    """bool [p]: query triangle i against triangle i -- Q, V float32 [p, 3, 3]"""
    (ql, QS), (sl, SS) = prepare(Q), prepare(V)
    out = ql & sl
    i = np.nonzero(out)[0]
    out[i] = t1(QS[i], SS[i])
    i = np.nonzero(out)[0]
    out[i] = t2(QS[i], SS[i])
    return out


def overlaps(tris, tri):
    """bool [n, m]: every query triangle of `tris` (float32 [n, 9]) against every triangle of `tri`"""
    (ql, QS), (sl, SS) = prepare(np.ascontiguousarray(tris, F).reshape(-1, 3, 3)), prepare(vertices(tri))
    n, m = QS.shape[0], SS.shape[0]
    out = np.zeros((n, m), bool)
    bc = max(1, PAIRS // max(1, m))
    for i0 in range(0, n, bc):
        s = slice(i0, min(n, i0 + bc))
        out[s] = ql[s, None] & sl[None, :] & t1(QS[s, None], SS[None])
    i, k = np.nonzero(out)
    for p0 in range(0, i.size, PAIRS):
        s = slice(p0, p0 + PAIRS)
        out[i[s], k[s]] = t2(QS[i[s]], SS[k[s]])
    return out


def at(tris, tri, ids):
    """uint8 [n]: query triangle i against triangle ids[i]; an id outside the scene gives 0"""
    Q = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    V = vertices(tri)
    ids = np.asarray(ids).reshape(-1)
    ok = (ids >= 0) & (ids < V.shape[0])
    out = np.zeros(ids.shape[0], np.uint8)
    out[ok] = pairs(Q[ok], V[ids[ok]])
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


def query(tris, tri, k):
    """(tri int32 [n, k], n_overlap int32 [n]): what ezrt_query_tri_overlap_device writes"""
    return lowest(overlaps(tris, tri), k)

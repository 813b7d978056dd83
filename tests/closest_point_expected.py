"""The definition of include/ezrt_closest_point.h restated in numpy float32 (a helper, no test), and the query points of the
closest-point tests (tests/test_closest_point_expected.py on the CPU, tests/test_gpu_closest_point.py on the device).

Written from the header's comment, not from the kernel: every operation is one numpy float32 operation (one rounding each, numpy does
not contract), dot is x*x' + y*y' + z*z' left to right, the cases are selected with np.where in the header's order, the answer
ranges over ALL triangles -- there is no tree here.  Chunked over points x triangles."""
import numpy as np

F = np.float32
PAIRS = 1 << 19            # point-triangle pairs evaluated at a time


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _min(x, y):            # ez_min: (y < x) ? y : x
    return np.where(y < x, y, x)


def _max(x, y):            # ez_max: (x < y) ? y : x
    return np.where(x < y, y, x)


def per_triangle(p, a, b, c):
    """(q, v, w, dist2) of points p [n, 1, 3] against triangles a, b, c [1, m, 3], all float32: arrays [n, m, ...]"""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        c1 = (d1 <= 0) & (d2 <= 0)
        c2 = (d3 >= 0) & (d4 <= d3)
        c3 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        c4 = (d6 >= 0) & (d5 <= d6)
        c5 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        c6 = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        s = va + vb + vc
        zero, one = F(0), F(1)
        v = np.where(c1, zero, np.where(c2, one, np.where(c3, d1 / (d1 - d3), np.where(c4, zero, np.where(c5, zero, np.where(
            c6, one - w6, vb / s))))))
        w = np.where(c1, zero, np.where(c2, zero, np.where(c3, zero, np.where(c4, one, np.where(c5, d2 / (d2 - d6), np.where(
            c6, w6, vc / s))))))
        v, w = v.astype(F), w.astype(F)
        qp = (a + ab * v[..., None]) + ac * w[..., None]
        lo, hi = _min(_min(a, b), c), _max(_max(a, b), c)
        q = np.where(qp < lo, lo, np.where(qp > hi, hi, qp)).astype(F)
        e = p - q
        return q, v, w, _dot(e, e)


def closest_point(points, tri, d_max=None, with_ties=False):
    """(tri_id int32 [n], point [n, 3], dist [n], bary [n, 2]) -- and, with_ties, the number of triangles at the winner's dist2 -- of
    float32 `points` [n, 3] against the scene's triangle array `tri` [m, 36] (p1 p2 p3 in floats 0-8)."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    P = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    n, m = points.shape[0], P.shape[0]
    with np.errstate(all="ignore"):
        if d_max is None:
            B = np.full(n, np.inf, F)
            allowed = np.ones(n, bool)
        else:
            d_max = np.ascontiguousarray(d_max, F).reshape(n)
            B = d_max * d_max
            allowed = d_max >= 0                                   # (false for a NaN)
    best = np.full(n, np.inf, F)
    win = np.full(n, -1, np.int32)
    point = np.zeros((n, 3), F)
    bary = np.zeros((n, 2), F)
    ties = np.zeros(n, np.int64)
    tc = max(1, min(m, 4096))
    pc = max(1, PAIRS // tc)
    for i0 in range(0, n, pc):
        pi = slice(i0, min(n, i0 + pc))
        p = points[pi, None, :]
        for k0 in range(0, m, tc):                                 # ascending: an equal dist2 of a later chunk never replaces
            ks = slice(k0, min(m, k0 + tc))
            q, v, w, d2 = per_triangle(p, P[None, ks, 0], P[None, ks, 1], P[None, ks, 2])
            with np.errstate(all="ignore"):
                cand = np.isfinite(d2) & (d2 <= B[pi, None]) & allowed[pi, None]
            key = np.where(cand, d2, F(np.inf))
            j = np.argmin(key, axis=1)                             # the FIRST index of the smallest: the lowest k of the chunk
            r = np.arange(j.size)
            has = cand[r, j]
            cb = key[r, j]
            cnt = (cand & (key == cb[:, None])).sum(1)
            better = has & ((win[pi] < 0) | (cb < best[pi]))
            same = has & ~better & (cb == best[pi])
            ties[pi] = np.where(better, cnt, ties[pi] + np.where(same, cnt, 0))
            idx = np.nonzero(better)[0]
            g = idx + i0
            best[g] = cb[idx]
            win[g] = (j[idx] + k0).astype(np.int32)
            point[g] = q[idx, j[idx]]
            bary[g, 0] = v[idx, j[idx]]
            bary[g, 1] = w[idx, j[idx]]
    dist = np.where(win >= 0, np.sqrt(best), F(np.inf)).astype(F)
    out = (win, point, dist, bary)
    return out + (ties,) if with_ties else out


# ---- the query points of the tests

def points_for(tri, nodes, seed):
    """About 2 000 float32 points for the scene (tri [m, 36], nodes [k, 12]): uniform in the inflated bounding box; exactly on the
    surface (vertices, fp32 centroids, edge midpoints); just off vertices, along the vertex normal (the vertex is the nearest point of
    every triangle around it: exact ties); on box planes of the tree; far away at scales 1e3 and 1e6; non-finite or of magnitude
    3e38 (expected to miss).  Returns (points, the index of the first point expected to miss)."""
    rng = np.random.default_rng(seed)
    T = np.ascontiguousarray(tri, F).reshape(-1, 36)
    P = T[:, :9].reshape(-1, 3, 3)
    m = P.shape[0]
    lo, hi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)     # the bulk of the mesh
    size = float(np.max(hi - lo))
    parts = [rng.uniform(lo - 0.3 * size, hi + 0.3 * size, (500, 3))]
    k = rng.integers(0, m, 150)
    parts.append(P[k, rng.integers(0, 3, 150)])
    k = rng.integers(0, m, 150)
    parts.append(((P[k, 0] + P[k, 1]) + P[k, 2]) / F(3))
    k, e = rng.integers(0, m, 150), rng.integers(0, 3, 150)
    parts.append((P[k, e] + P[k, (e + 1) % 3]) * F(0.5))
    k, e = rng.integers(0, m, 400), rng.integers(0, 3, 400)
    nrm = T[:, 9:18].reshape(-1, 3, 3)[k, e].astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    parts.append(P[k, e].astype(np.float64) + nrm * size * 10.0 ** rng.uniform(-4, -2, (400, 1)))
    N = np.ascontiguousarray(nodes, F).reshape(-1, 12)
    on = rng.uniform(lo - 0.1 * size, hi + 0.1 * size, (200, 3))
    node, ax = rng.integers(1, N.shape[0], 200), rng.integers(0, 3, 200)
    plane = N[node, np.where(rng.random(200) < 0.5, 6, 9) + ax]
    on[np.arange(200), ax] = plane
    parts.append(on)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    parts.append(d * np.repeat([1e3, 1e6], 100)[:, None])
    finite = np.concatenate(parts).astype(F)
    finite = finite[rng.permutation(finite.shape[0])]
    bad = rng.uniform(lo, hi, (100, 3)).astype(F)
    vals = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38], F)
    bad[np.arange(100), rng.integers(0, 3, 100)] = vals[np.arange(100) % 5]
    return np.ascontiguousarray(np.concatenate([finite, bad]), F), finite.shape[0]

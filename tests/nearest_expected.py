"""The definition of include/ezrt_nearest.h restated in numpy float32 (a helper, no test), for tests/test_nearest_expected.py on the CPU
and tests/test_gpu_nearest.py on the device.

Built on tests/closest_point_expected.py: dist2 of every point-triangle pair is its per_triangle (the header's fp32 definition, one
numpy operation per written operation), the candidates are masked as its closest_point masks them, and the list is a STABLE argsort of
dist2 over ALL triangles in index order -- so equal dist2 come out by ascending index.  There is no tree here."""
import numpy as np

import closest_point_expected as E

F = np.float32


def dist2_all(points, tri):
    """dist2 [n, m] float32 of float32 `points` [n, 3] against every triangle of `tri` [m, 36]"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    P = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    n, m = points.shape[0], P.shape[0]
    out = np.empty((n, m), F)
    tc = max(1, min(m, 4096))
    pc = max(1, E.PAIRS // tc)
    for i0 in range(0, n, pc):
        p = points[i0:i0 + pc, None, :]
        for k0 in range(0, m, tc):
            ks = slice(k0, min(m, k0 + tc))
            out[i0:i0 + pc, ks] = E.per_triangle(p, P[None, ks, 0], P[None, ks, 1], P[None, ks, 2])[3]
    return out


def nearest(points, tri, k, d_max=None, d2=None):
    """(tri_id int32 [n, k], dist float32 [n, k], count int32 [n]) of float32 `points` [n, 3] against the scene's triangle array `tri`
    [m, 36]; `d2` = dist2_all(points, tri) where the caller has it already"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    if d2 is None:
        d2 = dist2_all(points, tri)
    m = d2.shape[1]
    with np.errstate(all="ignore"):
        if d_max is None:
            B = np.full(n, np.inf, F)
            allowed = np.ones(n, bool)
        else:
            d_max = np.ascontiguousarray(d_max, F).reshape(n)
            B = d_max * d_max
            allowed = d_max >= 0                                       # (false for a NaN)
        cand = np.isfinite(d2) & (d2 <= B[:, None]) & allowed[:, None]
    key = np.where(cand, d2, F(np.inf))
    order = np.argsort(key, axis=1, kind="stable")[:, :k]              # stable: ascending index among equal dist2
    r = np.arange(n)[:, None]
    used = cand[r, order]                                              # (the candidates are a prefix: the others have key inf)
    ids = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, F)
    w = order.shape[1]
    ids[:, :w] = np.where(used, order, -1)
    dist[:, :w] = np.where(used, np.sqrt(np.where(used, key[r, order], F(0))), F(np.inf))
    return ids, dist, cand.sum(1).astype(np.int32)

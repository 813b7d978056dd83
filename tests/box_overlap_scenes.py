"""The boxes of the box-overlap tests on the device (tests/test_gpu_box_overlap.py; a helper, no test): about 2 000 boxes per scene,
drawn with a fixed seed from the kinds that can go wrong -- box planes that coincide with the planes of the tree's slots and of the
triangles' own bounding boxes, boxes without an interior, a box that holds everything, boxes that are not live."""
import numpy as np


def boxes_for(tri, nodes, seed, n=2000):
    """(lo, hi) float32 [n', 3] for the scene's triangle array [m, 36] and the caller's tree [*, 12] (box at floats 6-11)"""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    N = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
    m = P.shape[0]
    blo, bhi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(bhi - blo))
    k = n // 7
    parts = []
    # node boxes of the caller's tree themselves: box planes coincide with slot planes
    sel = rng.integers(0, N.shape[0], k)
    parts.append((N[sel, 6:9], N[sel, 9:12]))
    # triangle bounding boxes
    t = rng.integers(0, m, k)
    parts.append((P[t].min(1), P[t].max(1)))
    # point boxes on vertices and on edge midpoints
    v = P[rng.integers(0, m, k), rng.integers(0, 3, k)]
    t, e = rng.integers(0, m, k), rng.integers(0, 3, k)
    mid = (P[t, e] + P[t, (e + 1) % 3]) * np.float32(0.5)
    parts.append((v, v))
    parts.append((mid, mid))
    # boxes of zero thickness through vertices
    v = P[rng.integers(0, m, k), rng.integers(0, 3, k)]
    half = rng.uniform(0.0, 0.05 * size, (k, 3)).astype(np.float32)
    half[np.arange(k), rng.integers(0, 3, k)] = 0
    parts.append((v - half, v + half))
    # small boxes around points of the surface, most of them a leaf's size, a few larger
    t = rng.integers(0, m, 2 * k)
    w = rng.dirichlet((1, 1, 1), 2 * k).astype(np.float32)
    c = (P[t] * w[:, :, None]).sum(1) + rng.normal(0, 0.01 * size, (2 * k, 3)).astype(np.float32)
    half = (size * 10.0 ** rng.uniform(-3, -0.8, (2 * k, 1)) * rng.uniform(0.3, 1.0, (2 * k, 3))).astype(np.float32)
    parts.append((c - half, c + half))
    # one box that holds the whole scene
    parts.append((P.reshape(-1, 3).min(0)[None], P.reshape(-1, 3).max(0)[None]))
    # boxes that are not live: lo > hi on one axis, a NaN, an infinity
    j = 60
    t = rng.integers(0, m, j)
    lo, hi = P[t].min(1) - np.float32(0.01 * size), P[t].max(1) + np.float32(0.01 * size)
    r, ax = np.arange(j), rng.integers(0, 3, j)
    what = r % 4
    s = what == 0
    lo[r[s], ax[s]], hi[r[s], ax[s]] = hi[r[s], ax[s]], lo[r[s], ax[s]]
    s = what == 1
    lo[r[s], ax[s]] = np.nan
    s = what == 2
    hi[r[s], ax[s]] = np.inf
    s = what == 3
    lo[r[s], ax[s]] = -np.inf
    parts.append((lo, hi))
    lo = np.concatenate([p[0] for p in parts]).astype(np.float32)
    hi = np.concatenate([p[1] for p in parts]).astype(np.float32)
    order = rng.permutation(lo.shape[0])
    return np.ascontiguousarray(lo[order]), np.ascontiguousarray(hi[order])

"""The query triangles of the triangle-overlap tests on the device (tests/test_gpu_tri_overlap.py; a helper, no test): about 2 000
per scene, drawn with a fixed seed from the kinds that can go wrong -- the scene's own triangles in other vertex orders, moved by
nothing and by next to nothing, triangles in the plane of a scene triangle, triangles whose bounding-box planes coincide with the
planes of the tree's slots, one that cuts the whole scene, some far outside, triangles that are not live."""
import numpy as np


def tris_for(tri, nodes, seed, n=2000):
    """float32 [n', 9] for the scene's triangle array [m, 36] and the caller's tree [*, 12] (box at floats 6-11)"""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    N = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
    m = P.shape[0]
    blo, bhi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(bhi - blo))
    k = n // 6
    parts = []
    # the scene's own triangles: as given, vertices rotated, winding reversed
    t = P[rng.integers(0, m, k)]
    how = rng.integers(0, 3, k)
    parts.append(np.stack([x if h == 0 else (np.roll(x, 1, axis=0) if h == 1 else x[::-1]) for x, h in zip(t, how)]))
    # ... translated by a tiny offset, and by exactly zero
    t = P[rng.integers(0, m, k)]
    off = (rng.normal(0, 1e-4 * size, (k, 1, 3)) * (rng.random((k, 1, 1)) < 0.7)).astype(np.float32)
    parts.append(t + off)
    # in the plane of a scene triangle: its medial triangle, and a copy scaled about a vertex
    t = P[rng.integers(0, m, k)]
    half = np.float32(0.5)
    medial = np.stack([(t[:, 0] + t[:, 1]) * half, (t[:, 1] + t[:, 2]) * half, (t[:, 2] + t[:, 0]) * half], 1)
    scale = rng.choice(np.float32([0.5, 2.0, -1.0, 0.25]), (k, 1, 1))
    scaled = t[:, :1] + (t - t[:, :1]) * scale
    parts.append(np.where(rng.random((k, 1, 1)) < 0.5, medial, scaled))
    # vertices on corners of the caller's node boxes: gate planes coincide with slot planes
    sel = rng.integers(0, N.shape[0], k)
    lo, hi = N[sel, 6:9], N[sel, 9:12]
    pick = rng.integers(0, 2, (k, 3, 3)).astype(bool)
    pick[:, 1] = ~pick[:, 0]                                         # two opposite corners, so that the triangle spans the box
    parts.append(np.where(pick, hi[:, None, :], lo[:, None, :]))
    # small triangles at the surface, most of them a leaf's size, a few larger
    t = rng.integers(0, m, 2 * k)
    w = rng.dirichlet((1, 1, 1), 2 * k).astype(np.float32)
    c = (P[t] * w[:, :, None]).sum(1) + rng.normal(0, 0.01 * size, (2 * k, 3)).astype(np.float32)
    r = (size * 10.0 ** rng.uniform(-3, -0.8, (2 * k, 1, 1))).astype(np.float32)
    parts.append(c[:, None, :] + r * rng.normal(0, 1, (2 * k, 3, 3)).astype(np.float32))
    # one triangle that cuts the whole scene, a few far outside it
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    mid, ext = (lo + hi) * half, (hi - lo)
    parts.append((mid + np.float32([[-3, -3, 0], [3, -3, 0.01], [0, 4, -0.01]]) * ext)[None].astype(np.float32))
    parts.append(((hi + 3 * ext)[None, None, :] + rng.normal(0, 1, (8, 3, 3)) * ext).astype(np.float32))
    # triangles that are not live: a NaN, an infinity, collinear vertices, a repeated vertex
    j = 60
    t = P[rng.integers(0, m, j)].copy()
    r, v, ax = np.arange(j), rng.integers(0, 3, j), rng.integers(0, 3, j)
    what = r % 5
    s = what == 0
    t[r[s], v[s], ax[s]] = np.nan
    s = what == 1
    t[r[s], v[s], ax[s]] = np.inf
    s = what == 2
    t[r[s], v[s], ax[s]] = -np.inf
    s = what == 3                                                    # collinear, exactly: p3 = p1 + 2 (p2 - p1) on small integers
    base = np.round(t[s, 0])
    step = np.float32([1, 2, -1])
    t[s] = np.stack([base, base + step, base + 2 * step], 1)
    s = what == 4
    t[r[s], (v[s] + 1) % 3] = t[r[s], v[s]]
    parts.append(t)
    out = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(out[rng.permutation(out.shape[0])].reshape(-1, 9))

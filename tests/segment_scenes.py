"""Scenes and queries of the segment tests (tests/test_segment_expected.py on the CPU, tests/test_gpu_segment.py on the device,
tools/segment_host_check.py; a helper, no test).  A query is [a, b]: TWO END POINTS.

queries_for: about 2 000 (segment, d_max, radius) per scene with a fixed seed.  Lengths run from 0.1 to 10 leaf sizes (leaf_size: twice
the median edge length of the scene -- about what a leaf of four triangles spans).  Kinds: segments that graze the mesh (off a face by
1e-5 .. 1e-3 of the extent, nearly in its plane), that pierce it (through a point of a face, along a direction near its normal), that
clear it (off it by up to a few leaf sizes); tangent segments that pass over an edge or a vertex with their middle; segments along mesh
edges, on parts of them and between vertices of different triangles; segments in the plane of a face and parallel to it; zero-length
segments on, next to and off the mesh; segments anywhere in the bounding box; and the kinds that are not live.  On a scene whose
coordinates are multiples of 1/4 (the voxel solid) also axis-parallel segments with end points on multiples of 1/8: distances,
radii and bounds are then exact, coplanar neighbours tie and the index rule decides.

constructed: pairs with known answers on an integer grid, exact in fp32 -- one scene that holds them all, 64 apart along x."""
import numpy as np

import allhits_scenes as A
import inside_scenes as IS

F = np.float32
NAMES = ("voxel_solid", "bunny", "nasty")
SEED = 2100                                                        # + the scene's index
N_DEAD = 8
MAX_K = 8                                                          # of the bit-for-bit capsule batches


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)


def leaf_size(tri):
    P = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3).astype(np.float64)
    P = P[np.isfinite(P).all((1, 2))]
    return 2.0 * float(np.median(np.linalg.norm(P - np.roll(P, 1, 1), axis=2)))


def dead_queries(lo, hi, rng):
    """float32 [8, 6]: a non-finite number in each place that can hold one"""
    s = rng.uniform(lo, hi, (N_DEAD, 2, 3)).reshape(N_DEAD, 6).astype(F)
    for i, (j, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, np.nan))):
        s[i, j] = v
    s[6] = np.nan
    s[7, :3] = s[7, 3:]
    s[7, 2] = s[7, 5] = np.inf                                         # a == b and not finite
    return s


def queries_for(tri, seed, n=2000):
    """(segs float32 [n', 6], d_max float32 [n'], radius float32 [n']) for the scene's triangle array [m, 36]"""
    rng = np.random.default_rng(seed)
    T = np.ascontiguousarray(tri, F).reshape(-1, 36)
    ok = np.isfinite(T[:, :9]).all(1)
    P = T[ok, :9].reshape(-1, 3, 3).astype(np.float64)
    lo, hi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(hi - lo))
    leaf = leaf_size(tri)
    m = P.shape[0]
    face_n = _unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    out = []

    def length(k, lo_=0.1, hi_=10.0):
        return leaf * 10.0 ** rng.uniform(np.log10(lo_), np.log10(hi_), k)

    def face_point(k):
        t = rng.integers(0, m, k)
        w = rng.dirichlet((1, 1, 1), k)
        return t, (P[t] * w[:, :, None]).sum(1)

    def tangent(t):
        v = np.cross(face_n[t], rng.normal(size=(t.shape[0], 3)))
        return _unit(v)

    def add(c, d, L, along=None):
        """a segment of length L along d whose point at parameter `along` (default: anywhere) is c"""
        u = rng.uniform(0, 1, c.shape[0]) if along is None else along
        out.append(np.concatenate([c - d * (L * u)[:, None], c + d * (L * (1 - u))[:, None]], 1))

    k = n // 16
    sign = lambda k: rng.choice([-1.0, 1.0], k)[:, None]               # noqa: E731
    for _ in range(2):                                                 # graze: nearly in the plane of a face, just off it
        t, p = face_point(k)
        d = _unit(tangent(t) + face_n[t] * rng.normal(size=(k, 1)) * 1e-3)
        add(p + face_n[t] * sign(k) * (size * 10.0 ** rng.uniform(-5, -3, k))[:, None], d, length(k))
    for _ in range(3):                                                 # pierce: through a point of a face
        t, p = face_point(k)
        add(p, _unit(face_n[t] * sign(k) + rng.normal(size=(k, 3)) * 0.5), length(k, 0.3), along=rng.uniform(0.1, 0.9, k))
    for _ in range(2):                                                 # clear: off a face by up to three leaf sizes, any direction
        t, p = face_point(k)
        add(p + face_n[t] * sign(k) * (leaf * rng.uniform(0.3, 3.0, k))[:, None], _unit(rng.normal(size=(k, 3))), length(k, 0.1, 2.0))
    for _ in range(4):                                                 # tangent, the middle over an edge or a vertex, a little off
        t, e = rng.integers(0, m, k), rng.integers(0, 3, k)
        w = np.where(rng.random(k) < 0.3, 0.0, rng.uniform(0, 1, k))[:, None]
        p = P[t, e] * (1 - w) + P[t, (e + 1) % 3] * w
        edge = _unit(P[t, (e + 1) % 3] - P[t, e])
        third = P[t, (e + 2) % 3] - P[t, e]
        outward = -_unit(third - edge * (third * edge).sum(1, keepdims=True))           # in the plane, away from the triangle
        up = _unit(face_n[t] * sign(k) + outward * rng.uniform(0.2, 1.5, (k, 1)))
        d = _unit(np.cross(up, edge) + edge * rng.normal(size=(k, 1)) * 0.5)
        add(p + up * (leaf * 10.0 ** rng.uniform(-3, 0, k))[:, None], d, length(k, 0.5), along=rng.uniform(0.3, 0.7, k))
    t, e = rng.integers(0, m, k), rng.integers(0, 3, k)                # along mesh edges, whole and in part; between vertices
    whole = np.concatenate([P[t, e], P[t, (e + 1) % 3]], 1)
    u = np.sort(rng.uniform(-0.2, 1.2, (k, 2)), 1)
    part = np.concatenate([P[t, e] + (P[t, (e + 1) % 3] - P[t, e]) * u[:, :1], P[t, e] + (P[t, (e + 1) % 3] - P[t, e]) * u[:, 1:]], 1)
    t2 = np.clip(t + rng.integers(-8, 9, k), 0, m - 1)
    between = np.concatenate([P[t, e], P[t2, rng.integers(0, 3, k)]], 1)
    out.extend([whole[:k // 3], part[k // 3:2 * k // 3], between[2 * k // 3:]])
    t = rng.integers(0, m, k)                                          # in the plane of a face, and parallel to it
    w1, w2 = rng.dirichlet((1, 1, 1), k), rng.dirichlet((1, 1, 1), k) * 3 - 1
    a, b = (P[t] * w1[:, :, None]).sum(1), (P[t] * w2[:, :, None]).sum(1)
    off = np.where(rng.random(k) < 0.5, 0.0, leaf * rng.uniform(0.01, 1.0, k))[:, None] * face_n[t] * sign(k)
    out.append(np.concatenate([a + off, b + off], 1))
    z = n // 12                                                        # zero length: on a vertex, on a face, next to it, off it
    t, p = face_point(z)
    p[:z // 4] = P[t[:z // 4], 0]
    p[z // 2:] += face_n[t[z // 2:]] * sign(z - z // 2) * (leaf * 10.0 ** rng.uniform(-4, 0.5, z - z // 2))[:, None]
    out.append(np.concatenate([p, p], 1))
    a = rng.uniform(lo, hi, (k, 3))                                    # anywhere in the bounding box
    add(a, _unit(rng.normal(size=(k, 3))), length(k))
    segs = np.concatenate(out).astype(F)
    if np.all(T[ok, :9] * 4 == np.round(T[ok, :9] * 4)):               # the voxel solid: axis-parallel segments on the 1/8 grid
        g = n // 6
        glo, ghi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
        a = np.round(rng.uniform(glo - 0.5, ghi + 0.5, (g, 3)) * 8) / 8
        b = a.copy()
        b[np.arange(g), rng.integers(0, 3, g)] += rng.choice([-1.0, 1.0], g) * rng.integers(0, 17, g) / 8
        segs = np.concatenate([segs, np.concatenate([a, b], 1).astype(F)])
    segs = np.concatenate([segs, dead_queries(lo, hi, rng)])
    segs = np.ascontiguousarray(segs[rng.permutation(segs.shape[0])], F)
    q = segs.shape[0]
    # d_max and radius: from next to nothing to a few leaf sizes, 0 included; on the grid scene multiples of 1/8
    d_max = (leaf * 10.0 ** rng.uniform(-4, 0.3, q)).astype(F)
    radius = (leaf * np.where(rng.random(q) < 0.5, 10.0 ** rng.uniform(-3, 0, q), rng.uniform(0.5, 4.0, q))).astype(F)
    if np.all(T[ok, :9] * 4 == np.round(T[ok, :9] * 4)):
        grid = np.all(segs * 8 == np.round(segs * 8), axis=1)
        d_max[grid] = (rng.integers(0, 9, int(grid.sum())) / 8).astype(F)
        radius[grid] = (rng.integers(0, 17, int(grid.sum())) / 8).astype(F)
    d_max[::13] = 0.0
    radius[::17] = 0.0
    return segs, d_max, radius


def host_case(name, bunny_small, leaf=None):
    """(tri, nodes, segs, d_max, radius) of the named scene; `leaf` rebuilds the tree with buildBVHwithSAH(leaf), which reorders the
    triangles (the queries stay those of the scene as it comes)"""
    if name == "voxel_solid":
        v = IS.voxel_solid()
        tri, nodes = v["tri"], v["nodes"]
    else:
        tri, nodes, _ = A.scene(name, bunny_small)
    segs, d_max, radius = queries_for(tri, SEED + NAMES.index(name))
    if leaf is not None:
        tri, nodes = IS.build(tri, leaf)
    return tri, nodes, segs, d_max, radius


def caps(segs, free, limited, count, max_k=MAX_K):
    """the shares the tests require of a bit-for-bit batch: `free` and `limited` the restatement's answers (tri, dist, x, y, crosses,
    sub) without and with d_max, `count` the capsules' full counts"""
    tri, dist, _, _, crosses, sub = free
    clear = (tri >= 0) & (crosses == 0)
    won = max(1, int(clear.sum()))
    return dict(crossing=float((crosses == 1).mean()), clear=float((clear & (dist > 0)).mean()),
                miss=float(((limited[0] < 0) & (tri >= 0)).mean()), end=float((sub[clear] <= 1).sum()) / won,
                edge=float((sub[clear] >= 2).sum()) / won, point=float((segs[:, :3] == segs[:, 3:]).all(1).mean()),
                under=float(((count > 0) & (count <= max_k)).mean()), over=float((count > max_k).mean()))


def caps_met(c):
    return (min(c["crossing"], c["clear"], c["miss"], c["under"], c["over"]) >= 0.10 and min(c["end"], c["edge"]) >= 0.20 and
            c["point"] >= 0.05)


# ---- constructed pairs on the triangle (0,0,0) (8,0,0) (0,8,0): (name, a, b, dist2, crosses, x, y, sub); integers, so every number
# below is exact in fp32.  x, y or sub None: not pinned (several features tie in exact arithmetic and rounding decides).
CASES = (
    ("an end point over the face", [2, 2, 3], [3, 2, 7], 9, 0, [2, 2, 3], [2, 2, 0], 0),
    ("the second end point over the face", [3, 2, 7], [2, 2, 3], 9, 0, [2, 2, 3], [2, 2, 0], 1),
    ("an end point over an edge", [4, -3, 4], [4, -8, 9], 25, 0, [4, -3, 4], [4, 0, 0], 0),
    ("an end point over a vertex", [-2, -1, 2], [-6, -5, 2], 9, 0, [-2, -1, 2], [0, 0, 0], 0),
    ("the interior against an edge, skew", [4, -2, -4], [4, -2, 4], 4, 0, [4, -2, 0], [4, 0, 0], 2),
    ("parallel to an edge", [2, -3, 4], [6, -3, 4], 25, 0, None, None, None),
    ("parallel to the face", [1, 1, 2], [3, 2, 2], 4, 0, [1, 1, 2], [1, 1, 0], 0),
    ("piercing the interior of the face", [2, 2, -3], [2, 2, 5], 0, 1, None, None, None),
    ("touching with an end point", [2, 2, 0], [2, 2, 6], 0, 1, [2, 2, 0], [2, 2, 0], 0),
    ("lying in the face", [1, 1, 0], [3, 2, 0], 0, 1, [1, 1, 0], [1, 1, 0], 0),
    ("a point on the triangle", [2, 3, 0], [2, 3, 0], 0, 1, [2, 3, 0], [2, 3, 0], 0),
    ("a point above the triangle", [2, 3, 4], [2, 3, 4], 16, 0, [2, 3, 4], [2, 3, 0], 0),
    ("a point beside the triangle", [-3, 4, 0], [-3, 4, 0], 9, 0, [-3, 4, 0], [0, 4, 0], 0),
    ("crossing the plane beside the triangle", [-3, -4, -3], [-3, -4, 3], 25, 0, [-3, -4, 0], [0, 0, 0], None),
)
PIERCING = 7
SPACING = 64


def constructed(leaf=4):
    """(tri [m, 36], nodes, segs float32 [n, 6], index of each case's triangle [n])"""
    base = F([[0, 0, 0], [8, 0, 0], [0, 8, 0]])
    P, segs = [], []
    for k, c in enumerate(CASES):
        shift = F([SPACING * k, 0, 0])
        P.append(base + shift)
        segs.append(np.concatenate([F(c[1]) + shift, F(c[2]) + shift]))
    filler = [F([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) + F([SPACING * k, 40 + 3 * j, 0]) for k in range(len(CASES)) for j in range(3)]
    tri, nodes = IS.build(IS.tri36(np.stack(P + filler)), leaf)
    V = np.ascontiguousarray(tri, F)[:, :9].reshape(-1, 3, 3)
    where = np.array([int(np.nonzero((V == p).all((1, 2)))[0][0]) for p in P])
    return tri, nodes, np.ascontiguousarray(np.stack(segs), F), where


# ---- the tree shapes of tests/tree_shapes.py

def shape_queries(tri, expect, seed, n=160):
    """(segs float32 [n', 6], d_max [n'], radius [n']): about 200 queries for a shape of tests/tree_shapes.py -- queries_for's, then 24
    short segments through the triangles that no leaf holds and 24 through the duplicated ones (where the shape has such)"""
    import tree_shapes as T
    segs, d_max, radius = queries_for(tri, seed, 2 * n)
    segs, d_max, radius = segs[:n], d_max[:n], radius[:n]
    V = T.vertices(tri).astype(np.float64)
    rng = np.random.default_rng(seed + 7)
    leaf = leaf_size(tri)
    extra = [np.asarray(expect.get("uncovered", []), int), T.copied(tri) if V.shape[0] > 8 else np.zeros(0, int)]
    for ids in extra:
        if ids.size:
            t = np.resize(ids, 24)
            c = (V[t] * rng.dirichlet((1, 1, 1), 24)[:, :, None]).sum(1)
            d = _unit(rng.normal(size=(24, 3))) * leaf * rng.uniform(0.05, 0.5, (24, 1))
            off = np.where(np.arange(24) % 2 == 0, 0.0, 2.0)[:, None] * d                # through the triangle, and next to it
            segs = np.concatenate([segs, np.concatenate([c - d + off, c + d + off], 1).astype(F)])
            d_max = np.concatenate([d_max, (leaf * rng.uniform(0.0, 2.0, 24)).astype(F)])
            radius = np.concatenate([radius, (leaf * rng.uniform(0.0, 2.0, 24)).astype(F)])
    return np.ascontiguousarray(segs, F), np.ascontiguousarray(d_max, F), np.ascontiguousarray(radius, F)

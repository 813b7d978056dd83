"""Scenes and query triangles of the triangle-distance tests (tests/test_tri_distance_expected.py on the CPU,
tests/test_gpu_tri_distance.py on the device, tools/tri_distance_host_check.py; a helper, no test).

tris_for: about 2 000 query triangles per scene with a fixed seed -- half of them tests/tri_overlap_scenes.py's (the scene's own
triangles in other vertex orders, moved by nothing and by next to nothing, coplanar ones, corners of node boxes, small ones at the
surface, far ones, triangles that are not live), half a second mesh: triangles of the scene turned and moved to graze it (off the
surface by 1e-5 .. 1e-3 of its size), to cross it and to clear it (by 0.05 .. 0.5 of its size).

constructed: pairs with known answers on an integer grid, exact in fp32 -- one scene that holds them all, 64 apart along x."""
import numpy as np

import allhits_scenes as A
import inside_scenes as IS
import tri_overlap_scenes as TS

F = np.float32
NAMES = ("voxel_solid", "bunny", "nasty")
SEED = 1900                                                        # + the scene's index


def second_mesh(tri, rng, n):
    """float32 [n, 3, 3]: triangles of the scene turned about their centroids and moved along their normals"""
    P = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3).astype(np.float64)
    blo, bhi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(bhi - blo))
    t = P[rng.integers(0, P.shape[0], n)]
    c = t.mean(1, keepdims=True)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    kind = np.arange(n) % 3                                            # graze, cross, clear
    sign = rng.choice([-1.0, 1.0], n)
    off = size * np.where(kind == 0, 10.0 ** rng.uniform(-5, -3, n), np.where(kind == 1, rng.uniform(0, 0.02, n), rng.uniform(0.05, 0.5, n)))
    angle = np.where(kind == 0, rng.uniform(0, 1e-3, n), rng.uniform(0, np.pi, n))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    v = (t - c) * rng.uniform(0.5, 2.0, (n, 1, 1))
    ax = axis[:, None, :]
    ca, sa = np.cos(angle)[:, None, None], np.sin(angle)[:, None, None]
    v = v * ca + np.cross(ax, v) * sa + ax * (ax * v).sum(-1, keepdims=True) * (1 - ca)   # Rodrigues
    return (c + v + (nrm * (sign * off)[:, None])[:, None, :]).astype(F)


def tris_for(tri, nodes, seed, n=2000):
    """float32 [n', 9] for the scene's triangle array [m, 36] and the caller's tree [*, 12]"""
    rng = np.random.default_rng(seed)
    a = TS.tris_for(tri, nodes, seed + 50, n // 2)
    b = second_mesh(tri, rng, n - n // 2).reshape(-1, 9)
    out = np.concatenate([a, b]).astype(F)
    return np.ascontiguousarray(out[rng.permutation(out.shape[0])])


def host_case(name, bunny_small, leaf=None):
    """(tri, nodes, query triangles) of the named scene; `leaf` rebuilds the tree with buildBVHwithSAH(leaf), which reorders the
    triangles (the queries stay those of the scene as it comes)"""
    if name == "voxel_solid":
        v = IS.voxel_solid()
        tri, nodes = v["tri"], v["nodes"]
    else:
        tri, nodes, _ = A.scene(name, bunny_small)
    q = tris_for(tri, nodes, SEED + NAMES.index(name))
    if leaf is not None:
        tri, nodes = IS.build(tri, leaf)
    return tri, nodes, q


# ---- constructed pairs: (name, scene triangle, query triangle, dist2, crosses); integers, so every number below is exact in fp32
CASES = (
    ("parallel faces at distance 3", [[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 0, 3], [4, 0, 3], [0, 4, 3]], 9, 0),
    ("edge-edge, skew", [[0, 0, 0], [4, 0, 0], [2, -4, 0]], [[2, 2, -2], [2, 2, 2], [2, 6, 0]], 4, 0),
    ("edge-edge, parallel", [[0, 0, 0], [4, 0, 0], [2, -4, 0]], [[-2, 0, 3], [6, 0, 3], [2, 4, 3]], 9, 0),
    ("edge-edge, parallel and coplanar", [[0, 0, 0], [4, 0, 0], [2, -4, 0]], [[1, 3, 0], [3, 3, 0], [2, 7, 0]], 9, 0),
    ("vertex of the query over a face", [[0, 0, 0], [8, 0, 0], [0, 8, 0]], [[2, 2, 5], [2, 3, 9], [3, 2, 9]], 25, 0),
    ("vertex of the scene under a face", [[2, 2, 5], [2, 3, 9], [3, 2, 9]], [[0, 0, 0], [8, 0, 0], [0, 8, 0]], 25, 0),
    ("an edge pierces a face", [[0, 0, 0], [8, 0, 0], [0, 8, 0]], [[2, 2, -3], [2, 2, 3], [2, 20, 0]], 0, 1),
    ("touching at a vertex", [[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[0, 0, 0], [-4, 0, 3], [0, -4, 3]], 0, 1),
    ("identical copies", [[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[1, 1, 2], [2, 1, 2], [1, 2, 2]], 4, 0),
)
PIERCING = 6
COPIES = 8
N_COPIES = 3
SPACING = 64


def constructed(leaf=4):
    """(tri [m, 36], nodes, queries float32 [n, 9], scene triangle of each query [n, 3, 3], dist2 float32 [n], crosses uint8 [n])"""
    P, Q = [], []
    for k, (_, s, q, _, _) in enumerate(CASES):
        shift = F([SPACING * k, 0, 0])
        P.append(F(s) + shift)
        Q.append(F(q) + shift)
    filler = [F([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) + F([SPACING * k, 40 + 3 * j, 0]) for k in range(len(CASES)) for j in range(3)]
    copies = [P[COPIES]] * (N_COPIES - 1)
    tri, nodes = IS.build(IS.tri36(np.stack(P + filler + copies)), leaf)
    return (tri, nodes, np.ascontiguousarray(np.stack(Q).reshape(-1, 9), F), np.stack(P), F([c[3] for c in CASES]),
            np.uint8([c[4] for c in CASES]))


# ---- the tree shapes of tests/tree_shapes.py

N_SHAPE_QUERIES = 192
N_TIES = 8


def tie_tris(tri, n=N_TIES):
    """(float32 [n, 9], h [n]): query triangles parallel to an axis-aligned triangle of the scene, h = 1/4 or 1/2 off its inside, kept
    where that triangle is the winner: on a scene whose coordinates are multiples of 1/4 every coordinate here is a multiple of 1/16,
    so the distance h, the radius h * h that d_max = h gives, the winner's dist2 and the lb of the winner's own bounding box against
    the query's are one float32 on the bits.  A walk that skips a box at lb == radius instead of descending it loses these winners."""
    import tri_distance_expected as TD
    V = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    flat = [t for t in range(V.shape[0]) if (V[t] == V[t, :1]).all(0).sum() == 1]
    flat = sorted(flat, key=lambda t: V[t].tobytes())[::3][:160]     # (by value: the same triangles in whatever order the scene holds them)
    axis = np.array([int(np.argmax((V[t] == V[t, :1]).all(0))) for t in flat])
    T = V[flat]
    w = F([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]])
    inner = np.einsum("vk,tkc->tvc", w, T).astype(F)                  # a smaller triangle inside each: exact
    found, hs = [], []
    for h in (0.25, -0.25, 0.5, -0.5):
        q = inner.copy()
        q[np.arange(len(flat)), :, axis] += F(h)
        win, dist = TD.query(q.reshape(-1, 9), tri, prune=True)[:2]
        W = V[np.maximum(win, 0)]
        lb = TD.box_lb(q.min(1), q.max(1), W.min(1), W.max(1))
        ok = (win == np.array(flat)) & (dist == F(abs(h))) & (lb == F(h * h))
        found.append(q[ok][:n // 4])
        hs.append(np.full(found[-1].shape[0], abs(h), F))
    found, hs = np.concatenate(found), np.concatenate(hs)
    assert found.shape[0] == n, found.shape
    return np.ascontiguousarray(found.reshape(-1, 9), F), hs


def shape_queries(tri, nodes, seed):
    """(float32 [n, 9], index of the first tie query or n): about 200 query triangles for a shape of tests/tree_shapes.py, the last
    eight of them tie_tris where the shape has more than 8 triangles"""
    q = tris_for(tri, nodes, seed, 2 * N_SHAPE_QUERIES)[:N_SHAPE_QUERIES]
    if tri.shape[0] <= 8:
        return q, q.shape[0]
    return np.ascontiguousarray(np.concatenate([q, tie_tris(tri)[0]]), F), q.shape[0]

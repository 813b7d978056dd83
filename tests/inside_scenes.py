"""The voxel solid of the inside tests (tests/test_inside_expected.py on the CPU, tests/test_gpu_inside.py on the device), its query
points and their truth (a helper, no test).

voxel_solid(): the boundary of a union of unit cubes on a 7^3 integer grid -- the voxels whose centre lies within 2.6 of the grid's
centre, minus a one-voxel tunnel along z through the middle: genus 1, concave edges, flat faces meeting at right angles.  Boundary
faces only, two triangles each, vertices shared by value.  Every coordinate is a small integer, so any sensible formulation of a
crossing rule is exact on it, and the truth is the occupancy grid itself: it owes nothing to any code under test.

Query points: every voxel centre (never on the surface), every point with two integer coordinates and one half-integer one (on a
grid line: the rays along two of the axes run exactly through mesh vertices, the rays along the third exactly along mesh edges and
inside the planes of faces), and every all-integer point (a grid vertex).  A point is inside if every voxel whose closed cube
contains it is occupied, outside if none is, and otherwise on the surface and left out."""
import itertools

import numpy as np

from ezrt_amd import scene as S

G = 7                      # voxels per axis
RADIUS = 2.6


def occupancy():
    """bool [7, 7, 7]: voxel (i, j, k) is the cube [i, i + 1] x [j, j + 1] x [k, k + 1]"""
    c = np.arange(G) + 0.5 - G / 2.0
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    occ = x * x + y * y + z * z <= RADIUS * RADIUS
    occ[G // 2, G // 2, :] = False                                  # the tunnel, along z
    assert not occ[0].any() and not occ[-1].any() and not occ[:, 0].any() and not occ[:, -1].any() and not occ[:, :, 0].any() \
        and not occ[:, :, -1].any()
    return occ


def boundary_triangles(occ):
    """float32 [m, 3, 3]: two triangles for every face between an occupied voxel and an empty one, wound outwards"""
    pad = np.zeros(tuple(n + 2 for n in occ.shape), bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    out = []
    for i, j, k in zip(*np.nonzero(occ)):
        for axis, side in itertools.product(range(3), (0, 1)):
            nb = [i + 1, j + 1, k + 1]
            nb[axis] += 2 * side - 1
            if pad[tuple(nb)]:
                continue
            a, b = (axis + 1) % 3, (axis + 2) % 3
            base = np.array([i, j, k], np.float64)
            base[axis] += side
            ea, eb = np.zeros(3), np.zeros(3)
            ea[a], eb[b] = 1.0, 1.0
            q = [base, base + ea, base + ea + eb, base + eb]        # counter-clockwise seen from +axis
            if not side:
                q = q[::-1]
            out.append([q[0], q[1], q[2]])
            out.append([q[0], q[2], q[3]])
    return np.asarray(out, np.float32)


def tri36(P):
    """the scene's triangle rows [m, 36] of vertices P [m, 3, 3]: flat normals, one material"""
    P = np.asarray(P, np.float32).reshape(-1, 3, 3)
    n = P.shape[0]
    T = np.zeros((n, 36), np.float32)
    T[:, :9] = P.reshape(n, 9)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    T[:, 9:18] = np.tile(nrm.astype(np.float32), 3)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    return T


def build(T, leaf=4):
    """(tri, nodes) as scene_create takes them: HostScene.addTriangles + buildBVHwithSAH"""
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(T, np.float32))
    hs.buildBVHwithSAH(leaf)
    return hs.encode()


def query_points(occ):
    """(points float32 [n, 3], inside bool [n], kept bool [n], kind int [n]: 0 voxel centre, 1 on a grid line, 2 a grid vertex)"""
    half = np.arange(G) + 0.5
    whole = np.arange(G + 1).astype(np.float64)
    sets = [(0, np.stack(np.meshgrid(half, half, half, indexing="ij"), -1).reshape(-1, 3))]
    for axis in range(3):
        c = [whole, whole, whole]
        c[axis] = half
        sets.append((1, np.stack(np.meshgrid(*c, indexing="ij"), -1).reshape(-1, 3)))
    sets.append((2, np.stack(np.meshgrid(whole, whole, whole, indexing="ij"), -1).reshape(-1, 3)))
    pts = np.concatenate([p for _, p in sets])
    kind = np.concatenate([np.full(p.shape[0], k) for k, p in sets])
    pad = np.zeros(tuple(n + 2 for n in occ.shape), bool)           # a cube outside the grid is empty
    pad[1:-1, 1:-1, 1:-1] = occ
    every = np.ones(pts.shape[0], bool)
    some = np.zeros(pts.shape[0], bool)
    for i, p in enumerate(pts):
        cells = [[int(np.floor(x))] if x != np.floor(x) else [int(x) - 1, int(x)] for x in p]
        got = [pad[a + 1, b + 1, c + 1] for a in cells[0] for b in cells[1] for c in cells[2]]
        every[i], some[i] = all(got), any(got)
    return np.ascontiguousarray(pts, np.float32), every, every | ~some, kind


_solid = None


def voxel_solid():
    """dict: tri [m, 36] and nodes (as scene_create takes them), occ, points, truth (bool), kept (bool), kind -- built once"""
    global _solid
    if _solid is None:
        occ = occupancy()
        tri, nodes = build(tri36(boundary_triangles(occ)))
        pts, truth, kept, kind = query_points(occ)
        _solid = dict(tri=tri, nodes=nodes, occ=occ, points=pts, truth=truth, kept=kept, kind=kind)
    return _solid


def surface_points(tri, nodes, seed, n=600):
    """float32 points exactly on vertices, edge midpoints and box planes of the tree (a third each): what the bit comparisons of the
    other scenes add to tests/closest_point_expected.py's points_for"""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    m = P.shape[0]
    lo, hi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(hi - lo))
    k = n // 3
    t = rng.integers(0, m, k)
    parts = [P[t, rng.integers(0, 3, k)]]
    t, e = rng.integers(0, m, k), rng.integers(0, 3, k)
    parts.append((P[t, e] + P[t, (e + 1) % 3]) * np.float32(0.5))
    N = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
    on = rng.uniform(lo - 0.1 * size, hi + 0.1 * size, (n - 2 * k, 3)).astype(np.float32)
    node, ax = rng.integers(1, N.shape[0], n - 2 * k), rng.integers(0, 3, n - 2 * k)
    on[np.arange(n - 2 * k), ax] = N[node, np.where(rng.random(n - 2 * k) < 0.5, 6, 9) + ax]
    parts.append(on)
    return np.ascontiguousarray(np.concatenate(parts), np.float32)

"""The scenes and planes of the plane-query tests (tests/test_plane_expected.py on the CPU, tests/test_gpu_plane.py on the device,
tools/plane_host_check.py) -- a helper, no test.

Scenes: those of tests/winding_scenes.py -- the voxel solid (closed, integer coordinates), `open_solid`, the small Bunny, "nasty"
(slivers, a coplanar grid, duplicates, a far cluster) and `not_nested`.
Planes, by KIND: 0 through the centroid of a randomly chosen triangle with a random normal (a random plane in the Bunny scene's box
mostly cuts its floor only); 1 axis planes EXACTLY through vertex coordinates, with both signs of the normal (vertices on the plane,
triangles in the plane, zero-length segments); 2 planes that miss everything; 3 planes that are not live: a zero normal, NaN and
infinite entries."""
import numpy as np

import plane_expected as PE
import winding_scenes as WS

CPU_NAMES = WS.CPU_NAMES
GPU_NAMES = WS.GPU_NAMES
SEED = 2400
KIND_CENTROID, KIND_AXIS, KIND_MISS, KIND_DEAD = 0, 1, 2, 3


def scene(name, bunny_small):
    """(tri [m, 36], nodes) as scene_create takes them"""
    return WS.scene(name, bunny_small)


def planes_for(tri, seed, n_random=48, n_axis=8):
    """(planes float32 [n, 4], kind int [n])"""
    rng = np.random.default_rng(seed)
    V = PE.vertices(tri)
    ok = np.isfinite(V).all(axis=(1, 2))
    Vf = V[ok]
    out, kind = [], []
    # 0: through centroids, random normals of any length
    k = rng.integers(0, Vf.shape[0], n_random)
    c = Vf[k].astype(np.float64).mean(1)
    nrm = rng.normal(size=(n_random, 3)) * rng.choice([0.01, 1.0, 37.0], n_random)[:, None]
    p = np.concatenate([nrm, (nrm * c).sum(1, keepdims=True)], 1).astype(np.float32)
    out.append(p), kind.append(np.full(n_random, KIND_CENTROID))
    # 1: axis planes exactly through vertex coordinates, both signs
    rows = []
    for axis in range(3):
        vals = np.unique(Vf[:, :, axis])
        for v in vals[np.linspace(0, vals.size - 1, min(n_axis, vals.size)).astype(np.int64)]:
            for sign in (1.0, -1.0):
                row = np.zeros(4, np.float32)
                row[axis], row[3] = sign, np.float32(sign) * v
                rows.append(row)
    out.append(np.asarray(rows, np.float32)), kind.append(np.full(len(rows), KIND_AXIS))
    # 2: misses
    lo, hi = Vf.reshape(-1, 3).min(0).astype(np.float64), Vf.reshape(-1, 3).max(0).astype(np.float64)
    far = float(np.abs(np.concatenate([lo, hi])).max()) * 3 + 10
    miss = np.float32([[1, 0, 0, far], [0, -1, 0, far], [0, 0, 2, -2 * far], [1, 1, 1, 4 * far], [-0.0, 0.0, 1e-30, 1.0]])
    out.append(miss), kind.append(np.full(miss.shape[0], KIND_MISS))
    # 3: not live
    mid = (lo + hi) / 2
    dead = np.float32([[0, 0, 0, 0], [0, -0.0, 0, 1], [np.nan, 0, 1, mid[2]], [1, np.nan, 0, mid[0]], [0, 1, np.nan, mid[1]],
                       [0, 0, 1, np.nan], [np.inf, 0, 0, mid[0]], [0, -np.inf, 1, mid[1]], [0, 0, 1, np.inf], [1, 0, 0, -np.inf]])
    out.append(dead), kind.append(np.full(dead.shape[0], KIND_DEAD))
    return np.ascontiguousarray(np.concatenate(out), np.float32), np.concatenate(kind)


def inputs(name, bunny_small):
    """(tri, nodes, planes float32 [n, 4], kind int [n])"""
    tri, nodes = scene(name, bunny_small)
    planes, kind = planes_for(tri, SEED + GPU_NAMES.index(name))
    return tri, nodes, planes, kind

"""The scenes and planes of the plane-clipping tests (tests/test_clip_expected.py on the CPU, tests/test_gpu_clip.py on the device) --
a helper, no test.  numpy, and the builders of tests/orient_scenes.py, topology_scenes.py, winding_scenes.py and plane_scenes.py.

  cube_pow2      orient_scenes: 12 triangles with corners in {0, 4}^3, wound outwards -- closed; exact volumes
  voxel_solid    winding_scenes: the voxel solid's triangles, integer coordinates -- closed
  torus32        topology_scenes.torus(32): 2048 triangles with shuffled ids -- closed
  bunny          the small Bunny: open (four holes)
  nasty          winding_scenes: slivers, a coplanar grid, duplicates, a far cluster
  dead           topology_scenes: NaN, infinities and degenerate triangles interleaved with live ones
  signed_zero    topology_scenes: a shared edge stored with +0 and with -0

rows(name, bunny_small) are the triangles with a seeded random normal at every corner and a seeded random material in every row, so
that K5 has something to interpolate and a copied float is told from its neighbours.  planes(name, bunny_small) are those of
plane_scenes.planes_for (all four kinds) and, kind 4, planes through the three vertices of a triangle, computed in fp32: vertices
within rounding of the plane."""
import numpy as np

import orient_scenes as OS
import plane_expected as PE
import plane_scenes as PS
import topology_scenes as TS
import winding_scenes as WS

F = np.float32
SEED = 3400
NAMES = ("cube_pow2", "voxel_solid", "torus32", "bunny", "nasty", "dead", "signed_zero")
CLOSED = ("cube_pow2", "voxel_solid", "torus32")
KIND_NEAR = 4
_cache = {}


def decorate(V, seed):
    """rows [n, 36] of vertices V [n, 3, 3]: random corner normals (not unit: K5 does not renormalise) and a random material"""
    V = np.ascontiguousarray(V, F).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    T = np.zeros((V.shape[0], 36), F)
    T[:, :9] = V.reshape(-1, 9)
    T[:, 9:18] = rng.normal(size=(V.shape[0], 9)).astype(F)
    T[:, 18:] = rng.random((V.shape[0], 18)).astype(F)
    return T


def triangles(name, bunny_small=None):
    if name == "cube_pow2":
        return OS.triangles("cube_pow2")
    if name == "torus32":
        return TS.torus(32)
    if name in ("dead", "signed_zero"):
        return TS.triangles(name)
    return np.ascontiguousarray(WS.scene(name, bunny_small)[0][:, :9].reshape(-1, 3, 3), F)


def rows(name, bunny_small=None):
    """float32 [n, 36], built once and handed out read-only"""
    if name not in _cache:
        T = decorate(triangles(name, bunny_small), SEED + NAMES.index(name))
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def near_planes(V, seed, n=4):
    """planes through the three vertices of seeded random finite triangles, normal and offset computed in fp32"""
    rng = np.random.default_rng(seed)
    V = V[np.isfinite(V).all(axis=(1, 2))]
    out = []
    for k in rng.integers(0, V.shape[0], 4 * n):
        a, b, c = V[k]
        nrm = np.cross(b - a, c - a).astype(F)
        if np.isfinite(nrm).all() and nrm.any():
            out.append(np.append(nrm, F(nrm @ a)).astype(F))
    return np.asarray(out[:n], F).reshape(-1, 4)


def planes(name, bunny_small=None, n_random=8, n_axis=2):
    """(planes float32 [n, 4], kind int [n])"""
    R = rows(name, bunny_small)
    seed = SEED + 100 + NAMES.index(name)
    p, kind = PS.planes_for(R, seed, n_random=n_random, n_axis=n_axis)
    near = near_planes(PE.vertices(R), seed + 50)
    return np.concatenate([p, near]), np.concatenate([kind, np.full(near.shape[0], KIND_NEAR)])


def rotate_rows(T, k):
    """rows with the vertices (and their normals) rotated by k[row] places within the winding: vertex j becomes vertex j - k"""
    T = np.array(T, F)
    k = np.broadcast_to(np.asarray(k), (T.shape[0],)) % 3
    r = np.arange(T.shape[0])[:, None]
    idx = (np.arange(3)[None, :] + k[:, None]) % 3
    for lo in (0, 9):
        T[:, lo:lo + 9] = T[:, lo:lo + 9].reshape(-1, 3, 3)[r, idx].reshape(-1, 9)
    return T


def resize(T, n):
    """n rows: T cut, or repeated with the repeats' vertices rotated so that a repeat is no copy"""
    T = np.ascontiguousarray(T, F)
    reps = -(-n // T.shape[0])
    out = np.concatenate([rotate_rows(T, i) for i in range(reps)])[:n]
    return np.ascontiguousarray(out)


def two_piece_rows(T):
    """the rows with their z made so that the plane z = 0 cuts every one of them in two pieces: vertex (row % 3) is strictly below, the
    other two strictly above.  Non-finite coordinates are replaced first."""
    T = np.array(T, F)
    V = np.nan_to_num(T[:, :9].reshape(-1, 3, 3), nan=1.5, posinf=3.0, neginf=-3.0)
    z = np.abs(V[:, :, 2]) + F(0.25)
    down = np.arange(T.shape[0]) % 3
    z[np.arange(T.shape[0]), down] *= F(-1)
    V[:, :, 2] = z
    T[:, :9] = V.reshape(-1, 9)
    return T

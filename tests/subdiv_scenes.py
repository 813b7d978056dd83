"""The scenes of the subdivision tests (tests/test_subdiv_expected.py on the CPU, tests/test_gpu_subdiv.py on the device) -- a helper,
no test.  numpy, and the builders of tests/topology_scenes.py, orient_scenes.py, weld_scenes.py, boundary_scenes.py and clip_scenes.py.

  tetra          topology_scenes: four triangles, every vertex of valence 3 (beta = 0.1875f) -- closed
  octa           an octahedron with vertices at +-2 on the axes: eight triangles, valence 4 -- closed
  cube_pow2      orient_scenes: 12 triangles with corners in {0, 4}^3, wound outwards -- closed; valences 4 and 5
  torus32        topology_scenes.torus(32): 2048 triangles with shuffled ids, valence 6 -- closed
  disc300        weld_scenes.disc(300): a cone of 300 triangles, an apex of valence 300 and a border ring
  strip_pow2     topology_scenes.strip(200) scaled by 0.5: border vertices only, all on two straight lines
  grid_pow2      the cells of boundary_scenes.grid_holes (an 8 x 8 grid with three cells missing) on the flat lattice (i / 4, j / 2, 0):
                 interior vertices of valence 6, straight borders and the corners of the holes -- every weight and sum is exact
  pinched        boundary_scenes: two fans that meet in one vertex (S7)
  book5          topology_scenes: five triangles on one spine (S7)
  moebius        topology_scenes: a band with FLIPPED edges
  signed_zero    topology_scenes: a shared edge stored with +0 and with -0
  dead           topology_scenes: NaN, infinities and degenerate triangles interleaved with live ones
  bunny          the small Bunny (scenes.mesh): open (four holes)

rows(name) are the triangles with a seeded random normal at every corner and a seeded random material in every row
(clip_scenes.decorate), so that S2 has something to average and a copied float is told from its neighbours.  pool() is every scene in
the order above -- small ones first, so that the smallest sizes still hold whole closed meshes -- each with its own rows shuffled;
sized(n) is the pool resized to n rows (clip_scenes.resize) with dead rows sprinkled in."""
import numpy as np

from ezrt_amd import scenes

import boundary_scenes as BS
import clip_scenes as CS
import orient_scenes as OS
import topology_scenes as TS
import weld_scenes as WS

F = np.float32
SEED = 3500
NAMES = ("tetra", "octa", "cube_pow2", "book5", "pinched", "signed_zero", "moebius", "grid_pow2", "disc300", "strip_pow2", "dead", "torus32",
         "bunny")
CLOSED = ("tetra", "octa", "cube_pow2", "torus32")
SD_TILE = 63                                                                   # the fill's tile (ezrt_subdiv_kernels.h)
SIZES = tuple(sorted({1, 63, 64, 65, 255, 256, 257, SD_TILE - 1, SD_TILE, SD_TILE + 1, 2049, 4097}))
GONE = {(3, 3), (3, 4), (5, 1)}
_cache = {}


def octa():
    px, nx, py, ny, pz, nz = F([2, 0, 0]), F([-2, 0, 0]), F([0, 2, 0]), F([0, -2, 0]), F([0, 0, 2]), F([0, 0, -2])
    return np.asarray([[px, py, pz], [py, nx, pz], [nx, ny, pz], [ny, px, pz], [py, px, nz], [nx, py, nz], [ny, nx, nz], [px, ny, nz]], F)


def grid_pow2():
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    P = np.stack([i / 4.0, j / 2.0, 0.0 * i], -1).astype(F)
    return BS._quads(P, [(a, b) for a in range(8) for b in range(8) if (a, b) not in GONE])


def _bunny():
    v, f = scenes.mesh("bunny")
    return np.ascontiguousarray(v[f], F)


_HAND = {"tetra": TS.tetra, "octa": octa, "cube_pow2": lambda: OS.cube(0, 4), "book5": TS.book5, "pinched": BS.pinched,
         "signed_zero": TS.signed_zero, "moebius": lambda: TS.moebius(20), "grid_pow2": grid_pow2, "disc300": lambda: WS.disc(300),
         "strip_pow2": lambda: TS.strip(200, shuffled=False) * F(0.5), "dead": TS.dead, "torus32": lambda: TS.torus(32), "bunny": _bunny}


def triangles(name):
    return np.ascontiguousarray(rows(name)[:, :9].reshape(-1, 3, 3))


def rows(name):
    """float32 [n, 36], built once and handed out read-only"""
    if name not in _cache:
        T = CS.decorate(np.ascontiguousarray(_HAND[name](), F), SEED + NAMES.index(name))
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def pool():
    if "pool" not in _cache:
        rng = np.random.default_rng(SEED + 21)
        parts = []
        for name in NAMES:
            T = rows(name)
            parts.append(T if name == "dead" else T[rng.permutation(T.shape[0])])
        T = np.ascontiguousarray(np.concatenate(parts))
        T.setflags(write=False)
        _cache["pool"] = T
    return _cache["pool"]


def sized(n):
    """n rows of the pool, with NaN, infinities and degenerate rows at any size above 2"""
    key = ("sized", n)
    if key not in _cache:
        R = CS.resize(pool(), n)
        dead = rows("dead")
        for j in range(min(n // 3, dead.shape[0])):
            R[(37 * j + 1) % n] = dead[j]
        R.setflags(write=False)
        _cache[key] = R
    return _cache[key]


def reverse_rows(T):
    """every row stored as (p1, p3, p2), with its normals"""
    T = np.array(T, F)
    for lo in (0, 9):
        T[:, lo:lo + 9] = T[:, lo:lo + 9].reshape(-1, 3, 3)[:, [0, 2, 1]].reshape(-1, 9)
    return T

"""The scenes of the boundary-loop tests (tests/test_boundary_expected.py on the CPU, tests/test_gpu_boundary.py on the device) -- a
helper, no test.  numpy, and the builders of tests/topology_scenes.py (TS), tests/orient_scenes.py (OS) and tests/weld_scenes.py (WS).

Each case is the smallest at which the kernels can still go wrong: several workgroups of 256, several scan tiles of 2048, a loop that
needs many jumping rounds, a long walk in one lane, chains that end at FLIPPED and NONMANIFOLD edges, no boundary at all.

  lone           one triangle: one loop of 3
  signed_zero    TS: two triangles joined across an edge stored with -0 and +0: one closed loop of 4
  islands        TS.islands(3000): 3000 closed loops of 3; 9000 half-edges, several scan tiles of 2048
  strip          TS.strip(6000), shuffled: one closed loop of 6002 across many workgroups, its head in the middle of the chain,
                 13 jumping rounds needed
  strip_rev      the strip with a seeded random 40 % of its triangles reversed: chains broken at FLIPPED edges into many open paths
  tube           a 64 x 64 quad cylinder open at both ends, shuffled: two closed loops of 64
  grid_holes     an 8 x 8 quad grid, integer coordinates with z = (i * j) % 3, the cells (3, 3), (3, 4) and (5, 1) removed, shuffled:
                 loops of 32, 4 and 6, all closed; the Stokes identity is exact
  bunny          the packaged Bunny (scenes.mesh("bunny"), 4968 triangles in the file's order): B = 42, four closed loops of 11, 12, 11
                 and 8
  pinched        two quarter-fans of 4 triangles that meet in the origin only: two closed loops of 6, each through the apex
  half_fan300    300 triangles round a border vertex: one walk of 299 rotation steps in one lane
  moebius        TS.moebius(20): two open paths of 20 (the band's one rim, broken where the stored windings disagree)
  book5          TS: five open paths of 2; NONMANIFOLD stops the walk
  dead           TS: triangles that do not take part; B = 10, two open paths
  torus, tetra   TS: B = 0, L = 0
  cube_open      OS.cube(0, 4) without its +z face: one loop of 4

rows(name) returns the rows [n, 36] read-only; scene(name) (tri [n, 36], nodes) as scene_create takes them, under the proxy tree of
topology_scenes.build (the boundary reads no tree); proxy_nodes(n) a tree for n rows, for the scene of a capped mesh."""
import numpy as np

from ezrt_amd import scenes

import orient_scenes as OS
import topology_scenes as TS
import weld_scenes as WS

F = np.float32
SEED = 3300
NAMES = ("lone", "signed_zero", "islands", "strip", "strip_rev", "tube", "grid_holes", "bunny", "pinched", "half_fan300", "moebius", "book5",
         "dead", "torus", "tetra", "cube_open")
# (B, the lengths of the loops in their order, closed loops), from include/ezrt_boundary.h by hand and by a numpy prototype
COUNTS = {"lone": (3, [3], 1), "signed_zero": (4, [4], 1), "islands": (9000, [3] * 3000, 3000), "strip": (6002, [6002], 1),
          "tube": (128, [64, 64], 2), "bunny": (42, [11, 12, 11, 8], 4), "pinched": (12, [6, 6], 2), "moebius": (40, [20, 20], 0),
          "book5": (10, [2] * 5, 0), "torus": (0, [], 0), "tetra": (0, [], 0), "cube_open": (4, [4], 1)}
SORTED_COUNTS = {"grid_holes": (42, [4, 6, 32], 3), "dead": (10, [2, 8], 0), "half_fan300": (302, [302], 1)}


def _shuffle(V, seed):
    return np.ascontiguousarray(V[np.random.default_rng(seed).permutation(V.shape[0])])


def _quads(P, cells):
    """two triangles (a, b, c), (a, c, d) per cell (i, j) of the vertex table P [ni, nj, 3], b = (i + 1, j), d = (i, j + 1); the first
    index wraps"""
    ni = P.shape[0]
    out = []
    for i, j in cells:
        a, b, c, d = P[i % ni, j], P[(i + 1) % ni, j], P[(i + 1) % ni, j + 1], P[i % ni, j + 1]
        out += [[a, b, c], [a, c, d]]
    return np.asarray(out, F)


def tube(n=64):
    th = 2 * np.pi * np.arange(n) / n
    P = np.stack([np.stack([np.cos(th), np.sin(th), np.full(n, z / 8.0)], 1) for z in range(n + 1)], 1).astype(F)   # [around, along, 3]
    return _shuffle(_quads(P, [(i, j) for i in range(n) for j in range(n)]), SEED + 1)


def grid_holes():
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    P = np.stack([i, j, (i * j) % 3], -1).astype(F)
    gone = {(3, 3), (3, 4), (5, 1)}
    # the shuffle decides the head of the rim, and the fan of C2 starts there: from (7, 0), (8, 1), (0, 7) or (1, 8) one of its edges
    # would run along the diagonal of a corner cell, an edge of four triangles then (the KNOWN LIMIT of C4); this seed's head is (8, 8)
    return _shuffle(_quads(P, [(a, b) for a in range(8) for b in range(8) if (a, b) not in gone]), SEED + 4)


def _fan(th, seed=None):
    ring = np.stack([np.cos(th), np.sin(th), 0 * th], 1).astype(F)
    V = np.stack([np.zeros((len(th) - 1, 3), F), ring[:-1], ring[1:]], 1)
    return V if seed is None else _shuffle(V, seed)


def pinched():
    return np.concatenate([_fan(np.linspace(0, np.pi / 2, 5)), _fan(np.linspace(np.pi, 3 * np.pi / 2, 5))])


def half_fan(k=300):
    return _fan(np.linspace(0, np.pi, k + 1), SEED + 3)


_HAND = {
    "lone": lambda: F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]), "signed_zero": TS.signed_zero, "islands": lambda: TS.islands(3000),
    "strip": lambda: TS.strip(6000), "strip_rev": lambda: OS.reverse(TS.strip(6000), OS.some(6000, 0.4, OS.SEED + 2)),
    "tube": tube, "grid_holes": grid_holes, "pinched": pinched, "half_fan300": half_fan, "moebius": lambda: TS.moebius(20),
    "book5": TS.book5, "dead": TS.dead, "torus": lambda: TS.torus(64), "tetra": TS.tetra, "cube_open": lambda: OS.cube(0, 4)[:10],
}
_cache = {}


def _bunny():
    v, f = scenes.mesh("bunny")
    return v[f]


_HAND["bunny"] = _bunny


def rows(name):
    """float32 [n, 36], built once and handed out read-only"""
    if name not in _cache:
        T = TS.tri36(np.ascontiguousarray(_HAND[name](), F))
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def triangles(name):
    return np.ascontiguousarray(rows(name)[:, :9].reshape(-1, 3, 3))


def proxy_nodes(n):
    return WS.proxy_nodes(n)


def scene(name):
    T = np.array(rows(name))
    return T, proxy_nodes(T.shape[0])

"""The scenes of the mesh-orientation tests (tests/test_orient_expected.py on the CPU, tests/test_gpu_orient.py on the device) -- a
helper, no test.  numpy, and the scene builders of tests/topology_scenes.py (TS) and tests/inside_scenes.py.

Each case is the smallest at which the kernels can still go wrong: several workgroups of 256, long chains of parents, many patches.

  tetra, tetra_flip   TS: the flipped tetrahedron comes out with exactly one flip
  moebius             TS.moebius(20): one patch, non-orientable and open
  klein               a Klein bottle as a 16 x 16 quad grid with the two identifications (one straight, one mirrored), 512 triangles
                      on a figure-8 immersion: closed and non-orientable
  torus, torus_rev    TS.torus(64), 8192 triangles with shuffled ids; _rev: a seeded random 40 % of the triangles reversed
  strip, strip_rev    TS.strip(6000): one patch of large diameter, the long-chain case of the union-find
  islands_rev         TS.islands(3000), random reversals: 3000 patches of one triangle
  book5               TS: five pages on one NONMANIFOLD spine, five patches of one component
  dup2, dup2_same     TS.dup(2), a face stored twice (opposite ways: MANIFOLD on all three edges) and the same face stored twice the
                      same way (FLIPPED on all three): one closed orientable patch of volume 0
  dead, signed_zero   TS: triangles that do not take part; -0 is +0 through the topology
  cube_pow2           a cube of 12 triangles with corners in {0, 4}^3, wound outwards; _shift: translated by (8, -16, 32);
                      _inside_out: every triangle reversed
  nested              cube_pow2 plus a smaller inside-out cube (corners in {1, 2}^3) inside it: two patches
  bunny_rev           the small Bunny with a seeded random 30 % of its triangles reversed; bunny_rev_not_nested: the same triangles
                      under another tree

triangles(name, bunny_small) returns the vertices [n, 3, 3]; scene(name, bunny_small) (tri [n, 36], nodes) as scene_create takes
them, under the proxy tree of topology_scenes.build (the orientation reads no tree) except for the Bunny's two; tree_scene(name,
bunny_small) the same triangles under the host builder's own tree, in the tree's order, for the tests that refit and trace."""
import numpy as np

import allhits_scenes as A
import inside_scenes as IS
import topology_scenes as TS

F = np.float32
SEED = 3200
NAMES = ("tetra", "tetra_flip", "moebius", "klein", "torus", "torus_rev", "strip", "strip_rev", "islands_rev", "book5", "dup2", "dup2_same",
         "dead", "signed_zero", "cube_pow2", "cube_pow2_shift", "cube_pow2_inside_out", "nested", "bunny_rev", "bunny_rev_not_nested")
BUNNY = ("bunny_rev", "bunny_rev_not_nested")


def reverse(V, which=None):
    """V [n, 3, 3] with the triangles `which` (bool [n], default all) stored as (p1, p3, p2)"""
    V = np.array(V, F)
    which = np.ones(V.shape[0], bool) if which is None else which
    V[which] = V[which][:, [0, 2, 1]]
    return V


def some(n, share, seed):
    """bool [n]: a seeded random `share` of n"""
    return np.random.default_rng(seed).random(n) < share


def reverse_rows(T, which):
    """rows [n, 36] with p2 <-> p3 and n2 <-> n3 exchanged in the rows `which`: the same surface, the other winding"""
    T = np.array(T, F)
    for lo in (3, 12):
        a, b = T[which, lo:lo + 3].copy(), T[which, lo + 3:lo + 6].copy()
        T[which, lo:lo + 3], T[which, lo + 3:lo + 6] = b, a
    return T


def klein(n=16):
    """the figure-8 immersion over an n x n grid: u closes straight, v closes mirrored ((u, v + 2 pi) is (-u, v)), so the vertices
    are taken from a table indexed modulo the identifications and shared on the bits"""
    v = 2 * np.pi * np.arange(n) / n
    u = 2 * np.pi * (np.arange(n) + 0.5) / n                                   # half a step off: no vertex on the curve where the surface crosses itself
    U, Vv = np.meshgrid(u, v, indexing="ij")
    r = 2.0
    c, s = np.cos(Vv / 2), np.sin(Vv / 2)
    w = r + c * np.sin(U) - s * np.sin(2 * U)
    P = np.stack([w * np.cos(Vv), w * np.sin(Vv), s * np.sin(U) + c * np.sin(2 * U)], -1).astype(F)

    def get(i, j):                                                             # i along u, j along v
        i = i % n
        return P[np.where(j >= n, n - 1 - i, i), j % n]                        # -u_i is u_(n - 1 - i)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = i.ravel(), j.ravel()
    a, b, cc, d = get(i, j), get(i + 1, j), get(i + 1, j + 1), get(i, j + 1)
    return np.stack([np.stack([a, b, cc], 1), np.stack([a, cc, d], 1)], 1).reshape(-1, 3, 3)


def cube(lo, hi):
    """12 triangles of the box [lo, hi]^3, wound outwards"""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], F)      # corner 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z, seen from outside
    out = []
    for a, b, cc, d in quads:
        out += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    return np.asarray(out, F)


def nested():
    return np.concatenate([cube(0, 4), reverse(cube(1, 2))])


def _bunny(bunny_small):
    T = np.ascontiguousarray(bunny_small.tri, F).reshape(-1, 36)
    return reverse_rows(T, some(T.shape[0], 0.3, SEED + 5))


_HAND = {
    "tetra": TS.tetra, "tetra_flip": TS.tetra_flip, "moebius": lambda: TS.moebius(20), "klein": klein,
    "torus": lambda: TS.torus(64), "torus_rev": lambda: reverse(TS.torus(64), some(8192, 0.4, SEED + 1)),
    "strip": lambda: TS.strip(6000), "strip_rev": lambda: reverse(TS.strip(6000), some(6000, 0.4, SEED + 2)),
    "islands_rev": lambda: reverse(TS.islands(3000), some(3000, 0.5, SEED + 3)),
    "book5": TS.book5, "dup2": lambda: TS.dup(2), "dup2_same": lambda: np.stack([TS.dup(1)[0], np.roll(TS.dup(1)[0], 1, axis=0)]),
    "dead": TS.dead, "signed_zero": TS.signed_zero,
    "cube_pow2": lambda: cube(0, 4), "cube_pow2_shift": lambda: cube(0, 4) + F([8, -16, 32]), "cube_pow2_inside_out": lambda: reverse(cube(0, 4)),
    "nested": nested,
}
_cache = {}


def rows(name, bunny_small=None):
    """float32 [n, 36], built once and handed out read-only"""
    if name not in _cache:
        T = _bunny(bunny_small) if name in BUNNY else TS.tri36(np.ascontiguousarray(_HAND[name](), F))
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def triangles(name, bunny_small=None):
    return np.ascontiguousarray(rows(name, bunny_small)[:, :9].reshape(-1, 3, 3))


_nodes = {}


def scene(name, bunny_small):
    T = np.array(rows(name, bunny_small))
    if name == "bunny_rev":
        return T, bunny_small.nodes
    if name == "bunny_rev_not_nested":
        return T, A.not_nested(bunny_small)[1]
    n = T.shape[0]
    if n not in _nodes:
        _nodes[n] = IS.build(TS.tri36(TS.islands(n)))[1]
    return T, _nodes[n]


def tree_scene(name, bunny_small):
    """(tri, nodes) under a tree that fits the triangles: what a refit and a trace need"""
    if name in BUNNY:
        return scene(name, bunny_small)
    tri, nodes = IS.build(np.array(rows(name)))
    return np.ascontiguousarray(tri, F).reshape(-1, 36), nodes

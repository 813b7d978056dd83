"""The scenes of the mesh-topology tests (tests/test_topology_expected.py on the CPU, tests/test_gpu_topology.py on the device) -- a
helper, no test.  numpy only, apart from the scene builders of tests/inside_scenes.py.

The fixtures of tests/winding_scenes.py (voxel_solid, open_solid, bunny, nasty, and not_nested on the device) plus hand-built scenes,
each a list of triangles [n, 3, 3] float32 whose vertices are shared BY VALUE:

  tetra          a tetrahedron, wound outwards: 6 MANIFOLD edges
  tetra_flip     ... with face 0 reversed: 3 FLIPPED and 3 MANIFOLD edges
  bowtie_edge    two tetrahedra sharing an edge by value: m = 4 on it, one component
  bowtie_vertex  two tetrahedra sharing one vertex: two components
  book5          five triangles on one edge, three one way and two the other: one twin is -1
  book4_same     four triangles on one edge, all the same way
  dup5, dup200   one face stored 5 and 200 times, vertex order rotated, some reversed
  signed_zero    a shared edge with a coordinate stored as +0 in one triangle and as -0 in the other: MANIFOLD
  dead           NaN, +inf, -inf, two and three equal vertices and one collinear sliver interleaved with live triangles: the sliver
                 takes part, the rest do not
  moebius        a Moebius band of 40 triangles: a FLIPPED edge whatever the windings
  torus          a 64 x 64 quad grid, 8192 triangles, closed, ids shuffled: 24 576 half-edges, 96 workgroups of 256
  strip          6000 triangles in a row, ids shuffled: one component of large diameter
  islands        3000 isolated triangles: C == n_tri

scene(name, bunny_small) returns (tri [n, 36], nodes) as scene_create takes them.  The topology reads no tree: the nodes of a
hand-built scene are the host builder's over as many well separated proxy triangles, and the triangle array keeps the order given
here (the scene is one whose tree does not fit its triangles, as open_solid's)."""
import numpy as np

import inside_scenes as IS
import winding_scenes as W

FIXTURES = W.CPU_NAMES
HAND = ("tetra", "tetra_flip", "bowtie_edge", "bowtie_vertex", "book5", "book4_same", "dup5", "dup200", "signed_zero", "dead", "moebius",
        "torus", "strip", "islands")
CPU_NAMES = FIXTURES + HAND
GPU_NAMES = W.GPU_NAMES + HAND
SEED = 2800
F = np.float32


def _tetra(v):
    v = np.asarray(v, F)
    return np.stack([v[[0, 2, 1]], v[[0, 1, 3]], v[[1, 2, 3]], v[[0, 3, 2]]])


_T0 = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]


def tetra():
    return _tetra(_T0)


def tetra_flip():
    V = tetra()
    V[0] = V[0, ::-1]
    return V


def bowtie_edge():
    return np.concatenate([_tetra(_T0), _tetra([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, -1]])])


def bowtie_vertex():
    return np.concatenate([_tetra(_T0), _tetra([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])])


def _book(ways):
    a, b = F([0, 0, 0]), F([0, 0, 1])
    out = []
    for i, fwd in enumerate(ways):
        th = 2 * np.pi * i / len(ways)
        p = F([np.cos(th), np.sin(th), 0.5])
        out.append([a, b, p] if fwd else [b, a, p])
    return np.asarray(out, F)


def book5():
    return _book([True, False, True, True, False])


def book4_same():
    return _book([True] * 4)


def dup(k):
    one = F([[0.25, -0.5, 1.0], [1.5, 0.75, -0.25], [-0.75, 1.25, 0.5]])
    out = []
    for i in range(k):
        t = np.roll(one, i % 3, axis=0)
        out.append(t[::-1] if i % 4 == 1 or i % 7 == 3 else t)
    return np.asarray(out, F)


def signed_zero():
    V = F([[[0.0, 0, 0], [1, 0.0, 0], [0, 1, 0]], [[1, -0.0, 0], [-0.0, 0, -0.0], [0, -1, 0]]])
    assert np.signbit(V[1, 0, 1]) and not np.signbit(V[0, 1, 1])
    return V


def dead():
    """live triangles (a fan around the origin) with the dead ones interleaved; the sliver is triangle 11"""
    fan = []
    for i in range(8):
        a, b = 2 * np.pi * i / 8, 2 * np.pi * (i + 1) / 8
        fan.append([[0, 0, 0], [np.cos(a), np.sin(a), 0], [np.cos(b) if i < 7 else 1.0, np.sin(b) if i < 7 else 0.0, 0]])
    fan = np.asarray(fan, F)
    fan[7, 2] = fan[0, 1]                                                      # closes on the bits
    p = F([[5, 5, 5], [6, 5, 5], [5, 6, 5]])
    bad = []
    for val, at in ((np.nan, (0, 0)), (np.inf, (1, 2)), (-np.inf, (2, 1)), (np.nan, (2, 2))):
        t = p.copy()
        t[at] = val
        bad.append(t)
    bad.append(F([[5, 5, 5], [5, 5, 5], [5, 6, 5]]))                           # two equal vertices
    bad.append(F([[5, 5, 5], [5, 6, 5], [5, 5, 5]]))
    bad.append(F([[0, 0, 0], [-0.0, 0, 0], [1, 0, 0]]))                        # ... equal by M1: -0 is +0
    bad.append(F([[5, 5, 5], [5, 5, 5], [5, 5, 5]]))                           # three
    sliver = F([[0, 0, 0], [0.5, 0, 0], [1, 0, 0]])                            # collinear, three distinct vertices: takes part
    order = [fan[0], bad[0], fan[1], bad[1], bad[2], fan[2], fan[3], bad[3], bad[4], fan[4], bad[5], sliver, fan[5], bad[6], fan[6],
             bad[7], fan[7]]
    return np.asarray(order, F)


DEAD_IDS = (1, 3, 4, 7, 8, 10, 13, 15)
SLIVER_ID = 11


def moebius(n=20):
    th = 2 * np.pi * np.arange(n) / n
    P = np.zeros((n, 2, 3), F)
    for side, s in enumerate((-0.3, 0.3)):
        r = 1 + s * np.cos(th / 2)
        P[:, side] = np.stack([r * np.cos(th), r * np.sin(th), s * np.sin(th / 2)], 1).astype(F)
    get = lambda i, side: P[i % n, side ^ ((i // n) % 2)]                       # the band closes with its sides swapped
    out = []
    for i in range(n):
        out.append([get(i, 0), get(i + 1, 0), get(i + 1, 1)])
        out.append([get(i, 0), get(i + 1, 1), get(i, 1)])
    return np.asarray(out, F)


def _shuffle(V, seed):
    return np.ascontiguousarray(V[np.random.default_rng(seed).permutation(V.shape[0])])


def torus(n=64, shuffled=True):
    u = 2 * np.pi * np.arange(n) / n
    U, Vv = np.meshgrid(u, u, indexing="ij")
    P = np.stack([(2 + 0.75 * np.cos(Vv)) * np.cos(U), (2 + 0.75 * np.cos(Vv)) * np.sin(U), 0.75 * np.sin(Vv)], -1).astype(F)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i, j = i.ravel(), j.ravel()
    a, b, c, d = P[i, j], P[(i + 1) % n, j], P[(i + 1) % n, (j + 1) % n], P[i, (j + 1) % n]
    V = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3, 3)
    return _shuffle(V, SEED + 1) if shuffled else V


def strip(n=6000, shuffled=True):
    k = np.arange(n // 2)
    z = np.zeros(n // 2)
    a, a1 = np.stack([k, z, z], 1).astype(F), np.stack([k + 1, z, z], 1).astype(F)
    b, b1 = np.stack([k, z + 1, z], 1).astype(F), np.stack([k + 1, z + 1, z], 1).astype(F)
    V = np.stack([np.stack([a, a1, b], 1), np.stack([a1, b1, b], 1)], 1).reshape(-1, 3, 3)
    return _shuffle(V, SEED + 2) if shuffled else V


def islands(n=3000):
    k = np.arange(n)
    o = np.stack([4 * (k % 50), 4 * (k // 50), 0 * k], 1).astype(F)
    return np.stack([o, o + F([1, 0, 0]), o + F([0, 1, 0.5])], 1)


_HAND = {"tetra": tetra, "tetra_flip": tetra_flip, "bowtie_edge": bowtie_edge, "bowtie_vertex": bowtie_vertex, "book5": book5,
         "book4_same": book4_same, "dup5": lambda: dup(5), "dup200": lambda: dup(200), "signed_zero": signed_zero, "dead": dead,
         "moebius": moebius, "torus": torus, "strip": strip, "islands": islands}
_cache = {}


def triangles(name, bunny_small=None):
    """float32 [n, 3, 3], built once and handed out read-only"""
    if name not in _cache:
        if name in _HAND:
            V = np.ascontiguousarray(_HAND[name](), F)
        else:
            V = np.ascontiguousarray(W.scene(name, bunny_small)[0][:, :9].reshape(-1, 3, 3), F)
        V.setflags(write=False)
        _cache[name] = V
    return _cache[name]


def tri36(V):
    """triangle rows [n, 36] of vertices V: one flat normal, one material (the topology reads neither)"""
    V = np.asarray(V, F).reshape(-1, 3, 3)
    T = IS.tri36(np.zeros_like(V) + F([[0, 0, 0], [1, 0, 0], [0, 1, 0]]))
    T[:, :9] = V.reshape(-1, 9)
    return T


def build(V):
    """(tri, nodes) of vertices V in THIS order, under a tree the topology never reads: the host builder's over as many well
    separated proxy triangles (a tree over V itself would be 200 levels deep for dup200, beyond what a scene accepts)"""
    T = tri36(V)
    _, nodes = IS.build(tri36(islands(T.shape[0])))
    return T, nodes


def scene(name, bunny_small):
    if name in _HAND:
        return build(triangles(name))
    return W.scene(name, bunny_small)

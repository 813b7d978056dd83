"""The scenes that the vertex-weld tests add to tests/topology_scenes.py (tests/test_weld_expected.py on the CPU,
tests/test_gpu_weld.py on the device) -- a helper, no test.  numpy and the host scene library only.

  disc300        300 triangles round one apex, ids shuffled: a star across several waves; its border vertices have valence 2
  two_discs      two such cones that share only the apex: fans 2 at valence 600
  quad_cube      the cube of the BASELINE scenes' floor box as its OBJ stores it: 24 vertex lines, 8 distinct values
  obj_bunny, obj_sphere, obj_sphere2
                 the rows readObj makes of the three smooth meshes of ezrt_amd/scenes.py, with the transforms used there, in the
                 OBJ's face order, WITH readObj's smooth normals in floats 9-17: the pin of N1 to N3

triangles(name) returns the vertices [n, 3, 3]; rows(name) the rows [n, 36] (readObj's for the OBJ scenes, flat normals for the
others); scene(name, bunny_small) (tri, nodes) as scene_create takes them, under the proxy tree of topology_scenes.build where the
order matters."""
import numpy as np

from ezrt_amd import scene as S
from ezrt_amd import scenes

import inside_scenes as IS
import topology_scenes as TS

F = np.float32
SEED = 2900
HAND = ("disc300", "two_discs")
OBJ = ("obj_bunny", "obj_sphere", "obj_sphere2")
NEW = HAND + ("quad_cube",) + OBJ
CPU_NAMES = TS.CPU_NAMES + NEW
GPU_NAMES = TS.GPU_NAMES + NEW


def disc(k=300, z=1.0, seed=SEED, shuffled=True):
    """a cone of k triangles (apex, ring[i], ring[i + 1]) round the apex at the origin, the ring closed on the bits"""
    th = 2 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(th), np.sin(th), np.full(k, z)], 1).astype(F)
    apex = np.zeros((k, 3), F)
    V = np.stack([apex, ring, np.roll(ring, -1, axis=0)], 1)
    return np.ascontiguousarray(V[np.random.default_rng(seed).permutation(k)]) if shuffled else V


def two_discs(k=300):
    V = np.concatenate([disc(k, 1.0, shuffled=False), disc(k, -1.0, shuffled=False)])
    return np.ascontiguousarray(V[np.random.default_rng(SEED + 1).permutation(2 * k)])


def sphere2_mesh():
    """sphere.obj subdivided three times and pushed back onto the sphere, as scenes.disney_grid_scene makes it"""
    sv, sf = scenes.subdivide(*scenes.mesh("sphere"), 3)
    c = sv.mean(axis=0, dtype=np.float32)
    r = np.sqrt(((sv[:162] - c) ** 2).sum(1)).mean(dtype=np.float32)
    dv = sv - c
    ln = np.sqrt((dv * dv).sum(1, dtype=np.float32)).astype(np.float32)
    return (c + dv * (r / ln)[:, None]).astype(np.float32), sf


# (vertices and faces, the transform of ezrt_amd/scenes.py)
_OBJ = {"obj_bunny": (lambda: scenes.mesh("bunny"), ((0, 0, 0), (0.3, -1.6, 0), (1.5, 1.5, 1.5))),
        "obj_sphere": (lambda: scenes.mesh("sphere"), ((0, 0, 0), (0.0, 0.9, -0.0), (1, 1, 1))),
        "obj_sphere2": (sphere2_mesh, ((0, 0, 0), (-2.4, -0.9, -2.4), (1.0, 1.0, 1.0))),
        "quad_cube": (lambda: scenes.mesh("quad"), ((0, 0, 0), (0, -1.4, 0), (18.83, 0.01, 18.83)))}
_cache = {}


def read_obj(name):
    """(rows float32 [n, 36] in the OBJ's face order with readObj's smooth normals, vertex lines, distinct vertex lines)"""
    mesh, trans = _OBJ[name]
    v, f = mesh()
    hs = S.HostScene()
    hs.readObjText(scenes.obj_text(v, f), S.Material.disney(baseColor=(1, 1, 1)), S.getTransformMatrix(*trans), True)
    tri, _ = hs.encode()
    tri = np.ascontiguousarray(tri, F).reshape(-1, 36)
    assert tri.shape[0] == f.shape[0]
    return tri, v.shape[0], np.unique(np.ascontiguousarray(v, F), axis=0).shape[0]


def rows(name):
    """float32 [n, 36], built once and handed out read-only"""
    if name not in _cache:
        if name in _OBJ:
            T = read_obj(name)[0]
        elif name == "disc300":
            T = TS.tri36(disc())
        else:
            T = TS.tri36(two_discs())
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def triangles(name, bunny_small=None):
    if name in NEW:
        return np.ascontiguousarray(rows(name)[:, :9].reshape(-1, 3, 3))
    return TS.triangles(name, bunny_small)


_nodes = {}


def proxy_nodes(n):
    """the tree of topology_scenes.build: the host builder's over n well separated proxy triangles, read by neither call"""
    if n not in _nodes:
        _nodes[n] = IS.build(TS.tri36(TS.islands(n)))[1]
    return _nodes[n]


def scene(name, bunny_small):
    if name in NEW:
        T = rows(name)
        return np.array(T), proxy_nodes(T.shape[0])
    return TS.scene(name, bunny_small)

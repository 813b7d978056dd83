"""The inputs of the decimation tests (tests/test_decimate_expected.py on the CPU, tests/test_gpu_decimate.py on the device) -- a
helper, no test.  numpy, the shipped meshes and the builders of tests/subdiv_scenes.py and tests/clip_scenes.py.

  shipped(name)  the rows of a shipped mesh (sphere 320, bunny 4968, sphere2 20480) in the file's order, decorated (seeded random corner
                 normals and materials, clip_scenes.decorate), so that a copied float is told from its neighbours
  sized(n)       subdiv_scenes.sized(n): n rows of every small scene there -- closed meshes, fans, strips, NaN, infinities, -0 and
                 degenerate rows -- and GRIDS, the divs under which the sizes are decimated (decimate_expected.grid_of)
  one_cell()     sphere2 under a grid so coarse that all 61440 corners share one cell
  edge(name)     (rows, grid4) for every name of EDGE_NAMES: the edge cases of D1, D2, D5 and D7, each small enough to read;
                 test_decimate_expected.py says what each must give

Every array is built once and handed out read-only."""
import numpy as np

from ezrt_amd import scenes

import clip_scenes as CS
import decimate_expected as DE
import subdiv_scenes as SS

F = np.float32
SEED = 3600
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)                       # wave, workgroup and fill tile, scan tile
GRIDS = (3, 256, 4096)                                                         # divs: a few cells, many, near one vertex value per cell
TABLE = (("sphere", 4, 112, 58, 208, 0), ("sphere", 8, 294, 149, 26, 0), ("sphere", 16, 320, 162, 0, 0), ("bunny", 8, 403, 200, 4540, 25),
         ("bunny", 16, 1446, 722, 3487, 35), ("bunny", 4096, 4968, 2503, 0, 0))   # mesh, div, rows out, cells, collapsed, duplicates
_cache = {}


def _once(key, make):
    if key not in _cache:
        x = make()
        for a in (x if isinstance(x, tuple) else (x,)):
            a.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def shipped(name):
    def make():
        v, f = scenes.mesh(name)
        return CS.decorate(np.ascontiguousarray(v[f], F), SEED + len(name))
    return _once(("shipped", name), make)


def sized(n):
    return SS.sized(n)


def grid(rows, div):
    return DE.grid_of(rows, div)


def one_cell():
    def make():
        R = shipped("sphere2")
        return R, F([-40.0, -40.0, -40.0, 100.0])
    return _once("one_cell", make)


def _rows(tris, seed):
    return CS.decorate(np.asarray(tris, F).reshape(-1, 3, 3), SEED + seed)


def _below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def _plate():
    """two faces of a plate 1/64 thick in a grid of unit cells: four quads of two triangles above, the same four below with the other
    winding; the two sheets share every cell, so every triangle below repeats the unordered triple of one above"""
    top, bottom = [], []
    for i in range(2):
        for j in range(2):
            a, b, c, d = (i + .5, j + .5), (i + 1.5, j + .5), (i + 1.5, j + 1.5), (i + .5, j + 1.5)
            for tri in ((a, b, c), (a, c, d)):
                top.append([(x, y, 0.515625) for x, y in tri])
                bottom.append([(x, y, 0.5) for x, y in tri[::-1]])
    return np.asarray(top + bottom, F)


def _flat():
    """an axis-aligned face: a 6 x 6 lattice of quads in the plane z = 0.3f, clustered four by four"""
    z = float(F(0.3))
    tris = []
    for i in range(6):
        for j in range(6):
            a, b, c, d = (i * .37, j * .41, z), ((i + 1) * .37, j * .41, z), ((i + 1) * .37, (j + 1) * .41, z), (i * .37, (j + 1) * .41, z)
            tris += [[a, b, c], [a, c, d]]
    return np.asarray(tris, F)


def _edge():
    big, far = 2.0 ** 20, 3.0e38
    E = {}
    # o and h powers of two; x = 0.5 is the face between cells 4 and 5 of the x axis, and belongs to 5
    E["on a face"] = (_rows([[(0.5, 0.3, 0.3), (_below(0.5), 0.3, 0.3), (0.3, 0.8, 0.3)],
                             [(0.5, 0.3, 0.3), (0.3, 0.8, 0.3), (0.5, 0.8, 0.8)]], 1), F([-2, -2, -2, 0.5]))
    # cells -1 and -2: -1.0 is on the face and belongs to -1
    E["negative"] = (_rows([[(-0.5, -0.5, -0.5), (-1.0, -1.5, -0.25), (_below(-1.0), -0.5, -2.5)],
                            [(-3.25, -0.5, -0.5), (-1.0, -1.5, -0.25), (-0.75, -2.5, -3.5)]], 2), F([0, 0, 0, 1]))
    # -0 lies in cell 0 and comes out as +0 (D5), alone in its cell or not
    E["minus zero"] = (_rows([[(-0.0, -0.0, -0.0), (1.5, -0.0, 0.5), (0.5, 1.5, -0.0)],
                              [(0.0, 0.0, -0.0), (-1.5, -0.0, 0.5), (-0.0, -1.5, 2.5)]], 3), F([0, 0, 0, 1]))
    # the last index that is in, 2^20 - 1 and -2^20, and the first that is out, on both sides
    E["index limits"] = (_rows([[(big - 0.5, 0, 0), (0, big - 0.5, 0), (0, 0, big - 0.5)], [(big, 0, 0), (0, 1, 0), (0, 0, 1)],
                                [(-big, 0, 0), (0, -big, 0), (0, 0, -big)], [(-big - 0.5, 0, 0), (0, 1, 0), (0, 0, 1)],
                                [(0, 0, 0), (0, 5, big), (7, 0, 0)]], 4), F([0, 0, 0, 1]))
    # u overflows to infinity: the row takes no part; its neighbour does
    E["u overflows"] = (_rows([[(far, 0, 0), (0, 1e-30, 0), (0, 0, 1e-30)], [(3e-30, 0, 0), (0, 1e-30, 0), (0, 0, 2e-30)]], 5), F([0, 0, 0, 1e-30]))
    # h denormal: a coordinate takes part within 2^20 denormal steps of the origin; 1.0 is out of range
    E["h denormal"] = (_rows([[(0, 0, 0), (0, 0, 0), (0, 0, 0)], [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 0), (1e-40, 0, 0), (0, 0, 0)]], 6),
                       F([0, 0, 0, 1e-45]))
    sphere = shipped("sphere")
    for name, g in (("h zero", [0, 0, 0, 0]), ("h minus zero", [0, 0, 0, -0.0]), ("h negative", [0, 0, 0, -1]), ("h NaN", [0, 0, 0, np.nan]),
                    ("h infinite", [0, 0, 0, np.inf]), ("origin NaN", [0, np.nan, 0, 1]), ("origin infinite", [-np.inf, 0, 0, 1])):
        E[name] = (sphere[:70], F(g))
    E["NaN and Inf rows"] = (np.concatenate([SS.rows("dead"), sphere[:5]]), F([-3, -3, -3, 0.75]))
    E["one cell"] = (sphere, F([-8, -8, -8, 16]))
    E["thin plate"] = (_rows(_plate(), 7), F([0, 0, 0, 1]))
    E["flat face"] = (_rows(_flat(), 8), F([-0.1, -0.1, -0.1, 0.8]))
    return E


EDGE_NAMES = ("on a face", "negative", "minus zero", "index limits", "u overflows", "h denormal", "h zero", "h minus zero", "h negative", "h NaN",
              "h infinite", "origin NaN", "origin infinite", "NaN and Inf rows", "one cell", "thin plate", "flat face")


def edge(name):
    """(rows [n, 36], grid4 [4]) of an edge case"""
    if "edge" not in _cache:
        E = _edge()
        assert tuple(E) == EDGE_NAMES
        for R, g in E.values():
            R.setflags(write=False), g.setflags(write=False)
        _cache["edge"] = E
    return _cache["edge"][name]

"""The fields of the isosurface tests (tests/test_iso_expected.py, tests/test_gpu_iso.py) -- a helper, no test.  numpy only.

Every function returns (values float32 [nz, ny, nx], grid8 float32 [8]) and is deterministic; the arrays are handed out read-only."""
import functools

import numpy as np

import iso_expected as IE

F = np.float32
SEED = 3901
# (nx, ny, nz) of the header's small grids: one cell; less than a wave; exactly two blocks; blocks ending mid-row; an x-row longer than
# a wave; one cell per x-row
DIMS = ((2, 2, 2), (5, 4, 3), (17, 9, 5), (19, 7, 6), (67, 5, 3), (2, 9, 40))
NO_CELLS = ((1, 5, 5), (5, 5, 1), (5, 1, 5), (1, 1, 1))


def _ro(V, g):
    V = np.ascontiguousarray(V, F)
    g = np.ascontiguousarray(g, F)
    V.flags.writeable = False
    g.flags.writeable = False
    return V, g


def _xyz(n):
    nz, ny, nx = (n, n, n) if np.ndim(n) == 0 else n
    return np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")


@functools.lru_cache(None)
def sphere(n=17):
    """a sphere with an off-lattice centre well inside the grid, in units of the grid; the grid is [-1, 1]^3"""
    z, y, x = _xyz(n)
    c = (n - 1) / 2.0
    V = np.sqrt((x - c - 0.13) ** 2 + (y - c + 0.09) ** 2 + (z - c - 0.27) ** 2) - 0.33 * (n - 1)
    return _ro(V, IE.grid8((-1, -1, -1), 2.0 / (n - 1), 0.0))


@functools.lru_cache(None)
def torus(n=17):
    z, y, x = _xyz(n)
    c = (n - 1) / 2.0
    R, r = 0.3125 * (n - 1), 0.131 * (n - 1)
    V = np.sqrt((np.sqrt((x - c - 0.13) ** 2 + (y - c + 0.09) ** 2) - R) ** 2 + (z - c - 0.27) ** 2) - r
    return _ro(V, IE.grid8((0.5, -0.25, 3.0), (0.125, 0.25, 0.0625), 0.0))


@functools.lru_cache(None)
def noise(dims=(17, 17, 17), padded=True, seed=0):
    """Gaussian noise, dense in rows; padded: one layer of outside values all round, so that the surface is closed"""
    nx, ny, nz = dims
    V = np.random.default_rng(SEED + seed).standard_normal((nz, ny, nx))
    if padded:
        V[0], V[-1], V[:, 0], V[:, -1], V[:, :, 0], V[:, :, -1] = 3.0, 3.0, 3.0, 3.0, 3.0, 3.0
    return _ro(V, IE.grid8((0.1, -0.3, 2.7), (0.37, 0.11, 1.3), 0.05))


@functools.lru_cache(None)
def at_level(n=19):
    """an integer field with hundreds of grid values exactly at the level: |x| + |y| + |z| about the middle vertex, level 8"""
    z, y, x = _xyz(n)
    c = (n - 1) // 2
    V = np.abs(x - c) + np.abs(y - c) + np.abs(z - c)
    assert int((V == 8).sum()) > 200
    return _ro(V, IE.grid8((0, 0, 0), 1.0, 8.0))


@functools.lru_cache(None)
def patterns():
    """all 256 corner-sign patterns of a cell: pattern p sits in the cell at (3 (p % 16), 3 (p / 16), 0) of a 48 x 48 x 2 grid, with values
    of random size on both sides of the level 0.25"""
    rng = np.random.default_rng(SEED + 1)
    V = 0.25 + rng.uniform(0.05, 2.0, (2, 48, 48))
    for p in range(256):
        a, b = 3 * (p % 16), 3 * (p // 16)
        for c in range(8):
            if p >> c & 1:
                dx, dy, dz = c & 1, c >> 1 & 1, c >> 2
                V[dz, b + dy, a + dx] = 0.25 - rng.uniform(0.05, 2.0)
    return _ro(V, IE.grid8((-3, 2, 0.5), (0.25, 0.5, 2.0), 0.25))


@functools.lru_cache(None)
def sparse_large():
    """more than 2048 blocks' worth of cells (129 x 65 x 65 = 545025 cells, 2130 blocks) with a small sphere: the scan's second tile, and
    most blocks are skipped by the fill; the sphere lies in the high blocks so that rows are offset by the second tile's sum too"""
    nz, ny, nx = 66, 66, 130
    z, y, x = _xyz((nz, ny, nx))
    V = np.minimum(np.sqrt((x - 40.3) ** 2 + (y - 30.7) ** 2 + (z - 20.1) ** 2) - 6.4, np.sqrt((x - 100.6) ** 2 + (y - 33.2) ** 2 + (z - 62.0) ** 2) - 2.7)
    return _ro(V, IE.grid8((0, 0, 0), (0.5, 0.5, 0.5), 0.0))


@functools.lru_cache(None)
def special():
    """values at the level, -0 against a level of +0, NaN and both infinities"""
    rng = np.random.default_rng(SEED + 2)
    V = rng.standard_normal((6, 7, 9)).astype(F)
    V[rng.random(V.shape) < 0.15] = 0.0
    V[rng.random(V.shape) < 0.1] = -0.0
    V[2, 3, 4], V[4, 1, 7], V[1, 5, 2], V[5, 6, 8] = np.nan, np.inf, -np.inf, np.nan
    return _ro(V, IE.grid8((1e3, -1e3, 0), (1e-3, 3.0, 0.7), 0.0))


def not_live():
    """(name, grid8) of each way for a grid not to be live"""
    base = IE.grid8((0.5, 1, 2), (0.5, 0.25, 1.0), 0.1)
    out = []
    for name, at, v in (("nan origin", 1, np.nan), ("inf origin", 0, np.inf), ("zero spacing", 3, 0.0), ("minus zero spacing", 4, -0.0),
                        ("negative spacing", 5, -1.0), ("inf spacing", 4, np.inf), ("nan spacing", 3, np.nan), ("nan level", 6, np.nan),
                        ("inf level", 6, np.inf), ("minus inf level", 6, -np.inf)):
        g = base.copy()
        g[at] = v
        out.append((name, g))
    return out


MATERIAL = np.arange(1, 19, dtype=np.float64).astype(F) * F(0.25)

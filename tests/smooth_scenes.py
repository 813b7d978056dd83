"""The scenes of the smoothing tests (tests/test_smooth_expected.py on the CPU, tests/test_gpu_smooth.py on the device) -- a helper,
no test.  numpy; the pool, rows(name), sized(n) and reverse_rows of tests/subdiv_scenes.py, and the sampled spheres of
tests/iso_scenes.py through the restated isosurface of tests/iso_expected.py.

  SIZES          the row counts of the device tests: wave, workgroup and fill tile (64 rows), more than one workgroup; the tests add the
                 three sizes around the library's tile_rows_max
  STEPS          the step counts with Taubin's pair
  iso_sphere(n)  the rows of iso_scenes.sphere(n) through iso_expected.iso: marching tetrahedra's slivers on a closed surface"""
import numpy as np

import iso_expected as IE
import iso_scenes as IS
import subdiv_scenes as SS

F = np.float32
SEED = 4100
NAMES = SS.NAMES
CLOSED = SS.CLOSED
SIZES = (1, 63, 64, 65, 255, 256, 257, 2049, 4097)
STEPS = (1, 2, 3, 7)
TAUBIN = (0.5, -0.53)
rows, sized, reverse_rows = SS.rows, SS.sized, SS.reverse_rows
_cache = {}


def iso_sphere(n):
    """(values float32 [n, n, n], grid8, rows float32 [m, 36]) of the sampled sphere (level 0, origin (-1, -1, -1), spacing 2 / (n - 1)),
    built once and handed out read-only"""
    if n not in _cache:
        V, g = IS.sphere(n)
        out = np.ascontiguousarray(IE.iso(V, g).out, F)
        out.setflags(write=False)
        _cache[n] = (V, g, out)
    return _cache[n]

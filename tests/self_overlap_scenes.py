"""The defect scene of the self-overlap tests (tests/test_self_overlap_expected.py on the CPU, tests/test_gpu_self_overlap.py on the
device; a helper, no test): the voxel solid of tests/inside_scenes.py, which crosses itself nowhere, with constructed defects whose
coordinates are multiples of 1/4 -- exactly representable, and inside the range where the rule of include/ezrt_self_overlap.h is
exact:

  COPY     a second copy of the solid translated by (0.5, 0.5, 0.5): its faces cut the faces of the first          (s = 0)
  TWIN     triangle 0 again, its vertices rotated: a duplicated face                                               (s = 3)
  FOLD     two coplanar triangles on one side of the edge they share, and beside them a proper dihedral (s = 2)
  FAN      two triangles that share a vertex and pierce each other along a segment from it                       (s = 1)
  BLADES   two large triangles that share a vertex, in the planes z = 3.25 and y = 3.25: they cross each other along the line
           from that vertex, and each cuts through both copies of the solid -- rows of more than 64 ids          (s = 1, s = 0)

moved_clear() is the same scene with the copy moved away by (0, 0, 16): what a refit is given."""
import numpy as np

import inside_scenes as IS

SHIFT = np.float32([0.5, 0.5, 0.5])
CLEAR = np.float32([0, 0, 16])

_scene = None


def _defects():
    fold = [[[20, 0, 0], [24, 0, 0], [22, 4, 0]], [[24, 0, 0], [21, 2, 0], [20, 0, 0]],       # folded onto each other
            [[20, 8, 0], [24, 8, 0], [22, 12, 0]], [[24, 8, 0], [20, 8, 0], [22, 10, 3]]]     # a dihedral: nothing
    fan = [[[30, 0, 0], [34, -2, 0], [34, 2, 0]], [[33, 0, -2], [30, 0, 0], [33, 0, 2]]]
    blades = [[[-4, 3.25, 3.25], [12, -6, 3.25], [12, 12.5, 3.25]], [[12, 3.25, 12.5], [-4, 3.25, 3.25], [12, 3.25, -6]]]
    return np.float32(fold + fan + blades)


def defect_scene():
    """dict: P float32 [n, 3, 3], tri [n, 36] and nodes as scene_create takes them (in the builder's order: P is tri's vertices),
    plain and copy bool [n] (the triangles of the solid and of its translated copy), m (the triangles of one solid) -- built once"""
    global _scene
    if _scene is None:
        base = IS.boundary_triangles(IS.occupancy())
        m = base.shape[0]
        P = np.concatenate([base, base + SHIFT, np.roll(base[:1], 1, axis=1), _defects()]).astype(np.float32)
        assert np.array_equal(P * 4, np.round(P * 4))
        T = IS.tri36(P)
        T[:, 21] = 0.75                                               # a material number marks the parts through the builder's reordering
        T[m:2 * m, 21] = 0.25
        T[2 * m:, 21] = 0.5
        tri, nodes = IS.build(T)
        copy, plain = tri[:, 21] == np.float32(0.25), tri[:, 21] == np.float32(0.75)
        assert copy.sum() == m and plain.sum() == m
        _scene = dict(P=np.ascontiguousarray(tri[:, :9].reshape(-1, 3, 3)), tri=tri, nodes=nodes, copy=copy, plain=plain, m=m)
    return _scene


def moved_clear():
    """float32 [n, 36]: the defect scene's triangle array with the copy translated by CLEAR"""
    s = defect_scene()
    tri = s["tri"].copy()
    for k in range(3):
        tri[s["copy"], 3 * k:3 * k + 3] += CLEAR
    return tri

"""The scenes and query points of the winding-number tests (tests/test_winding_expected.py on the CPU, tests/test_gpu_winding.py on
the device, tools/winding_host_check.py) -- a helper, no test.

Scenes: the voxel solid of tests/inside_scenes.py (closed, integer coordinates); `open_solid`, the same with every fifth face
removed; the small Bunny (open: it has holes); "nasty" of tests/allhits_scenes.py (slivers, a coplanar grid, duplicates, a far
cluster: no solid at all); `not_nested`, the Bunny's triangles under a tree that does not prune.
Points: tests/closest_point_expected.py's points_for (uniform in the inflated box, exactly on the surface, just off vertices, on box
planes of the tree, far away, non-finite) thinned, plus tests/inside_scenes.py's surface_points (exactly on vertices, edge midpoints
and box planes)."""
import numpy as np

import allhits_scenes as A
import closest_point_expected as E
import inside_scenes as IS

CPU_NAMES = ("voxel_solid", "open_solid", "bunny", "nasty")
GPU_NAMES = CPU_NAMES + ("not_nested",)
SEED = 2300


def open_solid():
    """the voxel solid with every fifth face (two triangles) removed: an open mesh with many holes; the solid's tree is kept (its
    leaf ranges then point past the shortened array's faces: the winding queries read no tree)"""
    v = IS.voxel_solid()
    keep = (np.arange(v["tri"].shape[0]) // 2) % 5 != 0
    tri = np.ascontiguousarray(v["tri"][keep])
    return IS.build(tri)


def scene(name, bunny_small):
    """(tri [m, 36], nodes) as scene_create takes them"""
    if name == "voxel_solid":
        v = IS.voxel_solid()
        return v["tri"], v["nodes"]
    if name == "open_solid":
        return open_solid()
    tri, nodes, _ = A.scene(name, bunny_small)
    return tri, nodes


def inputs(name, bunny_small, thin=2):
    """(tri, nodes, points float32 [n, 3]): every kind of point, the non-finite ones included"""
    tri, nodes = scene(name, bunny_small)
    seed = SEED + GPU_NAMES.index(name)
    base, _ = E.points_for(tri, nodes, seed)
    base = base[::thin]
    pts = np.concatenate([base, IS.surface_points(tri, nodes, seed, base.shape[0] // 3)])
    return tri, nodes, np.ascontiguousarray(pts, np.float32)

"""The yardstick of the inside tests pinned before the device is compared with it, and the parts of the binding that need no device
(include/ezrt_inside.h, ezrt_amd/query.py: inside, signed_distance).

tests/inside_expected.py restates the header's crossing rule in numpy over all triangles.  Here it is held against a truth that owes
nothing to it: the occupancy grid of tests/inside_scenes.py's voxel solid, at voxel centres and at points whose axis rays run exactly
through mesh edges and vertices -- for all six axes, 100 %.  Then the invariances the header promises (triangle order, winding,
vertex order, a doubled mesh), the triangles that never count, and the binding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_expected as IE  # noqa: E402
import inside_scenes as IS  # noqa: E402


@pytest.fixture(scope="module")
def solid():
    v = IS.voxel_solid()
    if "want" not in v:
        v["want"] = IE.all_axes(v["points"], v["tri"])               # computed once, shared, never changed
    return v


def test_the_scene_meets_its_conditions(solid):
    tri, kept, truth, kind = solid["tri"], solid["kept"], solid["truth"], solid["kind"]
    assert 200 <= tri.shape[0] <= 1000                                           # a few hundred
    P = tri[:, :9]
    assert np.array_equal(P, np.round(P)) and P.min() >= 0 and P.max() <= IS.G   # small integers
    assert kept[kind == 0].all() and (kind == 0).sum() == IS.G ** 3              # no voxel centre is left out
    on_grid = kept & (kind > 0)
    assert on_grid.sum() >= 200 and (on_grid & truth).sum() >= 50
    assert (kept & (kind == 1) & truth).any() and (kept & (kind == 2) & truth).any()
    assert (~kept).any()                                                         # some points do lie on the surface
    # closed, and every edge shared by an even number of triangles (4 along the concave touching edges, else 2)
    V = P.reshape(-1, 3, 3)
    edges = {}
    for t in V:
        for e in range(3):
            key = tuple(sorted((tuple(t[e]), tuple(t[(e + 1) % 3]))))
            edges[key] = edges.get(key, 0) + 1
    assert all(c % 2 == 0 for c in edges.values())
    occ = solid["occ"]
    assert occ.sum() > 50 and not occ[IS.G // 2, IS.G // 2].any()                # the tunnel


def test_equals_the_occupancy_truth_on_every_axis(solid):
    cr, ins = solid["want"]
    kept, truth = solid["kept"], solid["truth"]
    for axis in range(6):
        wrong = (ins[axis] != truth)[kept]
        assert not wrong.any(), "axis %d: %d of %d points differ from the occupancy grid" % (axis, int(wrong.sum()), int(kept.sum()))
    assert all(np.array_equal(ins[0][kept], ins[axis][kept]) for axis in range(1, 6))   # the six axes agree
    assert cr[:, kept].max() >= 3                                                # rays that enter, leave and enter again (the tunnel)


def test_order_winding_and_vertex_order_do_not_matter(solid):
    tri, pts = solid["tri"], solid["points"]
    cr, ins = solid["want"]
    rng = np.random.default_rng(7)
    P = tri[:, :9].reshape(-1, 3, 3)
    shuffled = P[rng.permutation(P.shape[0])]
    reversed_ = P[:, ::-1]
    rolled = np.stack([np.roll(t, int(r), axis=0) for t, r in zip(P, rng.integers(0, 3, P.shape[0]))])
    mixed = np.stack([t[rng.permutation(3)] for t in P])
    for what, Q in (("shuffled", shuffled), ("reversed", reversed_), ("rolled", rolled), ("mixed", mixed)):
        got = IE.all_axes(pts, Q)
        assert np.array_equal(got[0], cr) and np.array_equal(got[1], ins), what
    # ... and on a mesh that is not on a grid: random rotations make every predicate round
    ang = 0.37
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.6), -np.sin(0.6)], [0, np.sin(0.6), np.cos(0.6)]])
    Q = (P.astype(np.float64) @ R.T).astype(np.float32)
    q = (pts.astype(np.float64) @ R.T).astype(np.float32)
    base = IE.all_axes(q, Q)
    for Q2 in (Q[rng.permutation(Q.shape[0])], Q[:, ::-1], np.stack([t[rng.permutation(3)] for t in Q])):
        got = IE.all_axes(q, Q2)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    centres = solid["kind"] == 0                                                 # well off the surface: the truth again
    assert all(np.array_equal(base[1][axis][centres], solid["truth"][centres]) for axis in range(6))


def test_a_doubled_mesh_doubles_the_crossings(solid):
    tri, pts = solid["tri"], solid["points"]
    cr, ins = solid["want"]
    got = IE.all_axes(pts, np.concatenate([tri, tri]))
    assert np.array_equal(got[0], 2 * cr) and not got[1].any()


def test_triangles_that_never_count():
    pts = np.float32([[0.25, 0.25, -1.0], [0.25, 0.25, 1.0], [0.0, 0.0, -1.0], [2.0, 2.0, -1.0], [np.nan, 0.25, -1.0], [0.25, np.inf, -1.0]])
    one = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    cr = IE.crossings(pts, one, 4)[0]                                           # +z
    assert cr.tolist() == [1, 0, 1, 0, 0, 0]                                    # ahead; behind; under the lowest vertex; off; non-finite p
    assert IE.crossings(pts, one, 5)[0].tolist() == [0, 1, 0, 0, 0, 0]          # -z
    assert not IE.crossings(pts, one, 0)[0].any() and not IE.crossings(pts, one, 3)[0].any()   # edge-on along x and y
    on = np.float32([[0.25, 0.25, 0.0]])                                        # exactly on the triangle: not ahead of itself
    assert IE.crossings(on, one, 4)[0][0] == 0 and IE.crossings(on, one, 5)[0][0] == 0
    edge_on = np.float32([[[0, 0, 0], [1, 5, 0], [1, 9, 0]]])                   # in the plane z = 0: the rays along y run inside it
    for axis in (2, 3):
        assert not IE.crossings(np.float32([[0.5, -1.0, 0.0], [0.5, 12.0, 0.0], [1.0, -1.0, 0.0]]), edge_on, axis)[0].any()
    for bad in (np.nan, np.inf, -np.inf):
        for v in range(3):
            for c in range(3):
                t = one.copy()
                t[0, v, c] = bad
                for axis in range(6):
                    assert not IE.crossings(pts, t, axis)[0].any(), (bad, v, c, axis)
    # beside a good triangle the bad ones change nothing
    both = np.concatenate([one, np.float32([[[0, 0, 0.5], [np.nan, 0, 0.5], [0, 1, 0.5]]]), one[:, [0, 0, 1]]])
    assert IE.crossings(pts, both, 4)[0].tolist() == cr.tolist()


def test_two_triangles_share_an_edge_and_a_fan_shares_a_vertex():
    # a square of two triangles, held with the shared edge either way round: a point of the diagonal's projection crosses once
    a, b, c, d = [0, 0, 0], [4, 0, 1], [4, 4, 2], [0, 4, 3]
    pts = np.float32([[1, 1, -5], [2, 2, -5], [3, 3, -5], [0, 0, -5], [4, 4, -5], [0, 2, -5], [2, 0, -5], [4, 2, -5], [2, 4, -5]])
    for t1 in ([a, b, c], [c, a, b], [b, a, c]):
        for t2 in ([a, c, d], [c, a, d], [d, c, a]):
            cr = IE.crossings(pts, np.float32([t1, t2]), 4)[0]
            assert cr[:3].tolist() == [1, 1, 1] and (cr <= 1).all()
    # a fan of 8 triangles around (0, 0): the ray through the hub crosses exactly one, as does a ray through a spoke
    ang = np.arange(8) * np.pi / 4
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.arange(8)], 1).round(3)
    fan = np.float32([[[0, 0, 1], rim[i], rim[(i + 1) % 8]] for i in range(8)])
    q = np.float32([[0, 0, -1]] + [[0.5 * rim[i, 0], 0.5 * rim[i, 1], -1] for i in range(8)])
    assert IE.crossings(q[:1], fan, 4)[0].tolist() == [1]
    spokes = IE.crossings(q[1:], fan, 4)[0]                                     # (half a rim vertex lies on its spoke exactly)
    assert spokes.tolist() == [1] * 8


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi, query
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ezrt_inside.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.INSIDE_ABI) == ["ezrt_query_inside_device", "ezrt_query_signed_distance_device"]
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.INSIDE_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "NEAREST_ABI", "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other
    assert callable(query.inside) and callable(query.signed_distance)
    assert query.SignedDistance._fields == ("tri", "point", "dist", "bary", "inside")


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    pts = torch.zeros((4, 3), dtype=torch.float32)
    for axis in (6, -1, 1.0, True, None, "x"):
        with pytest.raises(ValueError, match="axis must be an int"):
            query.inside(None, pts, axis)
        with pytest.raises(ValueError, match="axis must be an int"):
            query.signed_distance(None, pts, axis=axis)
    for f in (query.inside, query.signed_distance):
        with pytest.raises(TypeError, match="GPU tensor"):
            f(None, pts)
        with pytest.raises(TypeError, match="GPU tensor"):
            f(None, np.zeros((4, 3), np.float32))

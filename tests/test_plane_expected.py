"""tests/plane_expected.py -- the numpy restatement of include/ezrt_plane.h that the GPU test and the host check compare with on the
bits -- held against exact rational arithmetic and against the header's own claims.  Needs no GPU and no library.

* Against the truth: `fractions` on the voxel solid (integer coordinates) with axis and skew planes of integer and half-integer
  coefficients: the classification is THE exact one, q0 and q1 lie on the edges the exact walk names, and every end point is within
  the header's DERIVED bound  2^-24 |P*| + 2^-49 max(|A|, |B|)  of the exact rational point P*.
* The loop guarantee (every bit pattern as often a q0 as a q1) on the closed solid for random, axis and skew planes; the
  orientation (signed area +8.0 of the section z = 1.5 about the plane's normal, for both signs of the plane); zero-length segments.
* On the bits: vertex orders (three keep, three swap q0 and q1), the order of the triangles, `part` of every slicing.
* The edge cases of P3: a triangle in the plane, touching from either side, the negated plane, degenerate and non-finite triangles,
  planes that are not live, huge finite values."""
import itertools
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import plane_expected as PE  # noqa: E402
import plane_scenes as PS  # noqa: E402

F = np.float32


def _solid():
    return IS.voxel_solid()["tri"]


def _grid_planes():
    """integer and half-integer planes on the voxel solid's grid: axis planes (both signs) and skew ones"""
    rows = []
    for axis in range(3):
        for d in (1, 1.5, 2, 3, 3.5, 5.5, 6):
            for sign in (1, -1):
                r = [0, 0, 0, sign * d]
                r[axis] = sign
                rows.append(r)
    for nrm in ((1, 2, 3), (2, -1, 1), (-3, 1, 0.5), (1, 1, 1), (0.5, -2.5, 1.5), (7, 5, -3)):
        for d in (0, 3.5, 10, 10.5, -2, 21):
            rows.append(list(nrm) + [d])
    return np.asarray(rows, F)


def test_against_exact_rational_arithmetic():
    tri = _solid()
    V = PE.vertices(tri)
    planes = _grid_planes()
    offsets, ids, seg, cr = PE.section(planes, tri)
    VF = [[[Fraction(float(x)) for x in v] for v in t] for t in V]
    worst, n_inexact, n_zero = 0.0, 0, 0
    for i, pl in enumerate(planes):
        a, b, c, d = (Fraction(float(x)) for x in pl)
        rows = {int(k): seg[r] for r, k in zip(range(offsets[i], offsets[i + 1]), ids[offsets[i]:offsets[i + 1]])}
        for k, t in enumerate(VF):
            s = [a * v[0] + b * v[1] + c * v[2] - d for v in t]
            up = [x >= 0 for x in s]
            exact_crossed = any(up) and not all(up)
            assert exact_crossed == bool(cr[i, k]) == (k in rows), (i, k)
            if not exact_crossed:
                continue
            for e in range(3):                                           # the walk p1 -> p2 -> p3 -> p1
                f = (e + 1) % 3
                if up[e] == up[f]:
                    continue
                q = 0 if up[e] else 1                                    # UP -> DOWN is q0
                tt = s[e] / (s[e] - s[f])
                exact = [t[e][x] + tt * (t[f][x] - t[e][x]) for x in range(3)]
                for x in range(3):
                    got = Fraction(float(rows[k][q][x]))
                    M = max(abs(t[e][x]), abs(t[f][x]))
                    bound = Fraction(1, 2 ** 24) * abs(exact[x]) + Fraction(1, 2 ** 49) * M
                    err = abs(got - exact[x])
                    assert err <= bound, (i, k, q, x, float(err), float(bound))
                    if err:
                        n_inexact += 1
                        worst = max(worst, float(err / bound))
            n_zero += bool((rows[k][0] == rows[k][1]).all())
    print("%d planes x %d triangles, %d crossed, %d inexact coordinates, worst error / bound %.3f, %d zero-length segments"
          % (planes.shape[0], V.shape[0], ids.size, n_inexact, worst, n_zero))
    assert ids.size > 1500 and n_inexact > 100 and n_zero > 100       # thirds and sevenths occur, and so do vertices on the plane
    assert worst <= 1.0


def _loop_planes():
    tri = _solid()
    V = PE.vertices(tri)
    rng = np.random.default_rng(24)
    k = rng.integers(0, V.shape[0], 12)
    nrm = rng.normal(size=(12, 3))
    rand = np.concatenate([nrm, (nrm * V[k].astype(np.float64).mean(1)).sum(1, keepdims=True)], 1).astype(F)
    axis = []
    for ax, d in ((0, 1), (0, 3), (0, 6), (1, 2), (1, 4), (1, 6), (2, 1), (2, 3), (2, 5)):
        for sign in (1, -1):
            r = [0, 0, 0, sign * d]
            r[ax] = sign
            axis.append(r)
    skew = [[1, 2, 3, 1 * 3 + 2 * 3 + 3 * 2]]                           # through the grid vertex (3, 3, 2)
    return rand, np.asarray(axis, F), np.asarray(skew, F)


def test_sections_of_the_closed_solid_close_on_the_bits():
    tri = _solid()
    rand, axis, skew = _loop_planes()
    planes = np.concatenate([rand, axis, skew])
    assert planes.shape[0] == 31
    offsets, ids, seg, cr = PE.section(planes, tri)
    zero_len = []
    for i in range(planes.shape[0]):
        s = seg[offsets[i]:offsets[i + 1]]
        assert s.shape[0] >= 8 or (12 <= i < 30 and s.shape[0] == 0), i
        q0, q1 = PE.loop_balance(s)
        assert np.array_equal(q0, q1), i                                # every end point as often a q0 as a q1: closed loops
        zero_len.append(int((s[:, 0].view(np.uint32) == s[:, 1].view(np.uint32)).all(1).sum()))
    z_axis = zero_len[12:30]
    print("zero-length segments of the axis planes through integer coordinates:", z_axis)
    crossing = [z for z, i in zip(z_axis, range(12, 30)) if offsets[i + 1] > offsets[i]]
    assert len(crossing) == 14 and min(crossing) >= 12 and max(crossing) <= 28
    # (the other four are the solid's bounding planes x = 1, x = 6, y = 6, z = 1 with the normal pointing AT the solid: every vertex is
    # UP, nothing is crossed; their negations touch from the DOWN side and cross in zero-length segments and edges)
    assert not any(zero_len[:12])                                       # a random plane meets no vertex


def test_orientation_and_signed_area():
    tri = _solid()
    for plane in ([0, 0, 1, 1.5], [0, 0, -1, -1.5]):
        offsets, ids, seg, _ = PE.section(np.asarray([plane], F), tri)
        assert ids.size == 32
        assert PE.signed_area(seg, plane) == 8.0                        # counter-clockwise about the plane's own normal, both times
    # q0 -> q1 runs along n x N, triangle by triangle
    planes, _ = PS.planes_for(tri, 7)
    offsets, ids, seg, _ = PE.section(planes, tri)
    V = PE.vertices(tri).astype(np.float64)
    i = np.repeat(np.arange(planes.shape[0]), np.diff(offsets))
    N = np.cross(V[ids, 1] - V[ids, 0], V[ids, 2] - V[ids, 0])
    along = np.cross(planes[i, :3].astype(np.float64), N)
    d = seg[:, 1].astype(np.float64) - seg[:, 0].astype(np.float64)
    long_enough = np.linalg.norm(d, axis=1) > 1e-3
    assert long_enough.sum() > 500
    cosine = (d * along).sum(1)[long_enough] / (np.linalg.norm(d, axis=1) * np.linalg.norm(along, axis=1))[long_enough]
    assert cosine.min() > 0.999


def test_vertex_orders_keep_or_swap_exactly(bunny_small):
    for name in ("voxel_solid", "nasty"):
        tri, _ = PS.scene(name, bunny_small)
        planes, _ = PS.planes_for(tri, 11)
        V = PE.vertices(tri)
        offsets, ids, seg, cr = PE.section(planes, V)
        assert ids.size > 300
        for order in itertools.permutations(range(3)):
            even = order in ((0, 1, 2), (1, 2, 0), (2, 0, 1))
            o2, i2, s2, c2 = PE.section(planes, V[:, list(order)])
            assert np.array_equal(o2, offsets) and np.array_equal(i2, ids) and np.array_equal(c2, cr), order
            assert np.array_equal(s2.view(np.uint32), (seg if even else seg[:, ::-1]).view(np.uint32)), order
        o2, i2, s2, _ = PE.section(planes, PE.flipped(tri))
        assert np.array_equal(o2, offsets) and np.array_equal(i2, ids) and np.array_equal(s2.view(np.uint32), seg[:, ::-1].view(np.uint32))


def test_the_order_of_the_triangles_and_the_slicing_do_not_matter(bunny_small):
    tri, _ = PS.scene("nasty", bunny_small)
    planes, _ = PS.planes_for(tri, 13)
    offsets, ids, seg, cr = PE.section(planes, tri)
    perm = np.random.default_rng(5).permutation(tri.shape[0])
    o2, i2, s2, c2 = PE.section(planes, tri[perm])
    assert np.array_equal(o2, offsets) and np.array_equal(c2, cr[:, perm])
    for i in range(planes.shape[0]):                                    # the same triangles with the same rows, under their new ids
        a, b = slice(offsets[i], offsets[i + 1]), np.argsort(perm[i2[offsets[i]:offsets[i + 1]]])
        assert np.array_equal(perm[i2[a]][b], ids[a]) and np.array_equal(s2[a][b].view(np.uint32), seg[a].view(np.uint32))
    m = tri.shape[0]
    for slices in (1, 2, 7, 10 ** 6):
        S = PE.slices_of(planes.shape[0], m, slices)
        part = PE.part_of(cr, S)
        assert part.shape == (planes.shape[0], S) and np.array_equal(part.sum(1), np.diff(offsets))
    assert PE.slices_of(5, m, 10 ** 6) == -(-m // 64) and PE.slices_of(5, 10 ** 6, 10 ** 6) == 4096 and PE.slices_of(5, 0, 3) == 1


def test_the_edge_cases_of_the_crossing_rule():
    z = lambda *h: np.asarray([[[0, 0, h[0]], [1, 0, h[1]], [0, 1, h[2]]]], F)
    up, down = np.asarray([[0, 0, 1, 0]], F), np.asarray([[0, 0, -1, 0]], F)
    count = lambda pl, T: int(PE.classify(pl, T).sum())
    assert count(up, z(0, 0, 0)) == 0 and count(down, z(0, 0, 0)) == 0      # in the plane: never crossed (-0 - 0 = -0 is UP too)
    assert count(up, z(0, -1, -1)) == 1 and count(up, z(0, 1, 1)) == 0      # one vertex on it: from the DOWN side, from the UP side
    assert count(down, z(0, -1, -1)) == 0 and count(down, z(0, 1, 1)) == 1  # the negated plane: exactly the other way round
    assert count(up, z(0, 0, -1)) == 1 and count(up, z(0, 0, 1)) == 0       # an edge on it
    assert count(up, z(1, -1, 2)) == 1 and count(down, z(1, -1, 2)) == 1    # a proper crossing: both
    _, _, seg, _ = PE.section(up, z(0, -1, -1))
    assert np.array_equal(seg[0, 0], seg[0, 1]) and np.array_equal(seg[0, 0], F([0, 0, 0]))   # crossed in a segment of length zero
    _, _, seg, _ = PE.section(up, z(0, 0, -1))
    assert np.array_equal(seg[0], F([[1, 0, 0], [0, 0, 0]]))               # the edge p1 p2 itself: q0 on p2 -> p3, q1 on p3 -> p1
    # degenerate triangles are cut as the segments they are
    two = np.asarray([[[0, 0, 1], [0, 0, 1], [2, 0, -1]]], F)
    _, ids, seg, _ = PE.section(up, two)
    assert ids.size == 1 and np.array_equal(seg[0, 0], seg[0, 1]) and np.array_equal(seg[0, 0], F([1, 0, 0]))
    line = np.asarray([[[0, 0, -1], [2, 0, 1], [4, 0, 3]]], F)
    _, ids, seg, _ = PE.section(up, line)
    assert ids.size == 1 and np.array_equal(seg[0], F([[1, 0, 0], [1, 0, 0]]))
    assert count(up, np.asarray([[[3, 3, 3]] * 3], F)) == 0
    # non-finite triangles, planes that are not live
    for bad in (np.inf, -np.inf, np.nan):
        for j in range(9):
            T = z(1, -1, 2).copy()
            T.reshape(-1)[j] = bad
            assert count(up, T) == 0
    planes, kind = PS.planes_for(_solid(), 3)
    cr = PE.classify(planes, _solid())
    assert not cr[kind >= PS.KIND_MISS].any() and (kind == PS.KIND_DEAD).sum() == 10 and not PE.live(planes)[kind == PS.KIND_DEAD].any()
    assert PE.live(planes)[kind < PS.KIND_DEAD].all() and cr[kind == PS.KIND_CENTROID].any(1).all()
    # huge finite values: no fp64 operation overflows, the point stays on the edge
    big = np.asarray([[[3e38, -3e38, 3e38], [-3e38, 3e38, -3e38], [3e38, 3e38, -3e38]]], F)
    _, ids, seg, _ = PE.section(np.asarray([[3e38, 3e38, 3e38, -3e38]], F), big)
    assert ids.size == 1 and np.isfinite(seg).all()


def test_section_at_is_the_same_rule(bunny_small):
    tri, _ = PS.scene("open_solid", bunny_small)
    planes, kind = PS.planes_for(tri, 17)
    m = tri.shape[0]
    offsets, ids, seg, cr = PE.section(planes, tri)
    every = np.tile(np.arange(m, dtype=np.int32), (planes.shape[0], 1))
    c, side, sg = PE.section_at(planes, tri, every)
    assert np.array_equal(c, cr) and np.array_equal(sg[c].view(np.uint32), seg.view(np.uint32))
    assert not side[kind == PS.KIND_DEAD].any() and not sg[~c].any()
    assert (side[kind == PS.KIND_AXIS] == 0).any() and set(np.unique(side)) == {-1, 0, 1}
    closed = (side >= 0).any(2) & (side <= 0).any(2) & PE.live(planes)[:, None]       # a caller's closed touching rule
    assert (closed & ~c).any() and not (c & ~closed).any()
    out = np.int32([[-1, m], [2 ** 31 - 1, -2 ** 31]])
    c, side, sg = PE.section_at(planes[:2], tri, out)
    assert not c.any() and not side.any() and not sg.any()

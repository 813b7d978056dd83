"""The yardstick of the closest-point tests pinned to true geometry before the device is compared with it, and the parts of the binding
that need no device (include/ezrt_closest_point.h, ezrt_amd/query.py).

tests/closest_point_expected.py restates the header's definition in numpy float32.  Here, on the scenes and points
tests/test_gpu_closest_point.py uses: its distances agree with a float64 evaluation of the true point-triangle distance (written
differently: plane projection and the three edges), the lowest index wins among identical triangles, d_max cuts at the winner's own
distance exactly, and the non-finite points miss."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import closest_point_expected as E  # noqa: E402

# |dist32 - dist64| <= MARGIN * max(dist64, largest |coordinate| of p and of the scene).  4 x the largest value measured on the CPU for
# the fixed seeds below (1.03e-7 on `nasty`, 2026-10-17; bunny 6.0e-8, ties 7.6e-8, not_nested 7.0e-8): the seeds are fixed, and the bound only has to catch a wrong region
# (an error of the size of a triangle), not a rounding.
MARGIN = 4 * 1.03e-7

_cache = {}


def _case(name, bunny_small):
    if name not in _cache:
        tri, nodes, _ = A.scene(name, bunny_small)
        pts, n_finite = E.points_for(tri, nodes, 300 + A.SCENES.index(name))
        _cache[name] = (tri, nodes, pts, n_finite, E.closest_point(pts, tri, with_ties=True))
    return _cache[name]


def _seg(p, a, b):
    ab = b - a
    t = np.clip(np.einsum("...k,...k", p - a, ab) / np.maximum(np.einsum("...k,...k", ab, ab), 1e-300), 0.0, 1.0)
    return np.linalg.norm(p - (a + ab * t[..., None]), axis=-1)


def true_distance(points, tri):
    """float64: min over the triangles of the distance to the plane projection where it falls inside, else to the nearest edge"""
    P = np.asarray(tri, np.float64).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    a, b, c = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    out = np.empty(points.shape[0])
    with np.errstate(all="ignore"):
        for i0 in range(0, points.shape[0], 64):
            p = np.asarray(points[i0:i0 + 64], np.float64)[:, None, :]
            d = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
            n = np.cross(b - a, c - a)
            nn = np.einsum("...k,...k", n, n)
            h = np.einsum("...k,...k", p - a, n) / nn
            f = p - n * h[..., None]                                   # the foot of the perpendicular
            inside = ((np.einsum("...k,...k", np.cross(b - a, f - a), n) >= 0) & (np.einsum("...k,...k", np.cross(c - b, f - b), n) >= 0) &
                      (np.einsum("...k,...k", np.cross(a - c, f - c), n) >= 0) & (nn > 0))
            d = np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn)), d)
            out[i0:i0 + 64] = d.min(1)
    return out


@pytest.mark.parametrize("name", A.SCENES)
def test_against_true_geometry(bunny_small, name):
    tri, nodes, pts, n_finite, (win, point, dist, bary, ties) = _case(name, bunny_small)
    p = pts[:n_finite]
    d64 = true_distance(p, tri)
    scale = np.maximum(d64, max(float(np.abs(p).max()), float(np.abs(tri[:, :9]).max())))
    err = np.abs(dist[:n_finite].astype(np.float64) - d64) / scale
    print("%s: largest relative error %.3g" % (name, err.max()))
    assert err.max() <= MARGIN
    # the outputs belong together: point = p1 + (p2 - p1) v + (p3 - p1) w up to rounding, |p - point| = dist
    P = tri[:, :9].reshape(-1, 3, 3).astype(np.float64)[win[:n_finite]]
    v, w = bary[:n_finite, 0:1].astype(np.float64), bary[:n_finite, 1:2].astype(np.float64)
    rebuilt = P[:, 0] + (P[:, 1] - P[:, 0]) * v + (P[:, 2] - P[:, 0]) * w
    assert np.abs(rebuilt - point[:n_finite]).max() <= 1e-5 * np.abs(tri[:, :9]).max()
    assert np.all(np.abs(np.linalg.norm(p.astype(np.float64) - point[:n_finite], axis=1) - dist[:n_finite]) <= 4 * MARGIN * scale)
    assert (v >= 0).all() and (w >= 0).all() and (v + w <= 1 + 1e-6).all()


def test_tie_rule_bounds_and_misses(bunny_small):
    tri, nodes, pts, n_finite, (win, point, dist, bary, ties) = _case("ties", bunny_small)
    # identical copies: every winner has at least two equals, and is the lowest index among the triangles at its dist2
    assert (ties[:n_finite] >= 3).all()
    P = tri[:, :9]
    for i in range(0, n_finite, 25):
        equal = np.nonzero((P == P[win[i]]).all(1))[0]
        assert equal.size >= 3 and win[i] == equal.min()
    # the non-finite and huge points miss: (-1, zeros, +inf, zeros)
    assert (win[:n_finite] >= 0).all() and (win[n_finite:] < 0).all()
    assert not point[n_finite:].any() and not bary[n_finite:].any() and np.all(np.isposinf(dist[n_finite:]))
    # d_max at the winner's own dist keeps it, one ulp below loses it (to a farther triangle never: nothing is nearer), one above keeps it
    sel = np.arange(0, n_finite, 9)
    p, own = pts[sel], dist[sel]
    at = E.closest_point(p, tri, own)
    above = E.closest_point(p, tri, np.nextafter(own, np.float32(np.inf)))
    below = E.closest_point(p, tri, np.nextafter(own, np.float32(-np.inf)))
    sq = own * own == (dist[sel] * dist[sel])                        # B = d_max * d_max is compared with dist2, not with dist
    assert sq.all()
    assert np.array_equal(above[0], win[sel])
    with np.errstate(all="ignore"):
        d2 = E.per_triangle(p[:, None, :], *(tri[win[sel], 3 * k:3 * k + 3][None] for k in range(3)))[3]
    d2 = d2[np.arange(sel.size), np.arange(sel.size)]
    assert np.array_equal(at[0] >= 0, d2 <= own * own) and np.array_equal(at[0][at[0] >= 0], win[sel][at[0] >= 0])
    lower = np.nextafter(own, np.float32(-np.inf))
    assert np.array_equal(below[0] >= 0, (d2 <= lower * lower) & (lower >= 0))    # (below a dist of 0 lies a negative d_max)
    assert (below[0] < 0).any() and (at[0] >= 0).any()
    for bad in (np.full(sel.size, np.nan, np.float32), np.full(sel.size, -1.0, np.float32)):
        assert (E.closest_point(p, tri, bad)[0] < 0).all()
    assert np.array_equal(E.closest_point(p, tri, np.full(sel.size, np.inf, np.float32))[0], win[sel])


def test_exact_tie_condition_of_the_device_test(bunny_small):
    ties = _case("bunny", bunny_small)[4][4]
    assert (ties >= 2).mean() >= 0.10


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import query
    assert query.ClosestPoint._fields == ("tri", "point", "dist", "bary")
    with pytest.raises(TypeError, match="GPU tensor"):
        query.closest_point(None, torch.zeros((4, 3), dtype=torch.float32))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.closest_point(None, np.zeros((4, 3), np.float32))


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ezrt_closest_point.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.CLOSEST_POINT_ABI) == ["ezrt_query_closest_point_device"]
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.CLOSEST_POINT_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "REFIT_ABI", "BUILD_ABI",
                  "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other

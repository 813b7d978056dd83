"""The yardstick of the nearest-K tests pinned before the device is compared with it, and the parts of the binding that need no device
(include/ezrt_nearest.h, ezrt_amd/query.py: nearest, closest_point_at).

tests/nearest_expected.py restates the header's definition in numpy float32 on tests/closest_point_expected.py's per-triangle
function.  Here: it equals a plain Python double loop on a tiny case; K = 1 is closest_point_expected.closest_point on the bits; the
first j slots of a K-row are the j-row; the counts agree with a float64 evaluation of the true point-triangle distance (written
differently) for every pair that is not within rounding of d_max."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import closest_point_expected as E  # noqa: E402
import nearest_expected as NE  # noqa: E402
from test_closest_point_expected import _seg  # noqa: E402

_cache = {}


def _case(name, bunny_small):
    if name not in _cache:
        tri, nodes, _ = A.scene(name, bunny_small)
        pts, n_finite = E.points_for(tri, nodes, 300 + A.SCENES.index(name))
        pts = np.ascontiguousarray(np.concatenate([pts[:n_finite:6], pts[n_finite::10]]))   # a sixth of the points: all kinds
        _cache[name] = (tri, pts, len(range(0, n_finite, 6)), NE.dist2_all(pts, tri))
    return _cache[name]


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_against_a_plain_double_loop():
    rng = np.random.default_rng(5)
    tri = np.zeros((23, 36), np.float32)
    tri[:, :9] = rng.uniform(-1, 1, (23, 9))
    tri[7, :9] = tri[3, :9]                                            # identical triangles: equal dist2, ascending index
    tri[19, :9] = tri[3, :9]
    tri[11, 4] = np.nan                                                # never a candidate
    pts = rng.uniform(-1.5, 1.5, (9, 3)).astype(np.float32)
    pts[8, 1] = np.inf                                                 # no candidates
    d_max = np.float32([np.inf, 0.9, 0.5, 0.0, -1.0, np.nan, 1.5, 0.7, 1.0])
    K = 5
    ids, dist, count = NE.nearest(pts, tri, K, d_max)
    for i in range(pts.shape[0]):
        found = []
        for k in range(tri.shape[0]):
            with np.errstate(all="ignore"):
                d2 = E.per_triangle(pts[i].reshape(1, 1, 3), *(tri[k, 3 * c:3 * c + 3].reshape(1, 1, 3) for c in range(3)))[3][0, 0]
                ok = bool(d_max[i] >= 0) and bool(np.isfinite(d2)) and bool(d2 <= d_max[i] * d_max[i])
            if ok:
                found.append((float(d2), k))
        found.sort()                                                   # by the pair (dist2, k)
        assert count[i] == len(found)
        want_ids = [k for _, k in found[:K]] + [-1] * (K - min(K, len(found)))
        want_d = [np.sqrt(np.float32(d)) for d, _ in found[:K]] + [np.float32(np.inf)] * (K - min(K, len(found)))
        assert ids[i].tolist() == want_ids, i
        assert _same(dist[i], np.float32(want_d)), i
    assert count[0] == 22 and count[4] == count[5] == count[8] == 0 and 0 < count[1] < 22
    row = ids[0].tolist()
    assert 7 not in row or row.index(3) + 1 == row.index(7)            # the copies are neighbours, lowest index first
    # more slots than triangles
    ids, dist, count = NE.nearest(pts[:1], tri, 64)
    assert (ids[0, :22] >= 0).all() and (ids[0, 22:] == -1).all() and np.isposinf(dist[0, 22:]).all() and count[0] == 22


@pytest.mark.parametrize("name", A.SCENES)
def test_slot_0_prefixes_and_order(bunny_small, name):
    tri, pts, n_finite, d2 = _case(name, bunny_small)
    rng = np.random.default_rng(3)
    for d_max in (None, rng.uniform(0.0, 0.5, pts.shape[0]).astype(np.float32)):
        ids, dist, count = NE.nearest(pts, tri, 64, d_max, d2=d2)
        cp = E.closest_point(pts, tri, d_max)
        one = NE.nearest(pts, tri, 1, d_max, d2=d2)
        assert np.array_equal(one[0][:, 0], cp[0]) and _same(one[1][:, 0], cp[2])      # K = 1 is closest_point, on the bits
        for j in (1, 2, 4, 63):                                                    # the first j slots of a K-row are the j-row
            sub = NE.nearest(pts, tri, j, d_max, d2=d2)
            assert np.array_equal(sub[0], ids[:, :j]) and _same(sub[1], dist[:, :j]) and np.array_equal(sub[2], count)
        used = ids >= 0
        assert np.array_equal(used.sum(1), np.minimum(count, 64)) and np.all(np.isposinf(dist[~used]))
        assert (count[n_finite:] == 0).all() and (d_max is not None or (count[:n_finite] > 0).all())
        for i in range(0, pts.shape[0], 7):                                        # no id twice; ascending (dist, id)
            row = ids[i][used[i]]
            assert np.unique(row).size == row.size
            pairs = list(zip(d2[i, row].tolist(), row.tolist()))
            assert pairs == sorted(pairs)


@pytest.mark.parametrize("name", A.SCENES)
def test_counts_against_true_geometry(bunny_small, name):
    """float64: the distance to the plane projection where it falls inside, else to the nearest edge -- per PAIR.  A pair counts where
    its float64 distance is <= d_max; pairs within 4 x the rounding error measured here of d_max are left out of the comparison."""
    tri, pts, n_finite, d2 = _case(name, bunny_small)
    p32 = pts[:n_finite:3]
    P = np.asarray(tri, np.float64).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    a, b, c = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    p = p32.astype(np.float64)[:, None, :]
    with np.errstate(all="ignore"):
        d = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
        nrm = np.cross(b - a, c - a)
        nn = np.einsum("...k,...k", nrm, nrm)
        h = np.einsum("...k,...k", p - a, nrm) / nn
        f = p - nrm * h[..., None]
        inside = ((np.einsum("...k,...k", np.cross(b - a, f - a), nrm) >= 0) & (np.einsum("...k,...k", np.cross(c - b, f - b), nrm) >= 0) &
                  (np.einsum("...k,...k", np.cross(a - c, f - c), nrm) >= 0) & (nn > 0))
        d64 = np.where(inside, np.minimum(d, np.abs(h) * np.sqrt(nn)), d)
    d32 = np.sqrt(d2[:n_finite:3].astype(np.float64))
    scale = np.maximum(d64, np.maximum(np.abs(p32).max(1).astype(np.float64), float(np.abs(tri[:, :9]).max()))[:, None])   # per point
    ok = np.isfinite(d32)
    err = float((np.abs(d32 - d64) / scale)[ok].max())
    print("%s: largest relative error of a pair %.3g" % (name, err))
    # (no bound on err itself: slivers of width 1e-5 lose digits in the face region, and test_closest_point_expected.py bounds the
    # winners' error; what is asserted below is that the margin leaves almost every pair in the comparison)
    size = float(np.ptp(np.percentile(tri[:, :9].reshape(-1, 3), [2, 98], axis=0), axis=0).max())
    for frac in (0.02, 0.05, 0.3):
        d_max = np.full(p32.shape[0], frac * size, np.float32)
        count = NE.nearest(p32, tri, 1, d_max, d2=d2[:n_finite:3])[2]
        clear = np.abs(d64 - np.float64(d_max)[:, None]) > 4 * err * scale
        lo = (clear & (d64 <= np.float64(d_max)[:, None])).sum(1)
        hi = lo + (~clear).sum(1)
        assert np.all((lo <= count) & (count <= hi)), frac
        assert (lo > 0).any() and (~clear).mean() < 0.01
        # ... and pair by pair: a clear pair is a candidate exactly where its true distance is within d_max
        with np.errstate(all="ignore"):
            cand = np.isfinite(d2[:n_finite:3]) & (d2[:n_finite:3] <= (d_max * d_max)[:, None])
        assert np.array_equal(cand[clear], (d64 <= np.float64(d_max)[:, None])[clear]), frac


def test_argument_errors_that_need_no_device():
    torch = pytest.importorskip("torch")
    from ezrt_amd import _abi, query
    assert query.Nearest._fields == ("tri", "dist", "count") and _abi.NEAREST_MAX == 64
    pts = torch.zeros((4, 3), dtype=torch.float32)
    for k in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be an int"):
            query.nearest(None, pts, k)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.nearest(None, pts, 4)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.nearest(None, np.zeros((4, 3), np.float32), 4)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.closest_point_at(None, pts, torch.zeros(4, dtype=torch.int32))


def test_binding_table_matches_the_header():
    import ctypes as C
    import re

    from ezrt_amd import _abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ezrt_nearest.h")).read()
    assert int(re.search(r"#define\s+EZRT_NEAREST_MAX\s+(\d+)", text).group(1)) == _abi.NEAREST_MAX == 64
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(ezrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src))
    assert sorted(protos) == sorted(_abi.NEAREST_ABI) == ["ezrt_closest_point_at_device", "ezrt_query_nearest_device"]
    hip = _abi.load_hip()                                                      # dlopen only
    for name, params in protos.items():
        res, args = _abi.NEAREST_ABI[name]
        want = [C.c_void_p if "*" in p else {"int": C.c_int, "float": C.c_float}[p.split()[0]] for p in params.split(",")]
        assert res is C.c_int and args == want, name
        assert getattr(hip, name).argtypes == args
    for other in ("TRACE_ABI", "HOST_ABI", "QUERY_ABI", "SURFACE_ABI", "SHADE_ABI", "PATH_ABI", "MULTIHIT_ABI", "CLOSEST_POINT_ABI",
                  "REFIT_ABI", "BUILD_ABI", "MGPU_ABI"):
        assert not set(protos) & set(getattr(_abi, other)), other

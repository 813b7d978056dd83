"""Closest-point queries on device tensors (include/ezrt_closest_point.h, ezrt_amd/query.py: closest_point), every output compared on
the bits (a NaN equal to a NaN) with tests/closest_point_expected.py -- the header's definition restated in numpy float32 over ALL
triangles, pinned to true geometry by tests/test_closest_point_expected.py:

* on the Bunny scene, 3 identical copies of a mesh (the lowest index wins), adversarial geometry (slivers, a coplanar grid, duplicates,
  a far cluster) and a scene that does not prune (the sweep route), with points in the box, exactly on the surface, just off
  vertices (exact ties), on box planes of the tree, far away, and non-finite or huge ones;
* batches of 1, 63, 64, 65 and 257 points, every combination of NULL outputs;
* d_max: random, at the winner's own distance and one ulp either side of it, +inf, 0, negative, NaN;
* the pruned route against the sweep route, a refit, stream order, a render call beside it, untouched counters, the error contract.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import closest_point_expected as E  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, nodes, points, the expected answer with tie counts, the device scene) of a named scene, computed once and shared"""
    if name not in _cache:
        tri, nodes, _ = A.scene(name, bunny_small)
        pts, n_finite = E.points_for(tri, nodes, 300 + A.SCENES.index(name))
        _cache[name] = (tri, nodes, pts, n_finite, E.closest_point(pts, tri, with_ties=True), hip.scene_create(tri, nodes))
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _query(sg, pts, dev, d_max=None, **kw):
    out = query.closest_point(sg, _gpu(pts, dev), None if d_max is None else _gpu(d_max, dev), **kw)
    torch.cuda.synchronize()
    assert isinstance(out, query.ClosestPoint)
    n = pts.shape[0]
    assert out.tri.dtype == torch.int32 and out.point.dtype == out.dist.dtype == out.bary.dtype == torch.float32
    assert tuple(out.tri.shape) == (n,) == tuple(out.dist.shape) and tuple(out.point.shape) == (n, 3) and tuple(out.bary.shape) == (n, 2)
    return tuple(x.cpu().numpy() for x in out)


def _expect(got, want, what):
    tri, point, dist, bary = got
    assert np.array_equal(tri, want[0]), "%s: %d triangle ids differ" % (what, int((tri != want[0]).sum()))
    assert _same(dist, want[2]), "%s: %d distances differ" % (what, int((_bits(dist) != _bits(want[2])).sum()))
    assert _same(point, want[1]), "%s: points differ" % what
    assert _same(bary, want[3]), "%s: barycentrics differ" % what


@pytest.mark.parametrize("name", A.SCENES)
def test_answers_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, pts, n_finite, want, sg = _case(name, hip, bunny_small)
    if name == "not_nested":
        assert sg.prune_info()["mode"] == -1                           # pruning is unavailable: the sweep route runs
    else:
        assert sg.prune_info()["mode"] != -1
    assert (want[0][:n_finite] >= 0).all() and (want[0][n_finite:] < 0).all()   # the non-finite and huge points miss, nothing else
    if name == "bunny":                                                # the exact-tie condition, on the restatement alone
        assert (want[4] >= 2).mean() >= 0.10
    if name == "ties":                                                 # 3 copies: every winner has equals, and is the lowest of them
        assert (want[4][:n_finite] >= 3).all()
    got = _query(sg, pts, dev)
    _expect(got, want, name)
    miss = got[0] < 0
    assert miss.any() and not got[1][miss].any() and not got[3][miss].any() and np.all(np.isposinf(got[2][miss]))


def test_batch_sizes_and_null_outputs(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, want, sg = _case("bunny", hip, bunny_small)
    for n in (1, 63, 64, 65, 257):
        sel = np.arange(n) * 7 % pts.shape[0]
        _expect(_query(sg, pts[sel], dev), tuple(x[sel] for x in want[:4]), "n=%d" % n)
    # every combination of point, dist and bary being NULL (the C entry point); what is not passed is not touched
    n = 257
    P = C.c_void_p
    p = _gpu(pts[:n], dev)
    for use in itertools.product((False, True), repeat=3):
        ids = torch.full((n,), -7, dtype=torch.int32, device=dev)
        bufs = [torch.full((n, 3), 7.0, device=dev), torch.full((n,), 7.0, device=dev), torch.full((n, 2), 7.0, device=dev)]
        args = [P(b.data_ptr()) if u else None for b, u in zip(bufs, use)]
        assert hip.lib.ezrt_query_closest_point_device(sg._h, P(p.data_ptr()), None, n, P(ids.data_ptr()), *args, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), want[0][:n]), use
        for b, u, w in zip(bufs, use, want[1:4]):
            if u:
                assert _same(b.cpu().numpy(), w[:n]), use
            else:
                assert bool((b == 7.0).all()), use


@pytest.mark.parametrize("name", A.SCENES)
def test_d_max(hip, bunny_small, dev, name):
    tri, nodes, pts, n_finite, want, sg = _case(name, hip, bunny_small)
    rng = np.random.default_rng(11)
    sel = rng.permutation(pts.shape[0])[:300]
    pts, own = pts[sel], want[2][sel]
    own = np.where(np.isfinite(own), own, np.float32(1.0)).astype(np.float32)
    n = pts.shape[0]
    cases = {
        "uniform": rng.uniform(0.0, 1.0, n).astype(np.float32),
        "own dist": own,
        "own dist + ulp": np.nextafter(own, np.float32(np.inf)),
        "own dist - ulp": np.nextafter(own, np.float32(-np.inf)),
        "+inf": np.full(n, np.inf, np.float32),
        "zero": np.zeros(n, np.float32),
        "negative": -rng.uniform(0.001, 3.0, n).astype(np.float32),
        "nan": np.full(n, np.nan, np.float32),
    }
    for what, d_max in cases.items():
        _expect(_query(sg, pts, dev, d_max), E.closest_point(pts, tri, d_max), "%s %s" % (name, what))
    assert (_query(sg, pts, dev, cases["negative"])[0] < 0).all() and (_query(sg, pts, dev, cases["nan"])[0] < 0).all()


def test_routes_agree(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, want, sg = _case("bunny", hip, bunny_small)
    swept = hip.scene_create(*A.not_nested(bunny_small))               # the same triangles, created so that pruning is unavailable
    assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    a, b = _query(sg, pts, dev), _query(swept, pts, dev)
    _expect(a, b, "pruned against sweep")


def test_after_a_refit(hip, bunny_small, dev):
    tri, nodes = bunny_small.tri, bunny_small.nodes
    pts = E.points_for(tri, nodes, 321)[0][::3]
    ang = 0.4
    R = np.float32([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    moved = tri.copy()
    for k in range(6):                                                 # p1 p2 p3 n1 n2 n3
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] @ R.T
    moved[:, 1:9:3] += np.float32(0.1)
    sg = hip.scene_create(tri, nodes)
    first = _query(sg, pts, dev)
    refit.refit(sg, moved)
    got = _query(sg, pts, dev)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))
    assert sg.prune_info()["mode"] != -1 and fresh.prune_info()["mode"] != -1
    assert not np.array_equal(first[0], got[0])
    _expect(got, _query(fresh, pts, dev), "after a refit")
    _expect(got, E.closest_point(pts, moved), "after a refit, against the definition")


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, want, sg = _case("ties", hip, bunny_small)
    src = _gpu(pts, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                   # the points are written on `side`, behind the sleep
    a = query.closest_point(sg, p, stream=side)                        # issued from the default stream's context, onto `side`
    b = query.closest_point(sg, p, stream=side.cuda_stream)            # a raw handle
    side.synchronize()
    _expect(tuple(x.cpu().numpy() for x in a), want, "side stream")
    _expect(tuple(x.cpu().numpy() for x in b), want, "raw handle")


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, want, _ = _case("bunny", hip, bunny_small)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    p = _gpu(pts, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    query.closest_point(sg, p)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.closest_point(sg, p, stream=b)
    torch.cuda.synchronize()
    assert _same(frame.cpu().numpy(), alone.cpu().numpy())
    _expect(tuple(x.cpu().numpy() for x in got), want, "beside a render call")


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, pts, n_finite, want, sg = _case("bunny", hip, bunny_small)
    lib = hip.lib
    n = 500
    p = _gpu(pts[:n], dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    q = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    d = torch.zeros(n, dtype=torch.float32, device=dev)
    host_pts = np.ascontiguousarray(pts[:n])
    host_ids = np.zeros(n, np.int32)
    host_f = np.zeros((n, 3), np.float32)
    P = C.c_void_p
    f = lib.ezrt_query_closest_point_device
    torch.cuda.synchronize()
    args = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("d_max"), kw.get("n", n), kw.get("tri", P(ids.data_ptr())),
                         kw.get("point", P(q.data_ptr())), kw.get("dist", P(d.data_ptr())), kw.get("bary"), None]
    assert f(*args()) == 0
    # host memory is rejected, never read or written
    assert f(*args(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*args(tri=P(host_ids.ctypes.data))) == EZRT_ERR_INVALID
    assert f(*args(d_max=P(host_f.ctypes.data))) == EZRT_ERR_INVALID
    for name in ("point", "dist", "bary"):
        assert f(*args(**{name: P(host_f.ctypes.data)})) == EZRT_ERR_INVALID
    assert not host_ids.any() and not host_f.any()
    # n < 0, NULL
    assert f(*args(n=-1)) == EZRT_ERR_INVALID
    assert f(*args(s=None)) == EZRT_ERR_INVALID and f(*args(pts=None)) == EZRT_ERR_INVALID and f(*args(tri=None)) == EZRT_ERR_INVALID
    assert f(*args(n=0)) == 0
    # the rejected calls left no HIP error behind: the next call works
    _expect(_query(sg, pts[:n], dev), tuple(x[:n] for x in want[:4]), "after the errors")
    # the wrapper
    with pytest.raises(TypeError):
        query.closest_point(sg, torch.from_numpy(host_pts))
    with pytest.raises(TypeError):
        query.closest_point(bunny_small.upload(oracle), p)
    with pytest.raises(ValueError):
        query.closest_point(sg, p, d[:10].contiguous())
    with pytest.raises(ValueError):
        query.closest_point(sg, torch.zeros((4, 6), device=dev))
    e = query.closest_point(sg, torch.empty((0, 3), device=dev))
    assert tuple(e.tri.shape) == (0,) and tuple(e.point.shape) == (0, 3) and tuple(e.bary.shape) == (0, 2)
    lead = query.closest_point(sg, p.reshape(5, 100, 3))
    torch.cuda.synchronize()
    assert tuple(lead.tri.shape) == (5, 100) and tuple(lead.point.shape) == (5, 100, 3) and tuple(lead.bary.shape) == (5, 100, 2)
    assert np.array_equal(lead.tri.cpu().numpy().reshape(-1), want[0][:n])

"""Nearest-K queries on device tensors (include/ezrt_nearest.h, ezrt_amd/query.py: nearest, closest_point_at), every output compared on
the bits (a NaN equal to a NaN) with tests/nearest_expected.py -- the header's definition restated in numpy float32 over ALL triangles
with a stable sort, pinned by tests/test_nearest_expected.py:

* on the scenes and points of the closest-point tests (the Bunny scene, 3 identical copies of a mesh, adversarial geometry, a scene that
  does not prune: the sweep route), K = 1, 2, 4 and 64, with and without the count; misses give rows of (-1, +inf) and a count of 0;
* ties at the cut: the K-th and the first excluded triangle at exactly the same dist2, where only the id decides;
* slot 0 against query.closest_point, the first columns of K = 64 against K = 4; more slots than candidates;
* batches of 1, 63, 64, 65 and 257 points with K = 3 and 63 (the cooperative finishing pass across a partial wave, an odd row length);
* d_max: random, at the winner's and at the K-th entry's own distance and one ulp either side, +inf, 0, negative, NaN;
* the pruned route against the sweep route, closest_point_at on the rows, a refit, stream order, a render call beside it, untouched
  counters, the error contract.
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
import nearest_expected as NE  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
KS = (1, 2, 4, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, nodes, points, the number of finite points, dist2 of every pair, the expected 65-rows and counts, the device scene) of a
    named scene, computed once and shared; the expected K-row is the first K columns (test_nearest_expected.py: the prefix property)"""
    if name not in _cache:
        tri, nodes, _ = A.scene(name, bunny_small)
        pts, n_finite = E.points_for(tri, nodes, 300 + A.SCENES.index(name))
        d2 = NE.dist2_all(pts, tri)
        _cache[name] = (tri, nodes, pts, n_finite, d2, NE.nearest(pts, tri, 65, d2=d2), hip.scene_create(tri, nodes))
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _host(out):
    return tuple(None if x is None else x.cpu().numpy() for x in out)


def _query(sg, pts, k, dev, d_max=None, count=False, **kw):
    out = query.nearest(sg, _gpu(pts, dev), k, None if d_max is None else _gpu(d_max, dev), count, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, query.Nearest)
    n = pts.shape[0]
    assert out.tri.dtype == torch.int32 and out.dist.dtype == torch.float32 and tuple(out.tri.shape) == (n, k) == tuple(out.dist.shape)
    if count:
        assert out.count.dtype == torch.int32 and tuple(out.count.shape) == (n,)
    else:
        assert out.count is None
    return _host(out)


def _expect(got, want, what):
    """`got` (tri, dist, count or None) against `want` (tri, dist, count) cut to got's K"""
    k = got[0].shape[1]
    ids, dist = want[0][:, :k], want[1][:, :k]
    assert np.array_equal(got[0], ids), "%s: %d triangle ids differ" % (what, int((got[0] != ids).sum()))
    assert _same(got[1], dist), "%s: %d distances differ" % (what, int((_bits(got[1]) != _bits(dist)).sum()))
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), "%s: %d counts differ" % (what, int((got[2] != want[2]).sum()))


def _both(sg, pts, k, dev, want, what, d_max=None):
    for count in (False, True):
        _expect(_query(sg, pts, k, dev, d_max, count), want, "%s K=%d count=%s" % (what, k, count))


@pytest.mark.parametrize("name", A.SCENES)
def test_answers_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, pts, n_finite, d2, want, sg = _case(name, hip, bunny_small)
    if name == "not_nested":
        assert sg.prune_info()["mode"] == -1                           # pruning is unavailable: the sweep route runs
    else:
        assert sg.prune_info()["mode"] != -1
    assert (want[2][:n_finite] > 64).all() and (want[2][n_finite:] == 0).all()   # the non-finite and huge points miss, nothing else
    for k in KS:
        for count in (False, True):
            got = _query(sg, pts, k, dev, count=count)
            _expect(got, want, "%s K=%d count=%s" % (name, k, count))
            assert (got[0][n_finite:] == -1).all() and np.all(np.isposinf(got[1][n_finite:]))
            assert (got[0][:n_finite] >= 0).all()


def test_ties_at_the_cut(hip, bunny_small, dev):
    """slot K - 1 and the first excluded triangle at the same dist2: only the id decides who is in the row"""
    tri, nodes, pts, n_finite, d2, want, sg = _case("ties", hip, bunny_small)
    r = np.arange(n_finite)
    assert np.array_equal(d2[r, want[0][:n_finite, 3]], d2[r, want[0][:n_finite, 4]])   # 3 identical copies: ranks 4 and 5 are equal
    assert (want[0][:n_finite, 3] < want[0][:n_finite, 4]).all()
    _both(sg, pts, 4, dev, want, "ties")
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    r = np.arange(n_finite)
    for k in (1, 2):
        tie = d2[r, want[0][:n_finite, k - 1]] == d2[r, want[0][:n_finite, k]]
        print("bunny K=%d: %.1f %% of the points have a tie at the cut" % (k, 100 * tie.mean()))
        assert tie.mean() >= 0.10
        _both(sg, pts, k, dev, want, "bunny")


def test_slot_0_and_prefix_on_the_device(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    rng = np.random.default_rng(17)
    own = np.where(np.isfinite(want[1][:, 0]), want[1][:, 0], np.float32(1.0)).astype(np.float32)
    p = _gpu(pts, dev)
    cases = {"none": None, "uniform": rng.uniform(0.0, 0.3, pts.shape[0]).astype(np.float32), "own": own,
             "own - ulp": np.nextafter(own, np.float32(-np.inf))}
    winners = {}
    for what, d_max in cases.items():
        dm = None if d_max is None else _gpu(d_max, dev)
        cp = query.closest_point(sg, p, dm)
        for count in (False, True):
            one = query.nearest(sg, p, 1, dm, count)
            torch.cuda.synchronize()
            assert torch.equal(one.tri[:, 0], cp.tri) and _same(one.dist[:, 0].cpu().numpy(), cp.dist.cpu().numpy()), what
        winners[what] = int((cp.tri >= 0).sum())
    # the d_max cases reach both outcomes: every finite point has a winner without a d_max, a random d_max keeps some, and one ulp below
    # the own distance loses winners that the own distance keeps (to a farther triangle never: nothing is nearer, so those points miss)
    assert winners["none"] == n_finite and 0 < winners["uniform"] < n_finite and winners["own - ulp"] < winners["own"]
    for count in (False, True):
        wide, narrow = query.nearest(sg, p, 64, count=count), query.nearest(sg, p, 4, count=count)
        torch.cuda.synchronize()
        assert torch.equal(wide.tri[:, :4], narrow.tri) and _same(wide.dist[:, :4].cpu().numpy(), narrow.dist.cpu().numpy())


def test_more_slots_than_candidates(hip, dev):
    T = np.zeros((2, 36), np.float32)
    T[0, :9] = (0, 0, 0, 1, 0, 0, 0, 1, 0)
    T[1, :9] = (0, 0, 1, 1, 0, 1, 0, 1, 1)
    T[:, 9:18] = np.tile([0, 0, 1], 3)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    hs = S.HostScene()
    hs.addTriangles(T)
    hs.buildBVHwithSAH(1)
    tri, nodes = hs.encode()
    sg = hip.scene_create(tri, nodes)
    rng = np.random.default_rng(23)
    pts = rng.uniform(-0.5, 1.5, (200, 3)).astype(np.float32)
    d_max = np.full(200, 0.7, np.float32)
    want = NE.nearest(pts, tri, 64, d_max)
    assert {0, 1, 2} == set(want[2].tolist())                            # 0 < count < K occurs, with 1 and with 2 candidates
    for count in (False, True):
        got = _query(sg, pts, 64, dev, d_max, count)
        _expect(got, want, "two triangles")
        for c in (0, 1, 2):
            rows = want[2] == c
            assert (got[0][rows, c:] == -1).all() and np.all(np.isposinf(got[1][rows, c:])) and (got[0][rows, :c] >= 0).all()
    _both(sg, pts, 64, dev, NE.nearest(pts, tri, 64), "two triangles, no d_max")


def test_batch_sizes(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    d_max = np.random.default_rng(29).uniform(0.0, 0.25, pts.shape[0]).astype(np.float32)   # rows of every fill, empty to full
    near = NE.nearest(pts, tri, 63, d_max, d2=d2)
    assert (near[2] == 0).any() and ((near[2] > 0) & (near[2] < 3)).any() and ((near[2] > 3) & (near[2] < 63)).any() and (near[2] > 63).any()
    for n in (1, 63, 64, 65, 257):
        sel = np.arange(n) * 7 % pts.shape[0]
        for k in (3, 63):
            _both(sg, pts[sel], k, dev, tuple(x[sel] for x in want), "n=%d" % n)
            _both(sg, pts[sel], k, dev, tuple(x[sel] for x in near), "n=%d with d_max" % n, d_max[sel])


@pytest.mark.parametrize("name", A.SCENES)
def test_d_max(hip, bunny_small, dev, name):
    tri, nodes, pts, n_finite, d2, want, sg = _case(name, hip, bunny_small)
    rng = np.random.default_rng(11)
    sel = rng.permutation(pts.shape[0])[:300]
    K = 4
    pts, d2 = pts[sel], d2[sel]
    finite = lambda x: np.where(np.isfinite(x), x, np.float32(1.0)).astype(np.float32)
    own, kth = finite(want[1][sel, 0]), finite(want[1][sel, K - 1])
    n = pts.shape[0]
    up, down = np.float32(np.inf), np.float32(-np.inf)
    cases = {
        "uniform": rng.uniform(0.0, 1.0, n).astype(np.float32),
        "own dist": own,
        "own dist + ulp": np.nextafter(own, up),
        "own dist - ulp": np.nextafter(own, down),
        "+inf": np.full(n, np.inf, np.float32),
        "zero": np.zeros(n, np.float32),
        "negative": -rng.uniform(0.001, 3.0, n).astype(np.float32),
        "nan": np.full(n, np.nan, np.float32),
        "K-th dist": kth,
        "K-th dist + ulp": np.nextafter(kth, up),
        "K-th dist - ulp": np.nextafter(kth, down),
    }
    for what, d_max in cases.items():
        _both(sg, pts, K, dev, NE.nearest(pts, tri, K, d_max, d2=d2), "%s %s" % (name, what), d_max)
    for what in ("negative", "nan"):
        got = _query(sg, pts, K, dev, cases[what], True)
        assert (got[0] == -1).all() and np.all(np.isposinf(got[1])) and not got[2].any()
    at = NE.nearest(pts, tri, K, kth, d2=d2)[2]
    assert (at >= K).mean() > 0.5 and (NE.nearest(pts, tri, K, cases["K-th dist - ulp"], d2=d2)[2] < at).any()


def test_routes_agree(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    swept = hip.scene_create(*A.not_nested(bunny_small))               # the same triangles, created so that pruning is unavailable
    assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    d_max = np.random.default_rng(31).uniform(0.0, 0.4, pts.shape[0]).astype(np.float32)
    for k, dm, count in ((8, None, False), (8, d_max, True), (64, d_max, False)):
        a, b = _query(sg, pts, k, dev, dm, count), _query(swept, pts, k, dev, dm, count)
        _expect(a, b, "pruned against sweep")


def test_closest_point_at(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    K, n_tri = 4, tri.shape[0]
    p = _gpu(pts, dev)
    d_max = _gpu(np.random.default_rng(37).uniform(0.0, 0.2, pts.shape[0]), dev)            # rows with unused slots
    near = query.nearest(sg, p, K, d_max)
    at = query.closest_point_at(sg, p, near.tri)
    cp = query.closest_point(sg, p, d_max)
    torch.cuda.synchronize()
    assert isinstance(at, query.ClosestPoint) and at.tri is near.tri
    assert tuple(at.point.shape) == (pts.shape[0], K, 3) and tuple(at.dist.shape) == (pts.shape[0], K) and tuple(at.bary.shape) == (pts.shape[0], K, 2)
    assert (near.tri < 0).any() and (near.tri[:, K - 1] >= 0).any()
    assert _same(at.dist.cpu().numpy(), near.dist.cpu().numpy())                          # +inf in the unused slots too
    assert _same(at.point[:, 0].cpu().numpy(), cp.point.cpu().numpy()) and _same(at.bary[:, 0].cpu().numpy(), cp.bary.cpu().numpy())
    # against the definition, entry by entry
    ids = near.tri.cpu().numpy()
    for j in range(K):
        k = np.maximum(ids[:, j], 0)
        with np.errstate(all="ignore"):
            q, v, w, dd = (x[:, 0] for x in E.per_triangle(pts[:, None, :], *(tri[k, None, 3 * c:3 * c + 3] for c in range(3))))
        ok = (ids[:, j] >= 0) & np.isfinite(dd)
        assert _same(at.point[:, j].cpu().numpy(), np.where(ok[:, None], q, 0)) and _same(at.bary[:, j].cpu().numpy(), np.where(ok[:, None], np.stack([v, w], 1), 0))
        assert _same(at.dist[:, j].cpu().numpy(), np.where(ok, np.sqrt(np.where(ok, dd, 0)), np.inf))
    # the flat form; ids of -1 and n_tri, and a non-finite point, give (zeros, +inf, zeros)
    n = 257
    flat = np.arange(n, dtype=np.int32) * 13 % n_tri
    flat[::5] = -1
    flat[1::5] = n_tri
    last = pts.shape[0] - n                                              # the last points: finite ones and all the non-finite ones
    one = query.closest_point_at(sg, p[last:].contiguous(), _gpu(flat, dev, np.int32))
    torch.cuda.synchronize()
    out = (flat < 0) | (flat >= n_tri) | ~np.isfinite(pts[last:]).all(1) | (np.abs(pts[last:]) > 1e38).any(1)
    got = _host(one)
    assert out.sum() > 100 and (~out).sum() > 50
    assert not got[1][out].any() and not got[3][out].any() and np.all(np.isposinf(got[2][out])) and np.all(np.isfinite(got[2][~out]))
    with np.errstate(all="ignore"):
        q, v, w, dd = (x[:, 0] for x in E.per_triangle(pts[last:, None, :], *(tri[np.clip(flat, 0, n_tri - 1), None, 3 * c:3 * c + 3] for c in range(3))))
    assert _same(got[1][~out], q[~out]) and _same(got[2][~out], np.sqrt(dd[~out])) and _same(got[3][~out], np.stack([v, w], 1)[~out])
    # every combination of NULL outputs through the C entry point; what is not passed is not touched, all NULL is an error
    P = C.c_void_p
    ps, ids_d = p[last:].contiguous(), _gpu(flat, dev, np.int32)
    for use in itertools.product((False, True), repeat=3):
        bufs = [torch.full((n, 3), 7.0, device=dev), torch.full((n,), 7.0, device=dev), torch.full((n, 2), 7.0, device=dev)]
        args = [P(b.data_ptr()) if u else None for b, u in zip(bufs, use)]
        rc = hip.lib.ezrt_closest_point_at_device(sg._h, P(ps.data_ptr()), P(ids_d.data_ptr()), n, *args, None)
        torch.cuda.synchronize()
        assert rc == (0 if any(use) else EZRT_ERR_INVALID), use
        for b, u, w in zip(bufs, use, got[1:]):
            if u:
                assert _same(b.cpu().numpy(), w), use
            else:
                assert bool((b == 7.0).all()), use
    with pytest.raises(ValueError):
        query.closest_point_at(sg, p, near.tri[:10].contiguous())
    with pytest.raises(TypeError):
        query.closest_point_at(sg, p, near.tri.to(torch.int64))


def test_after_a_refit(hip, bunny_small, dev):
    tri, nodes = bunny_small.tri, bunny_small.nodes
    pts = E.points_for(tri, nodes, 321)[0][::3]
    ang = 0.4
    R = np.float32([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    moved = tri.copy()
    for k in range(6):                                                 # p1 p2 p3 n1 n2 n3
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] @ R.T
    moved[:, 1:9:3] += np.float32(0.1)
    d_max = np.full(pts.shape[0], 0.3, np.float32)
    sg = hip.scene_create(tri, nodes)
    first = _query(sg, pts, 8, dev, d_max, True)
    refit.refit(sg, moved)
    got = _query(sg, pts, 8, dev, d_max, True)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))
    assert sg.prune_info()["mode"] != -1 and fresh.prune_info()["mode"] != -1
    assert not np.array_equal(first[0], got[0])
    _expect(got, _query(fresh, pts, 8, dev, d_max, True), "after a refit")
    _expect(got, NE.nearest(pts, moved, 8, d_max), "after a refit, against the definition")
    _expect(_query(sg, pts, 8, dev), NE.nearest(pts, moved, 8), "after a refit, no d_max")


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("ties", hip, bunny_small)
    src = _gpu(pts, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                   # the points are written on `side`, behind the sleep
    a = query.nearest(sg, p, 5, stream=side)                           # issued from the default stream's context, onto `side`
    b = query.nearest(sg, p, 5, stream=side.cuda_stream)               # a raw handle
    c = query.closest_point_at(sg, p, a.tri, stream=side)              # the broadcast copy runs on `side` too
    d = query.closest_point_at(sg, p, b.tri, stream=side.cuda_stream)
    side.synchronize()
    _expect(_host(a), want, "side stream")
    _expect(_host(b), want, "raw handle")
    assert _same(c.dist.cpu().numpy(), want[1][:, :5]) and _same(d.dist.cpu().numpy(), want[1][:, :5])


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, _ = _case("bunny", hip, bunny_small)
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
    near = query.nearest(sg, p, 8, count=True)
    query.closest_point_at(sg, p, near.tri)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.nearest(sg, p, 8, count=True, stream=b)
    torch.cuda.synchronize()
    assert _same(frame.cpu().numpy(), alone.cpu().numpy())
    _expect(_host(got), want, "beside a render call")


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, pts, n_finite, d2, want, sg = _case("bunny", hip, bunny_small)
    lib = hip.lib
    n, K = 500, 4
    p = _gpu(pts[:n], dev)
    ids = torch.zeros((n, K), dtype=torch.int32, device=dev)
    d = torch.zeros((n, K), dtype=torch.float32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    host_pts = np.ascontiguousarray(pts[:n])
    host_ids = np.zeros((n, K), np.int32)
    host_f = np.zeros((n, K), np.float32)
    P = C.c_void_p
    f = lib.ezrt_query_nearest_device
    torch.cuda.synchronize()
    args = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("d_max"), kw.get("n", n), kw.get("k", K),
                         kw.get("tri", P(ids.data_ptr())), kw.get("dist", P(d.data_ptr())), kw.get("within", P(cnt.data_ptr())), None]
    assert f(*args()) == 0
    # host memory is rejected, never read or written
    assert f(*args(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*args(tri=P(host_ids.ctypes.data))) == EZRT_ERR_INVALID
    for name in ("d_max", "dist", "within"):
        assert f(*args(**{name: P(host_f.ctypes.data)})) == EZRT_ERR_INVALID
    assert not host_ids.any() and not host_f.any()
    # n < 0, NULL, max_k outside [1, 64]
    assert f(*args(n=-1)) == EZRT_ERR_INVALID
    for name in ("s", "pts", "tri", "dist"):
        assert f(*args(**{name: None})) == EZRT_ERR_INVALID, name
    assert f(*args(k=0)) == EZRT_ERR_INVALID and f(*args(k=65)) == EZRT_ERR_INVALID
    assert b"max_k" in lib.ezrt_last_error()
    assert f(*args(within=None)) == 0 and f(*args(n=0)) == 0
    # closest_point_at
    g = lib.ezrt_closest_point_at_device
    flat = torch.zeros(n, dtype=torch.int32, device=dev)
    q = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    gargs = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("tri", P(flat.data_ptr())), kw.get("n", n),
                          kw.get("point", P(q.data_ptr())), kw.get("dist"), kw.get("bary"), None]
    assert g(*gargs()) == 0
    assert g(*gargs(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID and g(*gargs(tri=P(host_ids.ctypes.data))) == EZRT_ERR_INVALID
    for name in ("point", "dist", "bary"):
        assert g(*gargs(**{name: P(host_f.ctypes.data)})) == EZRT_ERR_INVALID
    assert not host_f.any()
    assert g(*gargs(n=-1)) == EZRT_ERR_INVALID and g(*gargs(point=None)) == EZRT_ERR_INVALID
    for name in ("s", "pts", "tri"):
        assert g(*gargs(**{name: None})) == EZRT_ERR_INVALID, name
    assert g(*gargs(n=0)) == 0
    # the rejected calls left no HIP error behind: the next call works
    _expect(_query(sg, pts[:n], K, dev, count=True), tuple(x[:n] for x in want), "after the errors")
    # the wrapper
    with pytest.raises(TypeError):
        query.nearest(sg, torch.from_numpy(host_pts), K)
    with pytest.raises(TypeError):
        query.nearest(bunny_small.upload(oracle), p, K)
    with pytest.raises(ValueError):
        query.nearest(sg, p, K, d[:10, 0].contiguous())
    with pytest.raises(ValueError):
        query.nearest(sg, torch.zeros((4, 6), device=dev), K)
    for k in (0, 65, 4.0):
        with pytest.raises(ValueError):
            query.nearest(sg, p, k)
    e = query.nearest(sg, torch.empty((0, 3), device=dev), K, count=True)
    assert tuple(e.tri.shape) == (0, K) == tuple(e.dist.shape) and tuple(e.count.shape) == (0,)
    lead = query.nearest(sg, p.reshape(5, 100, 3), K, count=True)
    at = query.closest_point_at(sg, p.reshape(5, 100, 3), lead.tri)
    torch.cuda.synchronize()
    assert tuple(lead.tri.shape) == (5, 100, K) == tuple(lead.dist.shape) and tuple(lead.count.shape) == (5, 100)
    assert tuple(at.point.shape) == (5, 100, K, 3) and tuple(at.bary.shape) == (5, 100, K, 2)
    assert np.array_equal(lead.tri.cpu().numpy().reshape(-1, K), want[0][:n, :K])
    assert _same(at.dist.cpu().numpy().reshape(-1, K), want[1][:n, :K])

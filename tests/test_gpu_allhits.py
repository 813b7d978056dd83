"""All-hits queries on device tensors (include/ezrt_multihit.h, ezrt_amd/query.py: all_hits, surface_at), compared on the bits (a NaN
equal to a NaN) with tests/allhits_expected.py -- the definition restated on the CPU oracle's hitAABB / hitTriangle tables, pinned to
ezrt_query_hits by tests/test_allhits_expected.py:

* the full lists (max_hits = 64), their truncations (1, 2, 5) with the count unchanged, with and without t_hit / n_hits;
* t_max: random, at the 2nd hit's own t and one ulp either side of it, +inf, NaN, 0, negative;
* slot 0 == query.closest and count > 0 == query.occluded on the same device, with and without t_max;
* on the Bunny scene, 3-way exact ties, adversarial geometry (slivers, a coplanar grid, duplicates) and a scene the binary kernel
  traces, with camera rays, axis-parallel and one-zero-component rays, unnormalised rays and rays that are not tame;
* surface_at against query.surface; stream order, a render call beside it, untouched counters, refit, the errors of the contract.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_expected as E  # noqa: E402
import allhits_scenes as A  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
KMAX = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, oracle, bunny_small):
    """(tri, nodes, rays, visits, the device scene) of a named scene: the reference's visit lists are computed once and shared"""
    if name not in _cache:
        tri, nodes, rays = A.scene(name, bunny_small)
        _cache[name] = (tri, nodes, rays, E.visit_lists(oracle, tri, nodes, rays), hip.scene_create(tri, nodes))
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _all_hits(sg, rays, K, dev, t_max=None):
    tri, t, count = query.all_hits(sg, _gpu(rays, dev), K, None if t_max is None else _gpu(t_max, dev))
    torch.cuda.synchronize()
    assert tri.dtype == torch.int32 and t.dtype == torch.float32 and count.dtype == torch.int32
    assert tuple(tri.shape) == (rays.shape[0], K) == tuple(t.shape) and tuple(count.shape) == (rays.shape[0],)
    return tri.cpu().numpy(), t.cpu().numpy(), count.cpu().numpy()


def _expect(got, lists, K, what):
    wt, wd, wc = E.rows(lists, K)
    tri, t, count = got
    assert np.array_equal(count, wc), "%s: %d counts differ" % (what, int((count != wc).sum()))
    assert np.array_equal(tri, wt), "%s: %d rows differ" % (what, int((tri != wt).any(1).sum()))
    assert _same(t, wd), what


@pytest.mark.parametrize("name", A.SCENES)
def test_full_lists_and_truncations(hip, oracle, bunny_small, dev, name):
    tri, nodes, rays, visits, sg = _case(name, hip, oracle, bunny_small)
    if name == "not_nested":
        assert sg.prune_info()["records4"] == 0                        # the scene the binary kernel traces
    lists = E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits)
    count = np.array([ids.size for ids, t in lists])
    assert count.max() <= KMAX and (count > 0).mean() > 0.05
    if name == "ties":                                                 # what the checks below rest on, by the reference's values alone
        assert (count >= 2).mean() >= 0.25 and (count > 5).mean() >= 0.05 and (count == 0).mean() >= 0.05
        assert any(t.size > 2 and t[1] == t[2] for ids, t in lists)    # an exact tie straddling position K = 2
    for K in (KMAX, 1, 2, 5):
        _expect(_all_hits(sg, rays, K, dev), lists, K, "%s K=%d" % (name, K))
    # without t_hit and without n_hits (the C entry point): the same ids
    P = C.c_void_p
    r = _gpu(rays, dev)
    for K in (1, 2, 5, KMAX):
        out = torch.full((rays.shape[0], K), -7, dtype=torch.int32, device=dev)
        assert hip.lib.ezrt_query_all_hits_device(sg._h, P(r.data_ptr()), None, rays.shape[0], K, P(out.data_ptr()), None, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), E.rows(lists, K)[0]), "%s K=%d, no t_hit" % (name, K)


def _second_hit_t(lists):
    return np.array([t[1] if t.size > 1 else (t[0] if t.size else np.float32(1.0)) for ids, t in lists], np.float32)


@pytest.mark.parametrize("name", A.SCENES)
def test_t_max(hip, oracle, bunny_small, dev, name):
    tri, nodes, rays, visits, sg = _case(name, hip, oracle, bunny_small)
    n = rays.shape[0]
    rng = np.random.default_rng(9)
    t2 = _second_hit_t(E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits))
    cases = {
        "uniform": rng.uniform(0.0, 8.0, n).astype(np.float32),
        "2nd t": t2,
        "2nd t + ulp": np.nextafter(t2, np.float32(np.inf)),
        "2nd t - ulp": np.nextafter(t2, np.float32(-np.inf)),
        "+inf": np.full(n, np.inf, np.float32),
        "nan": np.full(n, np.nan, np.float32),
        "zero": np.zeros(n, np.float32),
        "negative": -rng.uniform(0.0, 3.0, n).astype(np.float32),
    }
    for what, t_max in cases.items():
        lists = E.expected_all_hits(oracle, tri, nodes, rays, t_max, visits=visits)
        for K in (KMAX, 2):
            _expect(_all_hits(sg, rays, K, dev, t_max), lists, K, "%s %s K=%d" % (name, what, K))
    assert not _all_hits(sg, rays, 2, dev, cases["nan"])[2].any() and not _all_hits(sg, rays, 2, dev, cases["zero"])[2].any()


@pytest.mark.parametrize("name", A.SCENES)
def test_slot_0_is_closest_and_count_is_occluded(hip, oracle, bunny_small, dev, name):
    tri, nodes, rays, visits, sg = _case(name, hip, oracle, bunny_small)
    rng = np.random.default_rng(10)
    r = _gpu(rays, dev)
    t2 = _second_hit_t(E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits))
    mixed = np.where(rng.random(rays.shape[0]) < 0.5, t2, rng.choice(np.float32([np.nan, 0.0, 0.0005, -1.0, np.inf, 2.0]), rays.shape[0]))
    for t_max in (None, _gpu(rng.uniform(0.0, 8.0, rays.shape[0]), dev), _gpu(mixed, dev)):
        ct, cd = query.closest(sg, r, t_max)
        occ = query.occluded(sg, r, t_max)
        for K in (1, 3):
            at, ad, ac = query.all_hits(sg, r, K, t_max)
            torch.cuda.synchronize()
            assert torch.equal(at[:, 0], ct)
            assert _same(ad[:, 0].cpu().numpy(), cd.cpu().numpy())
            assert torch.equal(ac > 0, occ)


def test_surface_at(hip, oracle, bunny_small, dev):
    tri, nodes, rays, visits, sg = _case("bunny", hip, oracle, bunny_small)
    r = _gpu(rays, dev)
    for integ in (4, 50):
        s = query.surface(sg, r, integrator=integ)
        assert 0.05 < float((s.tri < 0).float().mean()) < 0.95          # misses included: the zero rows
        p, nrm, ins = query.surface_at(sg, r, s.tri, s.t, integrator=integ)
        at, ad, ac = query.all_hits(sg, r, 4)
        p4, n4, i4 = query.surface_at(sg, r, at, ad, integrator=integ)  # the all-hits output passed straight in
        torch.cuda.synchronize()
        assert ins.dtype == torch.bool and tuple(p.shape) == (rays.shape[0], 3) and tuple(p4.shape) == (rays.shape[0], 4, 3)
        assert _same(p.cpu().numpy(), s.point.cpu().numpy()) and _same(nrm.cpu().numpy(), s.normal.cpu().numpy())
        assert torch.equal(ins, s.inside)
        assert _same(p4[:, 0].cpu().numpy(), s.point.cpu().numpy()) and _same(n4[:, 0].cpu().numpy(), s.normal.cpu().numpy())
        assert torch.equal(i4[:, 0], s.inside)
        # every layer: the attributes of that triangle at that distance, asked for one layer at a time
        for j in (1, 3):
            pj, nj, ij = query.surface_at(sg, r, at[:, j].contiguous(), ad[:, j].contiguous(), integrator=integ)
            torch.cuda.synchronize()
            assert _same(pj.cpu().numpy(), p4[:, j].cpu().numpy()) and _same(nj.cpu().numpy(), n4[:, j].cpu().numpy())
            assert torch.equal(ij, i4[:, j])
            empty = (at[:, j] < 0).cpu().numpy()
            assert empty.any() and (j > 1 or not empty.all())
            assert not p4[:, j].cpu().numpy()[empty].any() and not n4[:, j].cpu().numpy()[empty].any() and not i4[:, j].cpu().numpy()[empty].any()
    # ids that are no triangle of the scene: zeros
    n_tri = tri.shape[0]
    ids = torch.tensor([-1, n_tri, n_tri + 5, -2**31, 2**31 - 1, 0], dtype=torch.int32, device=dev)
    p, nrm, ins = query.surface_at(sg, r[:6].contiguous(), ids, torch.full((6,), 2.0, device=dev))
    torch.cuda.synchronize()
    assert not p[:5].any() and not nrm[:5].any() and not ins[:5].any() and bool(p[5].any())
    # optional outputs (the C entry point): one alone is written, the others are not touched
    P = C.c_void_p
    s = query.surface(sg, r)
    only = torch.zeros((rays.shape[0], 3), dtype=torch.float32, device=dev)
    assert hip.lib.ezrt_surface_at_device(sg._h, P(r.data_ptr()), P(s.tri.data_ptr()), P(s.t.data_ptr()), rays.shape[0], 50, None,
                                          P(only.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    assert _same(only.cpu().numpy(), s.normal.cpu().numpy())


def test_all_hits_is_ordered_on_its_stream(hip, oracle, bunny_small, dev):
    tri, nodes, rays, visits, sg = _case("ties", hip, oracle, bunny_small)
    lists = E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits)
    src = _gpu(rays, dev)
    r = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        r.copy_(src)                                                   # the rays are written on `side`, behind the sleep
    at, ad, ac = query.all_hits(sg, r, 5, stream=side)                 # issued from the default stream's context, onto `side`
    p, nrm, ins = query.surface_at(sg, r, at, ad, stream=side.cuda_stream)   # a raw handle
    side.synchronize()
    _expect((at.cpu().numpy(), ad.cpu().numpy(), ac.cpu().numpy()), lists, 5, "side stream")
    s = query.surface(sg, r)
    torch.cuda.synchronize()
    assert _same(p[:, 0].cpu().numpy(), s.point.cpu().numpy())


def test_all_hits_beside_a_render_call_and_untouched_state(hip, oracle, bunny_small, dev):
    tri, nodes, rays, visits, _ = _case("bunny", hip, oracle, bunny_small)
    lists = E.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    p = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    r = _gpu(rays, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(p, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    for K in (1, KMAX):
        query.all_hits(sg, r, K)
    query.surface_at(sg, r, *query.closest(sg, r))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(p, frame.data_ptr(), a.cuda_stream)
    got = query.all_hits(sg, r, 8, stream=b)
    torch.cuda.synchronize()
    assert _same(frame.cpu().numpy(), alone.cpu().numpy())
    _expect(tuple(x.cpu().numpy() for x in got), lists, 8, "beside a render call")


def test_all_hits_after_a_refit(hip, bunny_small, dev):
    tri, nodes = bunny_small.tri, bunny_small.nodes
    rays = A.rays_for(tri, 105, 2000)
    ang = 0.4
    R = np.float32([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    moved = tri.copy()
    for k in range(6):                                                 # p1 p2 p3 n1 n2 n3
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] @ R.T
    moved[:, 1:9:3] += np.float32(0.1)
    sg = hip.scene_create(tri, nodes)
    r = _gpu(rays, dev)
    first = query.all_hits(sg, r, 6)
    refit.refit(sg, moved)
    got = query.all_hits(sg, r, 6)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))
    want = query.all_hits(fresh, r, 6)
    torch.cuda.synchronize()
    assert not torch.equal(first[0], got[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and _same(got[1].cpu().numpy(), want[1].cpu().numpy())
    ps = query.surface_at(sg, r, got[0], got[1])
    pf = query.surface_at(fresh, r, want[0], want[1])
    torch.cuda.synchronize()
    assert _same(ps[1].cpu().numpy(), pf[1].cpu().numpy())


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, rays, visits, sg = _case("bunny", hip, oracle, bunny_small)
    lib = hip.lib
    n, K = 1000, 4
    r = _gpu(rays[:n], dev)
    out = torch.zeros((n, K), dtype=torch.int32, device=dev)
    t = torch.zeros((n, K), dtype=torch.float32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    host_rays = np.ascontiguousarray(rays[:n])
    host_out = np.zeros((n, K), np.int32)
    P = C.c_void_p
    f = lib.ezrt_query_all_hits_device
    torch.cuda.synchronize()
    args = lambda **kw: [kw.get("s", sg._h), kw.get("rays", P(r.data_ptr())), kw.get("t_max"), kw.get("n", n), kw.get("K", K),
                         kw.get("tri", P(out.data_ptr())), kw.get("t", P(t.data_ptr())), kw.get("cnt", P(cnt.data_ptr())), None]
    assert f(*args()) == 0
    # host memory is rejected, never read or written
    assert f(*args(rays=P(host_rays.ctypes.data))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*args(tri=P(host_out.ctypes.data))) == EZRT_ERR_INVALID
    assert f(*args(t_max=P(host_rays.ctypes.data))) == EZRT_ERR_INVALID
    assert f(*args(cnt=P(host_out.ctypes.data))) == EZRT_ERR_INVALID
    assert not host_out.any()
    # max_hits, n_rays, NULL
    for bad in (0, 65, -1):
        assert f(*args(K=bad)) == EZRT_ERR_INVALID
    assert f(*args(n=-1)) == EZRT_ERR_INVALID
    assert f(*args(s=None)) == EZRT_ERR_INVALID and f(*args(rays=None)) == EZRT_ERR_INVALID and f(*args(tri=None)) == EZRT_ERR_INVALID
    assert f(*args(n=0)) == 0
    g = lib.ezrt_surface_at_device
    pt = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    ids, tt = out[:, 0].contiguous(), t[:, 0].contiguous()
    assert g(sg._h, P(r.data_ptr()), P(ids.data_ptr()), P(tt.data_ptr()), n, 50, P(pt.data_ptr()), None, None, None) == 0
    assert g(sg._h, P(r.data_ptr()), P(ids.data_ptr()), P(tt.data_ptr()), n, 50, None, None, None, None) == EZRT_ERR_INVALID
    assert g(sg._h, P(r.data_ptr()), P(ids.data_ptr()), P(tt.data_ptr()), n, 7, P(pt.data_ptr()), None, None, None) == EZRT_ERR_INVALID
    assert g(sg._h, P(host_rays.ctypes.data), P(ids.data_ptr()), P(tt.data_ptr()), n, 50, P(pt.data_ptr()), None, None, None) == EZRT_ERR_INVALID
    assert g(sg._h, P(r.data_ptr()), None, P(tt.data_ptr()), n, 50, P(pt.data_ptr()), None, None, None) == EZRT_ERR_INVALID
    assert g(sg._h, P(r.data_ptr()), P(ids.data_ptr()), P(tt.data_ptr()), -1, 50, P(pt.data_ptr()), None, None, None) == EZRT_ERR_INVALID
    assert g(sg._h, P(r.data_ptr()), P(ids.data_ptr()), P(tt.data_ptr()), 0, 50, P(pt.data_ptr()), None, None, None) == 0
    # the rejected calls left no HIP error behind: the next call works
    lists = E.expected_all_hits(oracle, tri, nodes, rays[:n], None, visits=visits[:n])
    _expect(_all_hits(sg, rays[:n], K, dev), lists, K, "after the errors")
    # the wrapper
    with pytest.raises(ValueError):
        query.all_hits(sg, r, 0)
    with pytest.raises(ValueError):
        query.all_hits(sg, r, 65)
    with pytest.raises(TypeError):
        query.all_hits(sg, torch.from_numpy(host_rays), K)
    with pytest.raises(TypeError):
        query.all_hits(bunny_small.upload(oracle), r, K)
    with pytest.raises(ValueError):
        query.surface_at(sg, r, out[:, :2].contiguous().reshape(-1), t[:, :2].contiguous().reshape(-1))
    e = query.all_hits(sg, torch.empty((0, 6), device=dev), 3)
    assert tuple(e[0].shape) == (0, 3) and tuple(e[2].shape) == (0,)

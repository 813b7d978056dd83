"""Sphere-cast queries on device tensors (include/ezrt_sphere_cast.h, ezrt_amd/query.py: sphere_cast, sphere_cast_at).

Every output is compared on the bits with tests/sphere_cast_expected.py -- the header's rule restated in numpy over queries x ALL
triangles, pinned to true geometry by tests/test_sphere_cast_expected.py:

* about 2 000 queries (tests/sphere_cast_scenes.py) against the voxel solid, the Bunny scene and the adversarial scene, each on SAH
  trees with leaves of 4 and of 8, and the constructed pairs with known answers; in every batch at least 10 % swept contacts at
  t > 0, 10 % touching starts and 10 % misses, and face, edge and vertex each supply at least 5 % of the swept winners;
* every tree shape of tests/tree_shapes.py with about 260 queries, those aimed at the uncovered and at the duplicated triangles among
  them, the sweep routes among the shapes, and a scene after a refit;
* t_max per query with the one-ulp cases, NaN and negative values; queries that are not live, each clause once; n == 0, batches
  that are no multiple of 64 with guard words, NULL outputs, leading dimensions, a stream and a raw stream handle;
* sphere_cast_at on the winners and on [n, K] rows of nearest; touching against closest_point; the error contract of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import sphere_cast_expected as SE  # noqa: E402
import sphere_cast_scenes as SS  # noqa: E402
import tree_shapes as T  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
F = np.float32
TREES = [(name, leaf) for name in SS.NAMES for leaf in (4, 8)]
SHAPES = [(name, None) for name in T.HOST_SHAPES + T.LBVH_SHAPES if name != "chain"] + [("chain", 0), ("chain", 1)]
OUTPUTS = ("tri", "t", "point", "touching")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _table(name, bunny_small):
    """(tri, nodes, rays, radius, the restatement's swept table over all pairs) of the scene as it comes, computed once"""
    if name not in _cache:
        tri, nodes, rays, radius = SS.host_case(name, bunny_small)
        _cache[name] = (tri, nodes, rays, radius, SE.swept_all(rays, radius, tri))
    return _cache[name]


def _case(name, leaf, hip, bunny_small):
    """(tri, nodes, rays, radius, expected outputs, table, touch, device scene) on the SAH tree with leaves of `leaf`.  The builder
    reorders the triangles: the table's columns are permuted with them (identical triangles have identical columns) instead of being
    computed again; the touching step is asked again, its ties go by index."""
    key = (name, leaf)
    if key not in _cache:
        tri0, _, rays, radius, table = _table(name, bunny_small)
        tri, nodes = IS.build(tri0, leaf)
        where = {}
        for k in range(tri0.shape[0] - 1, -1, -1):
            where.setdefault(tri0[k, :9].tobytes(), []).append(k)
        perm = np.array([where[tri[k, :9].tobytes()].pop() for k in range(tri.shape[0])])
        assert np.array_equal(tri0[perm, :9].view(np.uint32), tri[:, :9].view(np.uint32)) and np.unique(perm).size == perm.size
        table = tuple(x[:, perm] for x in table)
        touch = SE.touch(rays, radius, tri, prune=True)
        _cache[key] = (tri, nodes, rays, radius, SE.query(rays, radius, tri, table=table, touching=touch), table, touch,
                       hip.scene_create(tri, nodes))
    return _cache[key]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _np(r):
    return r.tri.cpu().numpy(), r.t.cpu().numpy(), r.point.cpu().numpy(), r.touching.cpu().numpy().astype(np.uint8)


def _cast(sg, rays, radius, dev, t_max=None, **kw):
    r = query.sphere_cast(sg, _gpu(rays, dev), _gpu(radius, dev), None if t_max is None else _gpu(t_max, dev), **kw)
    torch.cuda.synchronize()
    lead = tuple(rays.shape[:-1])
    assert isinstance(r, query.SphereCast) and r.tri.dtype == torch.int32 and r.t.dtype == torch.float32 and r.touching.dtype == torch.bool
    assert tuple(r.tri.shape) == lead == tuple(r.t.shape) == tuple(r.touching.shape) and tuple(r.point.shape) == lead + (3,)
    return _np(r)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def differing(got, want, rays=None, names=OUTPUTS):
    """the outputs that differ on the bits, with the first query at which they do"""
    bad = []
    for name, a, b in zip(names, got, want):
        ne = _bits(a).reshape(len(b), -1) != _bits(b).reshape(len(b), -1)
        if a.shape != b.shape or ne.any():
            i = int(np.argmax(ne.any(1)))
            bad.append("%s: %d of %d rows, first at %d: %s, not %s%s" % (name, int(ne.any(1).sum()), len(b), i, a[i].tolist(), b[i].tolist(),
                                                                         "" if rays is None else " (ray %s)" % rays[i].tolist()))
    return bad


@pytest.mark.parametrize("name,leaf", TREES, ids=["%s-leaf%d" % t for t in TREES])
def test_outputs_on_the_bits(hip, bunny_small, dev, name, leaf):
    tri, nodes, rays, radius, want, table, touch, sg = _case(name, leaf, hip, bunny_small)
    assert sg.prune_info()["mode"] != -1                                # the walk
    assert SS.caps_met(want) and 1900 <= rays.shape[0] <= 2500, SS.caps(want)
    assert not differing(_cast(sg, rays, radius, dev), want[:4], rays)


def test_constructed_pairs(hip, dev):
    for leaf in (4, 8):
        tri, nodes, rays, radius, where = SS.constructed(leaf)
        got = _cast(hip.scene_create(tri, nodes), rays, radius, dev)
        assert not differing(got, SE.query(rays, radius, tri)[:4], rays)
        for i, (name, o, d, r, hit, tt, x, touch, s) in enumerate(SS.CASES):
            assert got[0][i] == (where[i] if hit else -1) and got[3][i] == touch, name
            assert np.array_equal(got[2][i], F(x) + F([SS.SPACING * i, 0, 0]) if hit else F([0, 0, 0])), name
            assert tt is None or got[1][i] == F(tt), name


@pytest.mark.parametrize("name,retree", SHAPES, ids=["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in SHAPES])
def test_tree_shapes(hip, dev, name, retree):
    tri, nodes, expect = T.shape(name)
    key = ("shape", name)
    if key not in _cache:
        rays, radius = SS.shape_queries(tri, expect, T.SEEDS[name])
        table, touch = SE.swept_all(rays, radius, tri), SE.touch(rays, radius, tri)
        want = SE.query(rays, radius, tri, table=table, touching=touch)
        t_max = np.where(np.arange(rays.shape[0]) % 2 == 0, want[1], F(np.inf)).astype(F)     # the winner's own t: boxes AT the radius
        _cache[key] = (rays, radius, t_max, want, SE.query(rays, radius, tri, t_max, table=table, touching=touch))
    rays, radius, t_max, want, want_t = _cache[key]
    if retree is None:
        sg = hip.scene_create(tri, nodes)
    else:
        os.environ["EZRT_RETREE"], old = str(retree), os.environ.get("EZRT_RETREE")     # read at scene creation
        try:
            sg = hip.scene_create(tri, nodes)
        finally:
            os.environ.pop("EZRT_RETREE") if old is None else os.environ.__setitem__("EZRT_RETREE", old)
    assert (sg.prune_info()["mode"] != -1 and sg.prune_info()["records4"] > 0) == expect["walk"]
    swept = (want[0] >= 0) & (want[3] == 0)
    assert swept.sum() >= rays.shape[0] // 4 and 180 <= rays.shape[0] <= 270
    if "uncovered" in expect:                                          # the sweep behind each walk finds them
        assert np.isin(want[0][swept], expect["uncovered"]).sum() >= 8
    assert np.array_equal(want_t[0][swept], want[0][swept])            # t_max = the answer's t keeps it
    assert not differing(_cast(sg, rays, radius, dev), want[:4], rays)
    assert not differing(_cast(sg, rays, radius, dev, t_max), want_t[:4], rays)


def test_after_a_refit(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, _ = _case("voxel_solid", 4, hip, bunny_small)
    moved = tri.copy()
    shift = F([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * F(2) + shift
    mr = rays[:600].copy()
    mr[:, :3] = mr[:, :3] * F(2) + shift
    mrad = radius[:600] * F(2)
    sg = hip.scene_create(tri, nodes)
    first = _cast(sg, mr, mrad, dev)
    refit.refit(sg, moved)
    assert sg.prune_info()["mode"] != -1
    got = _cast(sg, mr, mrad, dev)
    assert not differing(got, SE.query(mr, mrad, moved)[:4], mr)
    assert not np.array_equal(first[0], got[0]) and (got[0] >= 0).sum() > 300


def test_t_max(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("bunny", 8, hip, bunny_small)
    n = rays.shape[0]
    own = want[1]
    k = np.arange(n) % 6
    with np.errstate(all="ignore"):
        t_max = np.select([k == 0, k == 1, k == 2, k == 3, k == 4],
                          [own, np.nextafter(own, F(-np.inf)), np.nextafter(own, F(np.inf)), np.full(n, np.nan, F), np.full(n, -1.0, F)],
                          own * F(0.5)).astype(F)
    wt = SE.query(rays, radius, tri, t_max, table=table, touching=touch)
    swept = (want[0] >= 0) & (want[3] == 0) & (own > 0)
    assert np.array_equal(wt[0][swept & (k == 0)], want[0][swept & (k == 0)]) and np.array_equal(wt[0][swept & (k == 2)], want[0][swept & (k == 2)])
    assert (swept & (k == 1)).sum() > 50 and (wt[1][swept & (k == 1)] > own[swept & (k == 1)]).all()      # one ulp below: a later contact or none
    assert (wt[0][swept & ((k == 3) | (k == 4))] == -1).all() and (wt[0][swept & (k == 5)] == -1).all()
    assert np.array_equal(wt[0][want[3] == 1], want[0][want[3] == 1])                                     # touching does not look at t_max
    assert not differing(_cast(sg, rays, radius, dev, t_max), wt[:4], rays)


def test_queries_that_are_not_live(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("nasty", 4, hip, bunny_small)
    lo, hi = F([-1, -1, -1]), F([1, 1, 1])
    dr, dd = SS.dead_queries(lo, hi, np.random.default_rng(1))
    assert not SE.live(dr, dd).any() and dr.shape[0] == SS.N_DEAD
    got = _cast(sg, dr, dd, dev)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and not got[2].any() and not got[3].any()
    ok = dr.copy()                                                      # ... and each of them lives once the clause is mended
    ok[:, :3] = 0.0
    ok[:, 3:] = (0.0, -0.0, 1.0)
    assert SE.live(ok, np.full(SS.N_DEAD, 0.5, F)).all()
    at = query.sphere_cast_at(sg, _gpu(dr, dev), _gpu(dd, dev), torch.zeros(SS.N_DEAD, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert np.isposinf(at.t.cpu().numpy()).all() and not at.point.cpu().numpy().any() and not at.touching.cpu().numpy().any()


def test_batch_sizes_guard_words_null_outputs_and_shapes(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("voxel_solid", 8, hip, bunny_small)
    P = C.c_void_p
    lib = hip.lib
    GUARD = 0x5a5a5a5a
    for n in (1, 63, 65, 257):
        q, r = _gpu(rays[:n], dev), _gpu(radius[:n], dev)
        # nothing is written past row n - 1: guard words behind every buffer (a whole wave's worth of them)
        ids = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        tt = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        px = torch.full((3 * n + 192,), GUARD, dtype=torch.int32, device=dev)
        tc = torch.full((n + 64,), 0x5a, dtype=torch.uint8, device=dev)
        assert lib.ezrt_query_sphere_cast_device(sg._h, P(q.data_ptr()), P(r.data_ptr()), None, n, P(ids.data_ptr()), P(tt.data_ptr()),
                                                 P(px.data_ptr()), P(tc.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = (ids.cpu().numpy()[:n], tt.cpu().numpy()[:n].view(F), px.cpu().numpy()[:3 * n].view(F).reshape(n, 3), tc.cpu().numpy()[:n])
        assert not differing(got, tuple(x[:n] for x in want[:4])), n
        assert bool((ids[n:] == GUARD).all() and (tt[n:] == GUARD).all() and (px[3 * n:] == GUARD).all() and (tc[n:] == 0x5a).all()), n
        # every optional output NULL: tri_id alone
        ids.fill_(GUARD)
        assert lib.ezrt_query_sphere_cast_device(sg._h, P(q.data_ptr()), P(r.data_ptr()), None, n, P(ids.data_ptr()), None, None, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy()[:n], want[0][:n]) and bool((ids[n:] == GUARD).all())
        # the _at call on the winners, t alone and touching alone
        tt.fill_(GUARD)
        tc.fill_(0x5a)
        w = _gpu(want[0][:n], dev, np.int32)
        assert lib.ezrt_sphere_cast_at_device(sg._h, P(q.data_ptr()), P(r.data_ptr()), P(w.data_ptr()), n, P(tt.data_ptr()), None, None, None) == 0
        assert lib.ezrt_sphere_cast_at_device(sg._h, P(q.data_ptr()), P(r.data_ptr()), P(w.data_ptr()), n, None, None, P(tc.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(tt.cpu().numpy()[:n], want[1][:n].view(np.int32)) and bool((tt[n:] == GUARD).all())
        assert np.array_equal(tc.cpu().numpy()[:n], want[3][:n]) and bool((tc[n:] == 0x5a).all())
    got = _cast(sg, rays[:30].reshape(2, 3, 5, 6), radius[:30].reshape(2, 3, 5), dev)      # leading dimensions are kept
    assert not differing(tuple(x.reshape((30,) + x.shape[3:]) for x in got), tuple(x[:30] for x in want[:4]))
    at = query.sphere_cast_at(sg, _gpu(rays[:30].reshape(2, 3, 5, 6), dev), _gpu(radius[:30].reshape(2, 3, 5), dev),
                              _gpu(want[0][:30].reshape(2, 3, 5), dev, np.int32))
    torch.cuda.synchronize()
    assert tuple(at.t.shape) == (2, 3, 5) and tuple(at.point.shape) == (2, 3, 5, 3) and tuple(at.touching.shape) == (2, 3, 5)
    e = query.sphere_cast(sg, torch.empty((0, 6), device=dev), torch.empty((0,), device=dev))        # n == 0
    assert tuple(e.tri.shape) == (0,) and tuple(e.point.shape) == (0, 3) and e.touching.dtype == torch.bool
    e = query.sphere_cast_at(sg, torch.empty((0, 6), device=dev), torch.empty((0,), device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
    assert tuple(e.t.shape) == (0,) and tuple(e.point.shape) == (0, 3)


def test_streams(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("voxel_solid", 4, hip, bunny_small)
    src = _gpu(rays, dev)
    q = torch.zeros_like(src)
    r = _gpu(radius, dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        q.copy_(src)                                                   # the rays are written on `side`, behind the sleep
    a = query.sphere_cast(sg, q, r, stream=side)                       # issued from the default stream's context, onto `side`
    b = query.sphere_cast_at(sg, q, r, _gpu(want[0], dev, np.int32), stream=side.cuda_stream)   # a raw handle
    side.synchronize()
    assert not differing(_np(a), want[:4], rays)
    assert not differing(_np(b)[1:], want[1:4], rays, OUTPUTS[1:])


def test_at_reproduces_the_winners_and_takes_rows(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("nasty", 8, hip, bunny_small)
    n, m = rays.shape[0], tri.shape[0]
    q, r = _gpu(rays, dev), _gpu(radius, dev)
    got = query.sphere_cast(sg, q, r)
    at = query.sphere_cast_at(sg, q, r, got.tri)                       # the winners: the query's own outputs, misses included
    torch.cuda.synchronize()
    assert at.tri is got.tri and not differing(_np(got), want[:4], rays)
    # (a swept winner is not touching by closest_point's rule over the scene, so not by the pair's either: the same outputs)
    assert not differing(_np(at), _np(got), rays)
    # ids outside the scene, random pairs
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.resize(np.int32([m, -1, -2, 2 ** 31 - 1, -2 ** 31, m + 64]), n), rng.integers(0, m, n)]).astype(np.int32)
    qq, rr = np.tile(rays, (2, 1)), np.tile(radius, 2)
    at = query.sphere_cast_at(sg, _gpu(qq, dev), _gpu(rr, dev), _gpu(ids, dev, np.int32))
    torch.cuda.synchronize()
    w = SE.at(qq, rr, tri, ids)
    assert not differing(_np(at)[1:], w, qq, OUTPUTS[1:])
    assert np.isposinf(w[0][:n]).all() and np.isfinite(w[0][n:]).sum() > n // 20 and w[2][n:].sum() > 10
    # [n, K] rows of nearest (at the origin): every entry against its row's ray and radius
    near = query.nearest(sg, q[:500, :3].contiguous(), 3).tri
    at = query.sphere_cast_at(sg, q[:500], r[:500], near)
    torch.cuda.synchronize()
    assert tuple(at.t.shape) == (500, 3) and tuple(at.point.shape) == (500, 3, 3) and at.tri is near
    w = SE.at(np.repeat(rays[:500], 3, 0), np.repeat(radius[:500], 3), tri, near.cpu().numpy().reshape(-1))
    assert not differing(tuple(x.reshape((1500,) + x.shape[2:]) for x in _np(at)[1:]), w, names=OUTPUTS[1:])


def test_touching_is_closest_point(hip, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("bunny", 4, hip, bunny_small)
    alive = SE.live(rays, radius)
    q, r = _gpu(rays[alive], dev), _gpu(radius[alive], dev)
    got = query.sphere_cast(sg, q, r)
    cp = query.closest_point(sg, q[:, :3].contiguous(), r)
    torch.cuda.synchronize()
    m = got.touching.cpu().numpy()
    assert np.array_equal(m, cp.tri.cpu().numpy() >= 0) and m.sum() > 100 and not m.all()
    assert np.array_equal(got.tri.cpu().numpy()[m], cp.tri.cpu().numpy()[m])
    assert np.array_equal(got.point.cpu().numpy()[m].view(np.uint32), cp.point.cpu().numpy()[m].view(np.uint32))
    assert not got.t.cpu().numpy()[m].any()


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, rays, radius, want, table, touch, sg = _case("voxel_solid", 4, hip, bunny_small)
    lib = hip.lib
    n = 500
    q, r = _gpu(rays[:n], dev), _gpu(radius[:n], dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    tt = torch.zeros(n, dtype=torch.float32, device=dev)
    px = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    tc = torch.zeros(n, dtype=torch.uint8, device=dev)
    tm = torch.ones(n, dtype=torch.float32, device=dev)
    host_q = rays[:n].copy()
    host_f, host_i, host_3, host_b = np.zeros(n, F), np.zeros(n, np.int32), np.zeros((n, 3), F), np.zeros(n, np.uint8)
    P = C.c_void_p
    f, g = lib.ezrt_query_sphere_cast_device, lib.ezrt_sphere_cast_at_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("rays", P(q.data_ptr())), kw.get("radius", P(r.data_ptr())), kw.get("t_max", P(tm.data_ptr())),  # noqa: E731
                       kw.get("n", n), kw.get("tri", P(ids.data_ptr())), kw.get("t", P(tt.data_ptr())), kw.get("px", P(px.data_ptr())),
                       kw.get("tc", P(tc.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("rays", P(q.data_ptr())), kw.get("radius", P(r.data_ptr())), kw.get("tri", P(ids.data_ptr())),  # noqa: E731
                       kw.get("n", n), kw.get("t", P(tt.data_ptr())), kw.get("px", P(px.data_ptr())), kw.get("tc", P(tc.data_ptr())), None]
    err = lambda: lib.ezrt_last_error()  # noqa: E731
    assert f(*fa()) == 0 and g(*ga()) == 0
    torch.cuda.synchronize()
    before = [x.clone() for x in (ids, tt, px, tc)]
    for kw in (dict(s=None), dict(rays=None), dict(radius=None), dict(tri=None), dict(n=-1)):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    assert g(*ga(t=None, px=None, tc=None)) == EZRT_ERR_INVALID and b"one of t, point and touching" in err()
    # host memory is rejected, never read or written
    for kw in (dict(rays=P(host_q.ctypes.data)), dict(radius=P(host_f.ctypes.data)), dict(t_max=P(host_f.ctypes.data)),
               dict(tri=P(host_i.ctypes.data)), dict(t=P(host_f.ctypes.data)), dict(px=P(host_3.ctypes.data)), dict(tc=P(host_b.ctypes.data))):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
        if "t_max" not in kw:
            assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    assert not host_f.any() and not host_i.any() and not host_3.any() and not host_b.any()
    assert np.array_equal(host_q.view(np.uint32), rays[:n].view(np.uint32))
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0
    torch.cuda.synchronize()
    assert all(bool((a == b).all()) for a, b in zip(before, (ids, tt, px, tc)))   # no rejected call launched anything
    # the rejected calls left no HIP error behind: the next call works
    assert not differing(_cast(sg, rays[:n], radius[:n], dev), tuple(x[:n] for x in want[:4]))
    # the wrapper
    one = torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.sphere_cast(sg, torch.from_numpy(host_q), r)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.sphere_cast(sg, q, torch.from_numpy(host_f))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.sphere_cast_at(sg, q, r, torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError, match="HIP library"):
        query.sphere_cast(bunny_small.upload(oracle), q, r)
    with pytest.raises(TypeError, match="HIP library"):
        query.sphere_cast_at(bunny_small.upload(oracle), q, r, one)
    with pytest.raises(ValueError, match=r"must have shape \[\.\.\., 6\]"):
        query.sphere_cast(sg, torch.zeros((4, 9), device=dev), torch.zeros(4, device=dev))
    with pytest.raises(ValueError, match="radius must have shape"):
        query.sphere_cast(sg, q, torch.zeros(n + 1, device=dev))
    with pytest.raises(ValueError, match="t_max must have shape"):
        query.sphere_cast(sg, q, r, torch.zeros(n + 1, device=dev))
    with pytest.raises(TypeError, match="tri must be int32"):
        query.sphere_cast_at(sg, q, r, torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="tri must have shape"):
        query.sphere_cast_at(sg, q, r, torch.zeros(n + 1, dtype=torch.int32, device=dev))

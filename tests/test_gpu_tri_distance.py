"""Triangle-distance queries on device tensors (include/ezrt_tri_distance.h, ezrt_amd/query.py: tri_distance, tri_distance_at).

Every output is compared on the bits with tests/tri_distance_expected.py -- the header's rule restated in numpy over query triangles x
ALL triangles, pinned to true geometry by tests/test_tri_distance_expected.py:

* about 2 000 query triangles (tests/tri_distance_scenes.py: a second mesh that grazes, crosses and clears the scene, and
  tests/tri_overlap_scenes.py's) against the voxel solid, the Bunny scene and the adversarial scene, each on SAH trees with leaves of 4
  and of 8, and the constructed pairs with known answers;
* every tree shape of tests/tree_shapes.py with about 200 queries, the sweep routes among them, and a scene after a refit;
* d_max per query with the one-ulp cases, NaN and negative values; queries that are not live; n == 0, batches that are no multiple
  of 64 with guard words, NULL outputs, leading dimensions, a stream and a raw stream handle;
* tri_distance_at on the winners and on [n, K] rows of tri_overlap and nearest; consistency with tri_overlap and closest_point;
* the error contract of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import tree_shapes as T  # noqa: E402
import tri_distance_expected as TD  # noqa: E402
import tri_distance_scenes as DS  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
F = np.float32
TREES = [(name, leaf) for name in DS.NAMES for leaf in (4, 8)]
SHAPES = [(name, None) for name in T.HOST_SHAPES + T.LBVH_SHAPES if name != "chain"] + [("chain", 0), ("chain", 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _table(name, bunny_small):
    """(tri, nodes, q, the restatement's table over all pairs) of the scene as it comes, computed once"""
    if name not in _cache:
        tri, nodes, q = DS.host_case(name, bunny_small)
        _cache[name] = (tri, nodes, q, TD.dist2_all(q, tri, prune=True))
    return _cache[name]


def _case(name, leaf, hip, bunny_small):
    """(tri, nodes, q, expected outputs, device scene) on the SAH tree with leaves of `leaf`.  The builder reorders the triangles:
    the table's columns are permuted with them (identical triangles have identical columns) instead of being computed again."""
    key = (name, leaf)
    if key not in _cache:
        tri0, _, q, table = _table(name, bunny_small)
        tri, nodes = IS.build(tri0, leaf)
        where = {}
        for k in range(tri0.shape[0] - 1, -1, -1):
            where.setdefault(tri0[k, :9].tobytes(), []).append(k)
        perm = np.array([where[tri[k, :9].tobytes()].pop() for k in range(tri.shape[0])])
        assert np.array_equal(tri0[perm, :9].view(np.uint32), tri[:, :9].view(np.uint32)) and np.unique(perm).size == perm.size
        table = tuple(x[:, perm] for x in table)
        _cache[key] = (tri, nodes, q, TD.query(q, tri, table=table), table, hip.scene_create(tri, nodes))
    return _cache[key]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _np(r):
    return (r.tri.cpu().numpy(), r.dist.cpu().numpy(), r.point_query.cpu().numpy(), r.point_scene.cpu().numpy(),
            r.crosses.cpu().numpy().astype(np.uint8))


def _distance(sg, q, dev, d_max=None, **kw):
    r = query.tri_distance(sg, _gpu(q, dev), None if d_max is None else _gpu(d_max, dev), **kw)
    torch.cuda.synchronize()
    lead = tuple(q.shape[:-1])
    assert isinstance(r, query.TriDistance) and r.tri.dtype == torch.int32 and r.dist.dtype == torch.float32 and r.crosses.dtype == torch.bool
    assert tuple(r.tri.shape) == lead == tuple(r.dist.shape) == tuple(r.crosses.shape)
    assert tuple(r.point_query.shape) == lead + (3,) == tuple(r.point_scene.shape)
    return _np(r)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def differing(got, want, q=None):
    """the outputs that differ on the bits, with the first query at which they do"""
    bad = []
    for name, a, b in zip(("tri", "dist", "point_query", "point_scene", "crosses"), got, want):
        ne = _bits(a).reshape(len(b), -1) != _bits(b).reshape(len(b), -1)
        if a.shape != b.shape or ne.any():
            i = int(np.argmax(ne.any(1)))
            bad.append("%s: %d of %d rows, first at %d: %s, not %s%s" % (name, int(ne.any(1).sum()), len(b), i, a[i].tolist(), b[i].tolist(),
                                                                         "" if q is None else " (query %s)" % q[i].tolist()))
    return bad


def caps(want):
    """the comparison is not of misses: the share of queries that cross and the share at a positive finite distance are >= 10 % each"""
    tri, dist, _, _, crosses = want
    return bool(crosses.mean() >= 0.10 and ((dist > 0) & np.isfinite(dist)).mean() >= 0.10 and (tri < 0).any())


@pytest.mark.parametrize("name,leaf", TREES, ids=["%s-leaf%d" % t for t in TREES])
def test_outputs_on_the_bits(hip, bunny_small, dev, name, leaf):
    tri, nodes, q, want, table, sg = _case(name, leaf, hip, bunny_small)
    assert sg.prune_info()["mode"] != -1                                # the walk
    assert caps(want) and 1900 <= q.shape[0] <= 2100
    assert not differing(_distance(sg, q, dev), want, q)


def test_constructed_pairs(hip, dev):
    for leaf in (4, 8):
        tri, nodes, q, S, d2, crosses = DS.constructed(leaf)
        V = TE.vertices(tri)
        got = _distance(hip.scene_create(tri, nodes), q, dev)
        assert not differing(got, TD.query(q, tri), q)
        lowest = np.array([np.nonzero((V == S[i]).all((1, 2)))[0].min() for i in range(q.shape[0])])
        assert np.array_equal(got[0], lowest) and np.array_equal(got[1], np.sqrt(d2)) and np.array_equal(got[4], crosses)


@pytest.mark.parametrize("name,retree", SHAPES, ids=["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in SHAPES])
def test_tree_shapes(hip, dev, name, retree):
    tri, nodes, expect = T.shape(name)
    key = ("shape", name)
    if key not in _cache:
        q, first_tie = DS.shape_queries(tri, nodes, T.SEEDS[name])
        table = TD.dist2_all(q, tri)
        want = TD.query(q, tri, table=table)
        d_max = np.where(np.arange(q.shape[0]) % 2 == 0, want[1], F(np.inf)).astype(F)  # the winner's own distance: boxes AT the radius
        _cache[key] = (q, first_tie, d_max, want, TD.query(q, tri, d_max, table=table))
    q, first_tie, d_max, want, want_d = _cache[key]
    if retree is None:
        sg = hip.scene_create(tri, nodes)
    else:
        os.environ["EZRT_RETREE"], old = str(retree), os.environ.get("EZRT_RETREE")     # read at scene creation
        try:
            sg = hip.scene_create(tri, nodes)
        finally:
            os.environ.pop("EZRT_RETREE") if old is None else os.environ.__setitem__("EZRT_RETREE", old)
    assert (sg.prune_info()["mode"] != -1 and sg.prune_info()["records4"] > 0) == expect["walk"]
    assert (want[0] >= 0).sum() > q.shape[0] // 2
    if first_tie < q.shape[0]:                                         # the tie queries: found, at h exactly, with and without d_max
        assert (want[0][first_tie:] >= 0).all() and (want_d[0][first_tie::2] >= 0).all()
    assert not differing(_distance(sg, q, dev), want, q)
    assert not differing(_distance(sg, q, dev, d_max), want_d, q)


def test_after_a_refit(hip, bunny_small, dev):
    tri, nodes, q, want, table, _ = _case("voxel_solid", 4, hip, bunny_small)
    moved = tri.copy()
    shift = F([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * F(2) + shift
    mq = (q.reshape(-1, 3, 3) * F(2) + shift).reshape(-1, 9)[:600]
    sg = hip.scene_create(tri, nodes)
    first = _distance(sg, mq, dev)
    refit.refit(sg, moved)
    assert sg.prune_info()["mode"] != -1
    got = _distance(sg, mq, dev)
    assert not differing(got, TD.query(mq, moved), mq)
    assert not np.array_equal(first[0], got[0])


def test_d_max(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("bunny", 8, hip, bunny_small)
    n = q.shape[0]
    own = want[1]
    r = np.arange(n) % 6
    with np.errstate(all="ignore"):
        d_max = np.select([r == 0, r == 1, r == 2, r == 3, r == 4],
                          [own, np.nextafter(own, F(-np.inf)), np.nextafter(own, F(np.inf)), np.full(n, np.nan, F), np.full(n, -1.0, F)],
                          own * F(0.5)).astype(F)
    wd = TD.query(q, tri, d_max, table=table)
    hit = want[0] >= 0
    d2 = table[1][np.arange(n), np.maximum(want[0], 0)]
    keep = (r == 0) & hit & (own * own >= d2)                          # B = d_max * d_max is compared with dist2, not with dist
    assert np.array_equal(wd[0][keep], want[0][keep]) and (keep & (own > 0)).sum() > 20 and (wd[0][(r == 0) & hit & ~keep] < 0).all()
    pos = hit & (own > 0)
    assert (wd[0][(r == 1) & pos] != want[0][(r == 1) & pos]).any() and np.array_equal(wd[0][(r == 2) & hit], want[0][(r == 2) & hit])
    assert (wd[0][r == 3] < 0).all() and (wd[0][r == 4] < 0).all()
    assert not differing(_distance(sg, q, dev, d_max), wd, q)


def test_queries_that_are_not_live(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("nasty", 4, hip, bunny_small)
    dead = ~TE.live(q.reshape(-1, 3, 3))
    assert dead.sum() >= 20 and np.isnan(q[dead]).any() and np.isinf(q[dead]).any() and np.isfinite(q[dead]).all(1).any()
    got = _distance(sg, q[dead], dev)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all() and not got[2].any() and not got[3].any() and not got[4].any()


def test_batch_sizes_guard_words_null_outputs_and_shapes(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("voxel_solid", 8, hip, bunny_small)
    P = C.c_void_p
    lib = hip.lib
    GUARD = 0x5a5a5a5a
    for n in (1, 63, 65, 257):
        t = _gpu(q[:n], dev)
        # nothing is written past row n - 1: guard words behind every buffer (a whole wave's worth of them)
        ids = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        dist = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        px = torch.full((3 * n + 192,), GUARD, dtype=torch.int32, device=dev)
        py = torch.full((3 * n + 192,), GUARD, dtype=torch.int32, device=dev)
        cr = torch.full((n + 64,), 0x5a, dtype=torch.uint8, device=dev)
        assert lib.ezrt_query_tri_distance_device(sg._h, P(t.data_ptr()), None, n, P(ids.data_ptr()), P(dist.data_ptr()), P(px.data_ptr()),
                                                  P(py.data_ptr()), P(cr.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = (ids.cpu().numpy()[:n], dist.cpu().numpy()[:n].view(F), px.cpu().numpy()[:3 * n].view(F).reshape(n, 3),
               py.cpu().numpy()[:3 * n].view(F).reshape(n, 3), cr.cpu().numpy()[:n])
        assert not differing(got, tuple(x[:n] for x in want)), n
        assert bool((ids[n:] == GUARD).all() and (dist[n:] == GUARD).all() and (px[3 * n:] == GUARD).all() and (py[3 * n:] == GUARD).all()
                    and (cr[n:] == 0x5a).all()), n
        # every optional output NULL: tri_id alone
        ids.fill_(GUARD)
        assert lib.ezrt_query_tri_distance_device(sg._h, P(t.data_ptr()), None, n, P(ids.data_ptr()), None, None, None, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy()[:n], want[0][:n]) and bool((ids[n:] == GUARD).all())
        # the _at call on the winners, dist alone and crosses alone
        dist.fill_(GUARD)
        cr.fill_(0x5a)
        w = _gpu(want[0][:n], dev, np.int32)
        assert lib.ezrt_tri_distance_at_device(sg._h, P(t.data_ptr()), P(w.data_ptr()), n, P(dist.data_ptr()), None, None, None, None) == 0
        assert lib.ezrt_tri_distance_at_device(sg._h, P(t.data_ptr()), P(w.data_ptr()), n, None, None, None, P(cr.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dist.cpu().numpy()[:n], want[1][:n].view(np.int32)) and bool((dist[n:] == GUARD).all())
        assert np.array_equal(cr.cpu().numpy()[:n], want[4][:n]) and bool((cr[n:] == 0x5a).all())
    got = _distance(sg, q[:30].reshape(2, 3, 5, 9), dev)                # leading dimensions are kept
    assert not differing(tuple(x.reshape((30,) + x.shape[3:]) for x in got), tuple(x[:30] for x in want))
    at = query.tri_distance_at(sg, _gpu(q[:30].reshape(2, 3, 5, 9), dev), _gpu(want[0][:30].reshape(2, 3, 5), dev, np.int32))
    torch.cuda.synchronize()
    assert tuple(at.dist.shape) == (2, 3, 5) and tuple(at.point_scene.shape) == (2, 3, 5, 3)
    e = query.tri_distance(sg, torch.empty((0, 9), device=dev))        # n == 0
    assert tuple(e.tri.shape) == (0,) and tuple(e.point_query.shape) == (0, 3) and e.crosses.dtype == torch.bool
    e = query.tri_distance_at(sg, torch.empty((0, 9), device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
    assert tuple(e.dist.shape) == (0,) and tuple(e.point_scene.shape) == (0, 3)


def test_streams(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("voxel_solid", 4, hip, bunny_small)
    src = _gpu(q, dev)
    t = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        t.copy_(src)                                                   # the triangles are written on `side`, behind the sleep
    a = query.tri_distance(sg, t, stream=side)                         # issued from the default stream's context, onto `side`
    b = query.tri_distance_at(sg, t, _gpu(want[0], dev, np.int32), stream=side.cuda_stream)   # a raw handle
    side.synchronize()
    assert not differing(_np(a), want, q)
    assert not differing(_np(b)[1:], want[1:], q)


def test_at_reproduces_the_winners_and_takes_rows(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("nasty", 8, hip, bunny_small)
    n, m = q.shape[0], tri.shape[0]
    t = _gpu(q, dev)
    got = query.tri_distance(sg, t)
    at = query.tri_distance_at(sg, t, got.tri)                         # the winners: the query's own outputs, misses included
    torch.cuda.synchronize()
    assert at.tri is got.tri and not differing(_np(at), _np(got), q) and not differing(_np(got), want, q)
    # ids outside the scene, random pairs
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.resize(np.int32([m, -1, -2, 2 ** 31 - 1, -2 ** 31, m + 64]), n), rng.integers(0, m, n)]).astype(np.int32)
    qq = np.tile(q, (2, 1))
    at = query.tri_distance_at(sg, _gpu(qq, dev), _gpu(ids, dev, np.int32))
    torch.cuda.synchronize()
    w = TD.at(qq, tri, ids)
    assert not differing(_np(at)[1:], w, qq)
    assert np.isposinf(w[0][:n]).all() and np.isfinite(w[0][n:]).sum() > n // 2
    # [n, K] rows of tri_overlap and of nearest (at the first vertex): every entry against its row's query triangle
    rows = query.tri_overlap(sg, t[:500], 4).tri
    near = query.nearest(sg, t[:500, :3].contiguous(), 3).tri
    for block in (rows, near):
        k = block.shape[1]
        at = query.tri_distance_at(sg, t[:500], block)
        torch.cuda.synchronize()
        assert tuple(at.dist.shape) == (500, k) and tuple(at.point_query.shape) == (500, k, 3)
        w = TD.at(np.repeat(q[:500], k, 0), tri, block.cpu().numpy().reshape(-1))
        assert not differing(tuple(x.reshape((500 * k,) + x.shape[2:]) for x in _np(at)[1:]), w)
    crossing = query.tri_distance_at(sg, t[:500], rows)                # a listed overlap crosses, an unused slot misses
    torch.cuda.synchronize()
    listed = rows.cpu().numpy() >= 0
    assert np.array_equal(crossing.crosses.cpu().numpy(), listed) and listed.any() and not listed.all()
    assert not crossing.dist.cpu().numpy()[listed].any() and np.isposinf(crossing.dist.cpu().numpy()[~listed]).all()


def test_consistent_with_tri_overlap_and_closest_point(hip, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("bunny", 4, hip, bunny_small)
    t = _gpu(q, dev)
    got = query.tri_distance(sg, t)
    over = query.tri_overlap(sg, t, 1, count=True)
    cp = [query.closest_point(sg, t[:, 3 * v:3 * v + 3].contiguous()) for v in range(3)]
    torch.cuda.synchronize()
    tri_id, dist, _, _, crosses = _np(got)
    n_over, first = over.n_overlap.cpu().numpy(), over.tri.cpu().numpy()[:, 0]
    assert np.array_equal(crosses == 1, n_over > 0) and crosses.any() and not crosses.all()
    assert np.array_equal(tri_id[crosses == 1], first[crosses == 1])   # all at dist2 = 0: the lowest index, which is the row's first
    # the vertex sub-candidates ARE closest_point's function: no vertex of a live query is nearer to the mesh than the triangle
    live = TE.live(q.reshape(-1, 3, 3))
    vertex = np.min([c.dist.cpu().numpy() for c in cp], axis=0)
    assert (dist[live] <= vertex[live]).all() and (dist[live] < vertex[live]).any()
    at_vertex = live & (crosses == 0) & (dist == vertex)
    assert at_vertex.sum() > 50                                         # ... and where a vertex is the nearest feature, on the bits


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, q, want, table, sg = _case("voxel_solid", 4, hip, bunny_small)
    lib = hip.lib
    n = 500
    live_q = q[TE.live(q.reshape(-1, 3, 3))][:n]
    t = _gpu(live_q, dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    dist = torch.zeros(n, dtype=torch.float32, device=dev)
    px, py = torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev)
    cr = torch.zeros(n, dtype=torch.uint8, device=dev)
    dm = torch.ones(n, dtype=torch.float32, device=dev)
    host_f, host_i, host_3, host_b = live_q.copy(), np.zeros(n, np.int32), np.zeros((n, 3), F), np.zeros(n, np.uint8)
    P = C.c_void_p
    f, g = lib.ezrt_query_tri_distance_device, lib.ezrt_tri_distance_at_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("tris", P(t.data_ptr())), kw.get("d_max", P(dm.data_ptr())), kw.get("n", n),
                       kw.get("tri", P(ids.data_ptr())), kw.get("dist", P(dist.data_ptr())), kw.get("px", P(px.data_ptr())),
                       kw.get("py", P(py.data_ptr())), kw.get("cr", P(cr.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("tris", P(t.data_ptr())), kw.get("tri", P(ids.data_ptr())), kw.get("n", n),
                       kw.get("dist", P(dist.data_ptr())), kw.get("px", P(px.data_ptr())), kw.get("py", P(py.data_ptr())),
                       kw.get("cr", P(cr.data_ptr())), None]
    err = lambda: lib.ezrt_last_error()
    assert f(*fa()) == 0 and g(*ga()) == 0
    torch.cuda.synchronize()
    before = [x.clone() for x in (ids, dist, px, py, cr)]
    for kw in (dict(s=None), dict(tris=None), dict(tri=None), dict(n=-1)):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    assert g(*ga(dist=None, px=None, py=None, cr=None)) == EZRT_ERR_INVALID and b"one of dist, point_query, point_scene and crosses" in err()
    # host memory is rejected, never read or written
    for kw in (dict(tris=P(host_f.ctypes.data)), dict(d_max=P(host_f.ctypes.data)), dict(tri=P(host_i.ctypes.data)),
               dict(dist=P(host_f.ctypes.data)), dict(px=P(host_3.ctypes.data)), dict(py=P(host_3.ctypes.data)), dict(cr=P(host_b.ctypes.data))):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
        if "d_max" not in kw:
            assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    assert not host_i.any() and not host_3.any() and not host_b.any() and np.array_equal(host_f.view(np.uint32), live_q.view(np.uint32))
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0
    torch.cuda.synchronize()
    assert all(bool((a == b).all()) for a, b in zip(before, (ids, dist, px, py, cr)))   # no rejected call launched anything
    # the rejected calls left no HIP error behind: the next call works
    assert not differing(_distance(sg, q[:n], dev), tuple(x[:n] for x in want))
    # the wrapper
    one = torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_distance(sg, torch.from_numpy(host_f))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.tri_distance_at(sg, t, torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError, match="HIP library"):
        query.tri_distance(bunny_small.upload(oracle), t)
    with pytest.raises(TypeError, match="HIP library"):
        query.tri_distance_at(bunny_small.upload(oracle), t, one)
    with pytest.raises(ValueError, match=r"must have shape \[\.\.\., 9\]"):
        query.tri_distance(sg, torch.zeros((4, 6), device=dev))
    with pytest.raises(ValueError, match="d_max must have shape"):
        query.tri_distance(sg, t, torch.zeros(n + 1, device=dev))
    with pytest.raises(TypeError, match="tri must be int32"):
        query.tri_distance_at(sg, t, torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="tri must have shape"):
        query.tri_distance_at(sg, t, torch.zeros(n + 1, dtype=torch.int32, device=dev))

"""Segment queries on device tensors (include/ezrt_segment.h, ezrt_amd/query.py: segment_distance, segment_distance_at,
capsule_overlap).

Every output is compared on the bits with tests/segment_expected.py -- the header's rule restated in numpy over segments x ALL
triangles, pinned to true geometry by tests/test_segment_expected.py:

* about 2 000 segments, d_max and radii (tests/segment_scenes.py: segments that graze, pierce and clear the mesh, along its edges, in
  and parallel to its faces, of zero length, of 0.1 to 10 leaf sizes, not live) against the voxel solid, the Bunny scene and the
  adversarial scene, each on SAH trees with leaves of 4 and of 8, for all three calls, with the caps asserted; the constructed pairs;
* every tree shape of tests/tree_shapes.py with about 200 queries, the sweep routes among them, with and without d_max / radius at the
  winner's own distance, and a scene after a refit;
* d_max and radius one ulp either side, 0, NaN, negative, +inf; each liveness clause; max_k of 0, 1, 8 and 64 and 65 rejected;
* n == 0, batches that are no multiple of 64 with guard words, NULL outputs, leading dimensions, a stream and a raw stream handle;
* segment_distance_at on the winners, on [n, K] rows of capsule_overlap and nearest, and with bad ids;
* the consequences the header states between the calls; the error contract of the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import segment_expected as SX  # noqa: E402
import segment_scenes as SS  # noqa: E402
import tree_shapes as T  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
F = np.float32
TREES = [(name, leaf) for name in SS.NAMES for leaf in (4, 8)]
SHAPES = [(name, None) for name in T.HOST_SHAPES + T.LBVH_SHAPES if name != "chain"] + [("chain", 0), ("chain", 1)]
NAMES5 = ("tri", "dist", "point_query", "point_scene", "crosses")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _table(name, bunny_small):
    """(tri, nodes, segs, d_max, radius, the restatement's table over all pairs) of the scene as it comes, computed once"""
    if name not in _cache:
        tri, nodes, segs, d_max, radius = SS.host_case(name, bunny_small)
        _cache[name] = (tri, nodes, segs, d_max, radius, SX.dist2_all(segs, tri, prune=True, reach=np.maximum(d_max, radius)))
    return _cache[name]


class Case:
    pass


def _case(name, leaf, hip, bunny_small):
    """the scene on the SAH tree with leaves of `leaf`, its queries, the expected outputs of the three calls and the device scene.
    The builder reorders the triangles: the table's columns are permuted with them instead of being computed again."""
    key = (name, leaf)
    if key not in _cache:
        tri0, _, segs, d_max, radius, table = _table(name, bunny_small)
        tri, nodes = IS.build(tri0, leaf)
        where = {}
        for k in range(tri0.shape[0] - 1, -1, -1):
            where.setdefault(tri0[k, :9].tobytes(), []).append(k)
        perm = np.array([where[tri[k, :9].tobytes()].pop() for k in range(tri.shape[0])])
        assert np.array_equal(tri0[perm, :9].view(np.uint32), tri[:, :9].view(np.uint32)) and np.unique(perm).size == perm.size
        c = Case()
        c.tri, c.nodes, c.segs, c.d_max, c.radius = tri, nodes, segs, d_max, radius
        c.table = tuple(x[:, perm] for x in table)
        c.free = SX.query(segs, tri, None, c.table)
        c.limited = SX.query(segs, tri, d_max, c.table)
        c.capsule = SX.capsule(segs, radius, tri, SS.MAX_K, c.table)
        c.sg = hip.scene_create(tri, nodes)
        _cache[key] = c
    return _cache[key]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _np(r):
    return (r.tri.cpu().numpy(), r.dist.cpu().numpy(), r.point_query.cpu().numpy(), r.point_scene.cpu().numpy(),
            r.crosses.cpu().numpy().astype(np.uint8))


def _distance(sg, segs, dev, d_max=None, **kw):
    r = query.segment_distance(sg, _gpu(segs, dev), None if d_max is None else _gpu(d_max, dev), **kw)
    torch.cuda.synchronize()
    lead = tuple(segs.shape[:-1])
    assert isinstance(r, query.SegmentDistance) and r.tri.dtype == torch.int32 and r.dist.dtype == torch.float32 and r.crosses.dtype == torch.bool
    assert tuple(r.tri.shape) == lead == tuple(r.dist.shape) == tuple(r.crosses.shape)
    assert tuple(r.point_query.shape) == lead + (3,) == tuple(r.point_scene.shape)
    return _np(r)


def _capsule(sg, segs, radius, dev, k, count=True, **kw):
    r = query.capsule_overlap(sg, _gpu(segs, dev), _gpu(radius, dev), k, count=count, **kw)
    torch.cuda.synchronize()
    lead = tuple(segs.shape[:-1])
    assert isinstance(r, query.CapsuleOverlap) and r.tri.dtype == torch.int32 and tuple(r.tri.shape) == lead + (k,)
    if not count:
        assert r.n_overlap is None
        return r.tri.cpu().numpy(), None
    assert r.n_overlap.dtype == torch.int32 and tuple(r.n_overlap.shape) == lead
    return r.tri.cpu().numpy(), r.n_overlap.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def differing(got, want, q=None, names=NAMES5):
    """the outputs that differ on the bits, with the first query at which they do"""
    bad = []
    for name, a, b in zip(names, got, want):
        ne = _bits(a).reshape(len(b), -1) != _bits(b).reshape(len(b), -1)
        if a.shape != b.shape or ne.any():
            i = int(np.argmax(ne.any(1)))
            bad.append("%s: %d of %d rows, first at %d: %s, not %s%s" % (name, int(ne.any(1).sum()), len(b), i, a[i].tolist(), b[i].tolist(),
                                                                         "" if q is None else " (query %s)" % q[i].tolist()))
    return bad


def rows_differ(got, want, q=None):
    return differing(got, want, q, ("rows", "count"))


@pytest.mark.parametrize("name,leaf", TREES, ids=["%s-leaf%d" % t for t in TREES])
def test_outputs_on_the_bits(hip, bunny_small, dev, name, leaf):
    c = _case(name, leaf, hip, bunny_small)
    assert c.sg.prune_info()["mode"] != -1                              # the walk
    caps = SS.caps(c.segs, c.free, c.limited, c.capsule[1])
    assert SS.caps_met(caps) and 1900 <= c.segs.shape[0] <= 2300, caps
    assert not differing(_distance(c.sg, c.segs, dev), c.free[:5], c.segs)
    assert not differing(_distance(c.sg, c.segs, dev, c.d_max), c.limited[:5], c.segs)
    assert not rows_differ(_capsule(c.sg, c.segs, c.radius, dev, SS.MAX_K), c.capsule, c.segs)
    at = query.segment_distance_at(c.sg, _gpu(c.segs, dev), _gpu(c.free[0], dev, np.int32))
    torch.cuda.synchronize()
    assert not differing(_np(at)[1:], c.free[1:5], c.segs, NAMES5[1:])


def test_constructed_pairs(hip, dev):
    for leaf in (4, 8):
        tri, nodes, segs, where = SS.constructed(leaf)
        sg = hip.scene_create(tri, nodes)
        got = _distance(sg, segs, dev)
        assert not differing(got, SX.query(segs, tri)[:5], segs)
        assert np.array_equal(got[0], where) and np.array_equal(got[1], np.sqrt(F([c[3] for c in SS.CASES])))
        assert np.array_equal(got[4], np.uint8([c[4] for c in SS.CASES]))
        for radius in (got[1], np.nextafter(got[1], F(-np.inf)), np.nextafter(got[1], F(np.inf))):
            assert not rows_differ(_capsule(sg, segs, radius, dev, 4), SX.capsule(segs, radius, tri, 4), segs)


@pytest.mark.parametrize("name,retree", SHAPES, ids=["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in SHAPES])
def test_tree_shapes(hip, dev, name, retree):
    tri, nodes, expect = T.shape(name)
    key = ("shape", name)
    if key not in _cache:
        segs, d_max, radius = SS.shape_queries(tri, expect, T.SEEDS[name])
        table = SX.dist2_all(segs, tri)
        want = SX.query(segs, tri, None, table)
        even = np.arange(segs.shape[0]) % 2 == 0                        # the winner's own distance: boxes AT the radius
        d_max = np.where(even, want[1], d_max).astype(F)
        radius = np.where(even & np.isfinite(want[1]), want[1], radius).astype(F)
        _cache[key] = (segs, d_max, radius, want, SX.query(segs, tri, d_max, table), SX.capsule(segs, radius, tri, 8, table))
    segs, d_max, radius, want, want_d, want_c = _cache[key]
    if retree is None:
        sg = hip.scene_create(tri, nodes)
    else:
        os.environ["EZRT_RETREE"], old = str(retree), os.environ.get("EZRT_RETREE")     # read at scene creation
        try:
            sg = hip.scene_create(tri, nodes)
        finally:
            os.environ.pop("EZRT_RETREE") if old is None else os.environ.__setitem__("EZRT_RETREE", old)
    assert (sg.prune_info()["mode"] != -1 and sg.prune_info()["records4"] > 0) == expect["walk"]
    assert (want[0] >= 0).sum() > segs.shape[0] // 2 and (want_c[1] > 0).sum() > segs.shape[0] // 4
    assert not differing(_distance(sg, segs, dev), want[:5], segs)
    assert not differing(_distance(sg, segs, dev, d_max), want_d[:5], segs)
    assert not rows_differ(_capsule(sg, segs, radius, dev, 8), want_c, segs)


def test_after_a_refit(hip, bunny_small, dev):
    c = _case("voxel_solid", 4, hip, bunny_small)
    moved = c.tri.copy()
    shift = F([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * F(2) + shift
    ms = (c.segs.reshape(-1, 2, 3) * F(2) + shift).reshape(-1, 6)[:600]
    mr = c.radius[:600] * F(2)
    sg = hip.scene_create(c.tri, c.nodes)
    first = _distance(sg, ms, dev)
    refit.refit(sg, moved)
    assert sg.prune_info()["mode"] != -1
    table = SX.dist2_all(ms, moved)
    got = _distance(sg, ms, dev)
    assert not differing(got, SX.query(ms, moved, None, table)[:5], ms)
    assert not rows_differ(_capsule(sg, ms, mr, dev, 8), SX.capsule(ms, mr, moved, 8, table), ms)
    assert not np.array_equal(first[0], got[0])


def test_d_max_and_radius(hip, bunny_small, dev):
    c = _case("bunny", 8, hip, bunny_small)
    segs, tri, table, want = c.segs, c.tri, c.table, c.free
    n = segs.shape[0]
    own = want[1]
    r = np.arange(n) % 8
    with np.errstate(all="ignore"):
        cut = np.select([r == 0, r == 1, r == 2, r == 3, r == 4, r == 5, r == 6],
                        [own, np.nextafter(own, F(-np.inf)), np.nextafter(own, F(np.inf)), np.full(n, np.nan, F), np.full(n, -1.0, F),
                         np.zeros(n, F), np.full(n, np.inf, F)], own * F(0.5)).astype(F)
    wd = SX.query(segs, tri, cut, table)
    hit = want[0] >= 0
    d2 = table[1][np.arange(n), np.maximum(want[0], 0)]
    keep = (r == 0) & hit & (own * own >= d2)                          # B = d_max * d_max is compared with dist2, not with dist
    assert np.array_equal(wd[0][keep], want[0][keep]) and (keep & (own > 0)).sum() > 20 and (wd[0][(r == 0) & hit & ~keep] < 0).all()
    pos = hit & (own > 0)
    assert (wd[0][(r == 1) & pos] != want[0][(r == 1) & pos]).any() and np.array_equal(wd[0][(r == 2) & hit], want[0][(r == 2) & hit])
    assert (wd[0][r == 3] < 0).all() and (wd[0][r == 4] < 0).all() and np.array_equal(wd[0][r == 6], want[0][r == 6])
    assert np.array_equal(wd[0][r == 5] >= 0, (own == 0)[r == 5]) and (wd[0][r == 5] >= 0).any()
    assert not differing(_distance(c.sg, segs, dev, cut), wd[:5], segs)
    # the same cuts as radii: NaN, negative and +inf are not live; 0 lists what is crossed or rounds to 0
    wc = SX.capsule(segs, cut, tri, 8, table)
    assert not wc[1][(r == 3) | (r == 4) | (r == 6)].any() and np.array_equal(wc[1][r == 5] > 0, (own == 0)[r == 5])
    same = r != 6                                                      # (+inf is a d_max, not a radius)
    assert np.array_equal((wc[1] > 0)[same], (wd[0] >= 0)[same])
    assert not rows_differ(_capsule(c.sg, segs, cut, dev, 8), wc, segs)
    huge = np.full(64, 3e19, F)                                        # R2 = +inf admits every candidate
    got = _capsule(c.sg, segs[:64], huge, dev, 8)
    assert not rows_differ(got, SX.capsule(segs[:64], huge, tri, 8), segs[:64]) and got[1].max() == TE.live(TE.vertices(tri)).sum()


def test_each_liveness_clause(hip, bunny_small, dev):
    c = _case("nasty", 4, hip, bunny_small)
    base = c.segs[SX.live(c.segs)][:16].copy()
    radius = np.full(16, 10.0, F)
    dead = base.copy()
    for i, (j, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf))):
        dead[i, j] = v
    radius[6], radius[7], radius[8] = np.nan, np.inf, -1.0             # the capsule's own clauses
    radius[9], radius[10] = -0.0, 0.0                                   # ... -0 is >= 0: live, and R2 = 0 as for +0
    dead[10] = dead[9]
    got = _distance(c.sg, dead, dev)
    assert (got[0][:6] == -1).all() and np.isposinf(got[1][:6]).all() and not got[2][:6].any() and not got[3][:6].any() and not got[4][:6].any()
    assert (got[0][6:] >= 0).all() and not differing(got, SX.query(dead, c.tri)[:5], dead)
    rows, count = _capsule(c.sg, dead, radius, dev, 4)
    assert not count[:9].any() and (rows[:9] == -1).all() and count[9] == count[10] and (count[11:] > 0).all()
    assert not rows_differ((rows, count), SX.capsule(dead, radius, c.tri, 4), dead)
    at = query.segment_distance_at(c.sg, _gpu(dead, dev), _gpu(np.zeros(16), dev, np.int32))
    torch.cuda.synchronize()
    assert np.isposinf(at.dist.cpu().numpy()[:6]).all() and not at.crosses.cpu().numpy()[:6].any()
    # a scene triangle that is not live is never found: the constructed scene with two of its triangles made degenerate
    tri, nodes, segs, where = SS.constructed(4)
    bad = tri.copy()
    bad[where[0], 3:6] = bad[where[0], 0:3]                            # a repeated vertex
    bad[where[4], 6:9] = bad[where[4], 0:3] + (bad[where[4], 3:6] - bad[where[4], 0:3]) * F(0.5)   # collinear
    assert not TE.live(TE.vertices(bad))[[where[0], where[4]]].any()
    sg = hip.scene_create(bad, nodes)
    want = SX.query(segs, bad)
    got = _distance(sg, segs, dev)
    assert not differing(got, want[:5], segs) and got[0][0] != where[0] and got[0][4] != where[4] and (got[0] >= 0).all()
    rad = np.full(segs.shape[0], 1000.0, F)
    rows, count = _capsule(sg, segs, rad, dev, 64)
    assert not rows_differ((rows, count), SX.capsule(segs, rad, bad, 64), segs) and not np.isin(rows, [where[0], where[4]]).any()
    at = query.segment_distance_at(sg, _gpu(segs, dev), _gpu(where, dev, np.int32))
    torch.cuda.synchronize()
    assert not differing(_np(at)[1:], SX.at(segs, bad, where)[:4], segs, NAMES5[1:]) and np.isposinf(at.dist.cpu().numpy()[[0, 4]]).all()


def test_max_k(hip, bunny_small, dev):
    c = _case("voxel_solid", 8, hip, bunny_small)
    segs, radius = c.segs[:700], c.radius[:700]
    table = tuple(x[:700] for x in c.table)
    full = SX.capsule(segs, radius, c.tri, 64, table)
    assert (full[1] > 64).any() and ((full[1] > 8) & (full[1] <= 64)).any() and (full[1] == 0).any()
    for k in (0, 1, 8, 64):
        rows, count = _capsule(c.sg, segs, radius, dev, k)
        assert np.array_equal(count, full[1]) and np.array_equal(rows, full[0][:, :k]), k          # a row is a prefix of every longer one
        if k:
            assert np.array_equal(_capsule(c.sg, segs, radius, dev, k, count=False)[0], rows)
    with pytest.raises(ValueError, match="max_k"):
        query.capsule_overlap(c.sg, _gpu(segs, dev), _gpu(radius, dev), 65)
    with pytest.raises(ValueError, match="count=True"):
        query.capsule_overlap(c.sg, _gpu(segs, dev), _gpu(radius, dev), 0)


def test_batch_sizes_guard_words_null_outputs_and_shapes(hip, bunny_small, dev):
    c = _case("voxel_solid", 8, hip, bunny_small)
    want, segs = c.free, c.segs
    P = C.c_void_p
    lib = hip.lib
    GUARD = 0x5a5a5a5a
    K = 5
    for n in (1, 63, 65, 257):
        t = _gpu(segs[:n], dev)
        rad = _gpu(c.radius[:n], dev)
        # nothing is written past row n - 1: guard words behind every buffer (a whole wave's worth of them)
        ids = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        dist = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        px = torch.full((3 * n + 192,), GUARD, dtype=torch.int32, device=dev)
        py = torch.full((3 * n + 192,), GUARD, dtype=torch.int32, device=dev)
        cr = torch.full((n + 64,), 0x5a, dtype=torch.uint8, device=dev)
        assert lib.ezrt_query_segment_distance_device(c.sg._h, P(t.data_ptr()), None, n, P(ids.data_ptr()), P(dist.data_ptr()), P(px.data_ptr()),
                                                      P(py.data_ptr()), P(cr.data_ptr()), None) == 0
        torch.cuda.synchronize()
        got = (ids.cpu().numpy()[:n], dist.cpu().numpy()[:n].view(F), px.cpu().numpy()[:3 * n].view(F).reshape(n, 3),
               py.cpu().numpy()[:3 * n].view(F).reshape(n, 3), cr.cpu().numpy()[:n])
        assert not differing(got, tuple(x[:n] for x in want[:5])), n
        assert bool((ids[n:] == GUARD).all() and (dist[n:] == GUARD).all() and (px[3 * n:] == GUARD).all() and (py[3 * n:] == GUARD).all()
                    and (cr[n:] == 0x5a).all()), n
        # every optional output NULL: tri_id alone
        ids.fill_(GUARD)
        assert lib.ezrt_query_segment_distance_device(c.sg._h, P(t.data_ptr()), None, n, P(ids.data_ptr()), None, None, None, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy()[:n], want[0][:n]) and bool((ids[n:] == GUARD).all())
        # ... one at a time
        for which in range(4):
            bufs = [dist, px, py, cr]
            for b in bufs:
                b.fill_(0x5a if b.dtype == torch.uint8 else GUARD)
            args = [P(b.data_ptr()) if j != which else None for j, b in enumerate(bufs)]
            assert lib.ezrt_query_segment_distance_device(c.sg._h, P(t.data_ptr()), None, n, P(ids.data_ptr()), *args, None) == 0
            torch.cuda.synchronize()
            assert bool((bufs[which] == (0x5a if which == 3 else GUARD)).all())                    # the NULL one's neighbour buffer: untouched
            assert np.array_equal(ids.cpu().numpy()[:n], want[0][:n])
            if which != 0:
                assert np.array_equal(dist.cpu().numpy()[:n], want[1][:n].view(np.int32))
        # the _at call on the winners, dist alone and crosses alone
        dist.fill_(GUARD)
        cr.fill_(0x5a)
        w = _gpu(want[0][:n], dev, np.int32)
        assert lib.ezrt_segment_distance_at_device(c.sg._h, P(t.data_ptr()), P(w.data_ptr()), n, P(dist.data_ptr()), None, None, None, None) == 0
        assert lib.ezrt_segment_distance_at_device(c.sg._h, P(t.data_ptr()), P(w.data_ptr()), n, None, None, None, P(cr.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dist.cpu().numpy()[:n], want[1][:n].view(np.int32)) and bool((dist[n:] == GUARD).all())
        assert np.array_equal(cr.cpu().numpy()[:n], want[4][:n]) and bool((cr[n:] == 0x5a).all())
        # the capsule's rows and count, then the rows alone and the count alone
        wr, wc = SX.capsule(segs[:n], c.radius[:n], c.tri, K, tuple(x[:n] for x in c.table))
        rows = torch.full((n * K + 64 * K,), GUARD, dtype=torch.int32, device=dev)
        cnt = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        for use_rows, use_cnt in ((True, True), (True, False), (False, True)):
            rows.fill_(GUARD)
            cnt.fill_(GUARD)
            assert lib.ezrt_query_capsule_overlap_device(c.sg._h, P(t.data_ptr()), P(rad.data_ptr()), n, K if use_rows else 0,
                                                         P(rows.data_ptr()) if use_rows else None, P(cnt.data_ptr()) if use_cnt else None,
                                                         None) == 0
            torch.cuda.synchronize()
            if use_rows:
                assert np.array_equal(rows.cpu().numpy()[:n * K].reshape(n, K), wr), n
            else:
                assert bool((rows == GUARD).all())
            assert bool((rows[n * K:] == GUARD).all())
            if use_cnt:
                assert np.array_equal(cnt.cpu().numpy()[:n], wc), n
            else:
                assert bool((cnt == GUARD).all())
            assert bool((cnt[n:] == GUARD).all())
    got = _distance(c.sg, segs[:30].reshape(2, 3, 5, 6), dev)          # leading dimensions are kept
    assert not differing(tuple(x.reshape((30,) + x.shape[3:]) for x in got), tuple(x[:30] for x in want[:5]))
    at = query.segment_distance_at(c.sg, _gpu(segs[:30].reshape(2, 3, 5, 6), dev), _gpu(want[0][:30].reshape(2, 3, 5), dev, np.int32))
    rows, count = _capsule(c.sg, segs[:30].reshape(2, 3, 5, 6), c.radius[:30].reshape(2, 3, 5), dev, SS.MAX_K)
    torch.cuda.synchronize()
    assert tuple(at.dist.shape) == (2, 3, 5) and tuple(at.point_scene.shape) == (2, 3, 5, 3)
    assert np.array_equal(rows.reshape(30, -1), c.capsule[0][:30]) and np.array_equal(count.reshape(30), c.capsule[1][:30])
    e = query.segment_distance(c.sg, torch.empty((0, 6), device=dev))  # n == 0
    assert tuple(e.tri.shape) == (0,) and tuple(e.point_query.shape) == (0, 3) and e.crosses.dtype == torch.bool
    e = query.segment_distance_at(c.sg, torch.empty((0, 6), device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
    assert tuple(e.dist.shape) == (0,) and tuple(e.point_scene.shape) == (0, 3)
    e = query.capsule_overlap(c.sg, torch.empty((0, 6), device=dev), torch.empty((0,), device=dev), 8, count=True)
    assert tuple(e.tri.shape) == (0, 8) and tuple(e.n_overlap.shape) == (0,)


def test_streams(hip, bunny_small, dev):
    c = _case("voxel_solid", 4, hip, bunny_small)
    src = _gpu(c.segs, dev)
    rad = _gpu(c.radius, dev)
    t = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        t.copy_(src)                                                   # the segments are written on `side`, behind the sleep
    a = query.segment_distance(c.sg, t, stream=side)                   # issued from the default stream's context, onto `side`
    b = query.segment_distance_at(c.sg, t, _gpu(c.free[0], dev, np.int32), stream=side.cuda_stream)   # a raw handle
    k = query.capsule_overlap(c.sg, t, rad, SS.MAX_K, count=True, stream=side.cuda_stream)
    side.synchronize()
    assert not differing(_np(a), c.free[:5], c.segs)
    assert not differing(_np(b)[1:], c.free[1:5], c.segs, NAMES5[1:])
    assert not rows_differ((k.tri.cpu().numpy(), k.n_overlap.cpu().numpy()), c.capsule, c.segs)


def test_at_reproduces_the_winners_and_takes_rows(hip, bunny_small, dev):
    c = _case("nasty", 8, hip, bunny_small)
    segs, tri = c.segs, c.tri
    n, m = segs.shape[0], tri.shape[0]
    t = _gpu(segs, dev)
    got = query.segment_distance(c.sg, t)
    at = query.segment_distance_at(c.sg, t, got.tri)                   # the winners: the query's own outputs, misses included
    torch.cuda.synchronize()
    assert at.tri is got.tri and not differing(_np(at), _np(got), segs) and not differing(_np(got), c.free[:5], segs)
    # ids outside the scene, random pairs
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.resize(np.int32([m, -1, -2, 2 ** 31 - 1, -2 ** 31, m + 64]), n), rng.integers(0, m, n)]).astype(np.int32)
    qq = np.tile(segs, (2, 1))
    at = query.segment_distance_at(c.sg, _gpu(qq, dev), _gpu(ids, dev, np.int32))
    torch.cuda.synchronize()
    w = SX.at(qq, tri, ids)
    assert not differing(_np(at)[1:], w[:4], qq, NAMES5[1:])
    assert np.isposinf(w[0][:n]).all() and np.isfinite(w[0][n:]).sum() > n // 2
    # [n, K] rows of capsule_overlap and of nearest (at the first end point): every entry against its row's segment
    rows = query.capsule_overlap(c.sg, t[:500], _gpu(c.radius[:500], dev), 4).tri
    near = query.nearest(c.sg, t[:500, :3].contiguous(), 3).tri
    for block in (rows, near):
        k = block.shape[1]
        at = query.segment_distance_at(c.sg, t[:500], block)
        torch.cuda.synchronize()
        assert tuple(at.dist.shape) == (500, k) and tuple(at.point_query.shape) == (500, k, 3)
        w = SX.at(np.repeat(segs[:500], k, 0), tri, block.cpu().numpy().reshape(-1))
        assert not differing(tuple(x.reshape((500 * k,) + x.shape[2:]) for x in _np(at)[1:]), w[:4], None, NAMES5[1:])
    listed = rows.cpu().numpy() >= 0                                   # a listed triangle is a candidate, an unused slot misses
    d = query.segment_distance_at(c.sg, t[:500], rows).dist.cpu().numpy()
    assert np.array_equal(np.isfinite(d), listed) and listed.any() and not listed.all()


def test_the_contracts_consequences(hip, bunny_small, dev):
    c = _case("bunny", 4, hip, bunny_small)
    segs, radius = c.segs, c.radius
    t, r = _gpu(segs, dev), _gpu(radius, dev)
    free = query.segment_distance(c.sg, t)
    lim = query.segment_distance(c.sg, t, r)
    cap = query.capsule_overlap(c.sg, t, r, SS.MAX_K, count=True)
    cp = [query.closest_point(c.sg, t[:, 3 * v:3 * v + 3].contiguous()) for v in range(2)]
    torch.cuda.synchronize()
    win, count, rows = lim.tri.cpu().numpy(), cap.n_overlap.cpu().numpy(), cap.tri.cpu().numpy()
    assert np.array_equal(win >= 0, count > 0) and (count > 0).any() and (count == 0).any()       # d_max = r finds one exactly where the capsule counts > 0
    fits = (count > 0) & (count <= SS.MAX_K)
    assert fits.sum() > 100 and (rows[fits] == win[fits][:, None]).any(1).all()                    # ... and that winner is in the row
    # dist * dist <= R2 holds through the restatement's dist2: the device's dist of every listed pair is sqrtf of a dist2 <= R2
    at = query.segment_distance_at(c.sg, t, cap.tri)
    torch.cuda.synchronize()
    d2 = SX.at(np.repeat(segs, SS.MAX_K, 0), c.tri, rows.reshape(-1))[4].reshape(rows.shape)
    with np.errstate(all="ignore"):
        R2 = (radius * radius).astype(F)[:, None]
        assert ((d2 <= R2) == (rows >= 0)).all() and np.array_equal(at.dist.cpu().numpy().view(np.uint32), np.sqrt(d2).astype(F).view(np.uint32))
    # crosses is 1 exactly when the segment crosses some live triangle, and tri is then the lowest such id
    cross = c.table[2]
    f = _np(free)
    assert np.array_equal(f[4] == 1, cross.any(1)) and np.array_equal(f[0][cross.any(1)], np.argmax(cross, 1)[cross.any(1)])
    # the end-point sub-candidates ARE closest_point's function: no end point of a live segment is nearer to the mesh than the segment
    live = SX.live(segs)
    end = np.min([x.dist.cpu().numpy() for x in cp], axis=0)
    assert (f[1][live] <= end[live]).all() and (f[1][live] < end[live]).any()
    assert (live & (f[4] == 0) & (f[1] == end)).sum() > 50             # ... and where an end point is the nearest feature, on the bits


def test_errors(hip, oracle, bunny_small, dev):
    c = _case("voxel_solid", 4, hip, bunny_small)
    lib = hip.lib
    n = 500
    live_q = c.segs[SX.live(c.segs)][:n]
    want = SX.query(live_q, c.tri)
    t = _gpu(live_q, dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    dist = torch.zeros(n, dtype=torch.float32, device=dev)
    px, py = torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev)
    cr = torch.zeros(n, dtype=torch.uint8, device=dev)
    dm = torch.ones(n, dtype=torch.float32, device=dev)
    rows = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    host_f, host_i, host_3, host_b = live_q.copy(), np.zeros(4 * n, np.int32), np.zeros((n, 3), F), np.zeros(n, np.uint8)
    P = C.c_void_p
    f, g, h = lib.ezrt_query_segment_distance_device, lib.ezrt_segment_distance_at_device, lib.ezrt_query_capsule_overlap_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", c.sg._h), kw.get("segs", P(t.data_ptr())), kw.get("d_max", P(dm.data_ptr())), kw.get("n", n),
                       kw.get("tri", P(ids.data_ptr())), kw.get("dist", P(dist.data_ptr())), kw.get("px", P(px.data_ptr())),
                       kw.get("py", P(py.data_ptr())), kw.get("cr", P(cr.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", c.sg._h), kw.get("segs", P(t.data_ptr())), kw.get("tri", P(ids.data_ptr())), kw.get("n", n),
                       kw.get("dist", P(dist.data_ptr())), kw.get("px", P(px.data_ptr())), kw.get("py", P(py.data_ptr())),
                       kw.get("cr", P(cr.data_ptr())), None]
    ha = lambda **kw: [kw.get("s", c.sg._h), kw.get("segs", P(t.data_ptr())), kw.get("radius", P(dm.data_ptr())), kw.get("n", n),
                       kw.get("k", 4), kw.get("rows", P(rows.data_ptr())), kw.get("cnt", P(cnt.data_ptr())), None]
    err = lambda: lib.ezrt_last_error()
    assert f(*fa()) == 0 and g(*ga()) == 0 and h(*ha()) == 0
    torch.cuda.synchronize()
    before = [x.clone() for x in (ids, dist, px, py, cr, rows, cnt)]
    for kw in (dict(s=None), dict(segs=None), dict(tri=None), dict(n=-1)):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    for kw in (dict(s=None), dict(segs=None), dict(radius=None), dict(n=-1)):
        assert h(*ha(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    assert g(*ga(dist=None, px=None, py=None, cr=None)) == EZRT_ERR_INVALID and b"one of dist, point_query, point_scene and crosses" in err()
    for k in (-1, 65):
        assert h(*ha(k=k)) == EZRT_ERR_INVALID and b"max_k out of range" in err()
    assert h(*ha(rows=None)) == EZRT_ERR_INVALID and b"tri_id is required" in err()
    assert h(*ha(k=0, cnt=None)) == EZRT_ERR_INVALID and b"n_overlap is required" in err()       # no output at all
    # host memory is rejected, never read or written
    for kw in (dict(segs=P(host_f.ctypes.data)), dict(d_max=P(host_f.ctypes.data)), dict(tri=P(host_i.ctypes.data)),
               dict(dist=P(host_f.ctypes.data)), dict(px=P(host_3.ctypes.data)), dict(py=P(host_3.ctypes.data)), dict(cr=P(host_b.ctypes.data))):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
        if "d_max" not in kw:
            assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    for kw in (dict(segs=P(host_f.ctypes.data)), dict(radius=P(host_f.ctypes.data)), dict(rows=P(host_i.ctypes.data)), dict(cnt=P(host_i.ctypes.data))):
        assert h(*ha(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    assert not host_i.any() and not host_3.any() and not host_b.any() and np.array_equal(host_f.view(np.uint32), live_q.view(np.uint32))
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0 and h(*ha(n=0)) == 0
    torch.cuda.synchronize()
    assert all(bool((a == b).all()) for a, b in zip(before, (ids, dist, px, py, cr, rows, cnt)))   # no rejected call launched anything
    # the rejected calls left no HIP error behind: the next call works
    assert not differing(_distance(c.sg, live_q, dev), want[:5])
    # the wrappers
    one = torch.zeros(n, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.segment_distance(c.sg, torch.from_numpy(host_f))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.segment_distance_at(c.sg, t, torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError, match="GPU tensor"):
        query.capsule_overlap(c.sg, t, torch.zeros(n))
    with pytest.raises(TypeError, match="HIP library"):
        query.segment_distance(bunny_small.upload(oracle), t)
    with pytest.raises(TypeError, match="HIP library"):
        query.segment_distance_at(bunny_small.upload(oracle), t, one)
    with pytest.raises(TypeError, match="HIP library"):
        query.capsule_overlap(bunny_small.upload(oracle), t, dm)
    with pytest.raises(ValueError, match=r"must have shape \[\.\.\., 6\]"):
        query.segment_distance(c.sg, torch.zeros((4, 9), device=dev))
    with pytest.raises(ValueError, match="d_max must have shape"):
        query.segment_distance(c.sg, t, torch.zeros(n + 1, device=dev))
    with pytest.raises(ValueError, match="radius must have shape"):
        query.capsule_overlap(c.sg, t, torch.zeros(n + 1, device=dev))
    with pytest.raises(TypeError, match="tri must be int32"):
        query.segment_distance_at(c.sg, t, torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="tri must have shape"):
        query.segment_distance_at(c.sg, t, torch.zeros(n + 1, dtype=torch.int32, device=dev))

"""Oriented-box queries on device tensors (include/ezrt_obb_overlap.h, ezrt_amd/query.py: obb_overlap, obb_overlap_at).

`tri` and `n_overlap` are compared on the bits with tests/obb_overlap_expected.py -- the header's rule restated in numpy over boxes x
ALL triangles, pinned to rational clipping by tests/test_obb_overlap_expected.py:

* on the voxel solid, the Bunny scene, adversarial geometry (slivers, a coplanar grid, duplicates, a far cluster) and a scene that
  does not prune (the sweep route), with tests/obb_overlap_scenes.py's boxes: node boxes of the tree and triangle bounding boxes as
  axis-aligned boxes, the same turned by 90 degrees, thin boxes along diagonals, sheared boxes, small boxes at the surface, the whole
  scene, boxes that are not live; K = 1, 8, 64 and count only;
* the walk against the sweep, the `_at` call, batches of 1, 63, 64, 65 and 4000 boxes, NULL outputs and guard words, a [2, 3, 5]
  leading shape;
* a refit, stream order, a render call beside it, untouched counters, the error contract;
* every tree shape of tests/tree_shapes.py: nothing depends on the tree.
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
import allhits_scenes as A  # noqa: E402
import inside_scenes as IS  # noqa: E402
import obb_overlap_expected as OE  # noqa: E402
import obb_overlap_scenes as OS  # noqa: E402
import tree_shapes as T  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = ("voxel_solid", "bunny", "nasty", "not_nested")
SEED = 2200


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, nodes, centre, axes, kind, the restatement's 64-rows and counts, the device scene), computed once and shared"""
    if name not in _cache:
        if name == "voxel_solid":
            v = IS.voxel_solid()
            tri, nodes = v["tri"], v["nodes"]
        else:
            tri, nodes, _ = A.scene(name, bunny_small)
        c, u, kind = OS.boxes_for(tri, nodes, SEED + NAMES.index(name))
        _cache[name] = (tri, nodes, c, u, kind, OE.query(c, u, tri, 64), hip.scene_create(tri, nodes))
    return _cache[name]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _overlap(sg, c, u, dev, k, count=True, **kw):
    r = query.obb_overlap(sg, _gpu(c, dev), _gpu(u, dev), k, count=count, **kw)
    torch.cuda.synchronize()
    assert isinstance(r, query.ObbOverlap) and r.tri.dtype == torch.int32 and tuple(r.tri.shape) == tuple(c.shape[:-1]) + (k,)
    if not count:
        assert r.n_overlap is None
        return r.tri.cpu().numpy(), None
    assert r.n_overlap.dtype == torch.int32 and tuple(r.n_overlap.shape) == tuple(c.shape[:-1])
    return r.tri.cpu().numpy(), r.n_overlap.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_counts_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, c, u, kind, (rows, count), sg = _case(name, hip, bunny_small)
    if name == "not_nested":
        assert sg.prune_info()["mode"] == -1                           # pruning is unavailable: the sweep route runs
    else:
        assert sg.prune_info()["mode"] != -1                           # the walk
    # the comparison is not of zeros: some box has more than 64 overlaps, some has none, most have a few; the box around the whole
    # scene counts every triangle; boxes that are not live count nothing; and among the thin diagonal boxes some node of the caller's
    # tree passes the hull gate and fails the face gate: the second gate has work to do
    assert (count > 64).any() and (count == 0).any() and ((count > 0) & (count <= 64)).sum() > count.size // 2
    assert (count[kind == OS.WHOLE] == OE.vertices(tri).shape[0]).all() and (kind == OS.WHOLE).sum() == 1
    dead = ~OE.live(c, u)
    assert not count[dead].any() and dead.sum() >= 40 and dead[kind == OS.DEAD].sum() >= 60
    thin = kind == OS.THIN
    assert OS.visited(c[thin], u[thin], nodes, True)[1].any()
    for k in (1, 8, 64):
        got, cnt = _overlap(sg, c, u, dev, k)
        bad = cnt != count
        assert not bad.any(), "%s K = %d: %d of %d counts differ, first at box %s %s (kind %d)" % (
            name, k, int(bad.sum()), bad.size, c[np.argmax(bad)], u[np.argmax(bad)].tolist(), kind[np.argmax(bad)])
        bad = (got != rows[:, :k]).any(1)
        assert not bad.any(), "%s K = %d: %d of %d rows differ, first at box %s %s (kind %d)" % (
            name, k, int(bad.sum()), bad.size, c[np.argmax(bad)], u[np.argmax(bad)].tolist(), kind[np.argmax(bad)])
        only, none = _overlap(sg, c, u, dev, k, count=False)           # without n_overlap: the same rows
        assert np.array_equal(only, got)
    empty, cnt = _overlap(sg, c, u, dev, 0)                            # count only
    assert empty.shape == (c.shape[0], 0) and np.array_equal(cnt, count)


def test_routes_agree(hip, bunny_small, dev):
    tri, nodes, c, u, kind, (rows, count), sg = _case("bunny", hip, bunny_small)
    swept = hip.scene_create(*A.not_nested(bunny_small))               # the same triangles, created so that pruning is unavailable
    assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    for k in (0, 5, 64):
        a, b = _overlap(sg, c, u, dev, k), _overlap(swept, c, u, dev, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    assert np.array_equal(a[0], rows) and np.array_equal(a[1], count)


@pytest.mark.parametrize("name", ("voxel_solid", "nasty"))
def test_at_call(hip, bunny_small, dev, name):
    tri, nodes, c, u, kind, (rows, count), sg = _case(name, hip, bunny_small)
    m = OE.vertices(tri).shape[0]
    rng = np.random.default_rng(31)
    n = c.shape[0]
    # pairs of the rows (overlaps, and -1), random pairs (mostly not), the neighbours of row entries, ids outside the scene
    ids = np.concatenate([rows[:, 0], rows[:, 7], rng.integers(0, m, n), np.clip(rows[:, 1] + 1, 0, m - 1),
                          np.resize(np.int32([m, -1, -2, 2 ** 31 - 1, -2 ** 31, m + 64]), n)]).astype(np.int32)
    bc, bu = np.tile(c, (5, 1)), np.tile(u, (5, 1, 1))
    want = OE.at(bc, bu, tri, ids)
    got = query.obb_overlap_at(sg, _gpu(bc, dev), _gpu(bu, dev), _gpu(ids, dev, np.int32))
    torch.cuda.synchronize()
    assert got.dtype == torch.bool and tuple(got.shape) == (5 * n,)
    got = got.cpu().numpy()
    assert np.array_equal(got, want.astype(bool))
    assert want[:n].astype(bool).tolist() == (rows[:, 0] >= 0).tolist() and not want[4 * n:].any()
    assert want[2 * n:4 * n].any() and not want[2 * n:4 * n].all()
    assert not want.reshape(5, n)[:, ~OE.live(c, u)].any()             # boxes that are not live, whatever the id
    # a whole [n, K] block of rows against its boxes: every listed id overlaps, every -1 does not
    block = query.obb_overlap_at(sg, _gpu(c, dev), _gpu(u, dev), _gpu(rows[:, :8], dev, np.int32))
    torch.cuda.synchronize()
    assert tuple(block.shape) == (n, 8) and np.array_equal(block.cpu().numpy(), rows[:, :8] >= 0)


def test_batch_sizes_null_outputs_and_shapes(hip, bunny_small, dev):
    tri, nodes, c, u, kind, (rows, count), sg = _case("voxel_solid", hip, bunny_small)
    for n in (1, 63, 64, 65, 4000):
        sel = np.arange(n) * 7 % c.shape[0]
        for k in (3, 64):
            got, cnt = _overlap(sg, c[sel], u[sel], dev, k)
            assert np.array_equal(got, rows[sel, :k]) and np.array_equal(cnt, count[sel]), (n, k)
    P = C.c_void_p
    lib = hip.lib
    GUARD = 0x5a5a5a5a
    for n, k in ((257, 5), (65, 64), (63, 1), (130, 0)):
        gc, gu = _gpu(c[:n], dev), _gpu(u[:n], dev)
        # nothing is written past row n - 1: guard words behind both buffers (and a whole wave's worth of them)
        ids = torch.full((n * k + 64 * max(k, 1),), GUARD, dtype=torch.int32, device=dev)
        cnt = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        assert lib.ezrt_query_obb_overlap_device(sg._h, P(gc.data_ptr()), P(gu.data_ptr()), n, k, P(ids.data_ptr()) if k else None,
                                                 P(cnt.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy()[:n * k].reshape(n, k), rows[:n, :k]) and bool((ids[n * k:] == GUARD).all()), (n, k)
        assert np.array_equal(cnt.cpu().numpy()[:n], count[:n]) and bool((cnt[n:] == GUARD).all()), (n, k)
        if k:                                                          # n_overlap NULL with max_k > 0
            ids.fill_(GUARD)
            assert lib.ezrt_query_obb_overlap_device(sg._h, P(gc.data_ptr()), P(gu.data_ptr()), n, k, P(ids.data_ptr()), None, None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(ids.cpu().numpy()[:n * k].reshape(n, k), rows[:n, :k]) and bool((ids[n * k:] == GUARD).all()), (n, k)
    out = torch.full((257 + 64,), 9, dtype=torch.uint8, device=dev)
    gc, gu, t = _gpu(c[:257], dev), _gpu(u[:257], dev), _gpu(rows[:257, 0], dev, np.int32)
    assert lib.ezrt_obb_overlap_at_device(sg._h, P(gc.data_ptr()), P(gu.data_ptr()), P(t.data_ptr()), 257, P(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:257], (rows[:257, 0] >= 0).astype(np.uint8)) and bool((out[257:] == 9).all())
    gc, gu = _gpu(c[:30].reshape(2, 3, 5, 3), dev), _gpu(u[:30].reshape(2, 3, 5, 3, 3), dev)
    r = query.obb_overlap(sg, gc, gu, count=True)                      # max_k = 8
    at = query.obb_overlap_at(sg, gc, gu, r.tri)
    one = query.obb_overlap_at(sg, gc, gu, r.tri[..., 0].contiguous())
    torch.cuda.synchronize()
    assert tuple(r.tri.shape) == (2, 3, 5, 8) and tuple(r.n_overlap.shape) == (2, 3, 5) and tuple(at.shape) == (2, 3, 5, 8)
    assert np.array_equal(r.tri.cpu().numpy().reshape(30, 8), rows[:30, :8]) and np.array_equal(r.n_overlap.cpu().numpy().reshape(-1), count[:30])
    assert np.array_equal(at.cpu().numpy(), r.tri.cpu().numpy() >= 0)
    assert tuple(one.shape) == (2, 3, 5) and np.array_equal(one.cpu().numpy().reshape(-1), rows[:30, 0] >= 0)
    e = query.obb_overlap(sg, torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), 4, count=True)
    assert tuple(e.tri.shape) == (0, 4) and tuple(e.n_overlap.shape) == (0,)


def test_after_a_refit(hip, bunny_small, dev):
    v = IS.voxel_solid()
    tri, nodes = v["tri"], v["nodes"]
    _, _, c, u, kind, (rows, count), _ = _case("voxel_solid", hip, bunny_small)
    moved = tri.copy()
    shift = np.float32([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + shift
    qc, qu = c * np.float32(2) + shift, u * np.float32(2)
    sg = hip.scene_create(tri, nodes)
    first = _overlap(sg, qc, qu, dev, 8)
    refit.refit(sg, moved)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))
    assert sg.prune_info()["mode"] != -1 and fresh.prune_info()["mode"] != -1
    got, ref = _overlap(sg, qc, qu, dev, 8), _overlap(fresh, qc, qu, dev, 8)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    want = OE.query(qc, qu, moved, 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(first[1], got[1]) and want[1].any()


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, c, u, kind, (rows, count), sg = _case("voxel_solid", hip, bunny_small)
    src_c, src_u = _gpu(c, dev), _gpu(u, dev)
    gc, gu = torch.zeros_like(src_c), torch.zeros_like(src_u)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        gc.copy_(src_c)                                                # the boxes are written on `side`, behind the sleep
        gu.copy_(src_u)
    a = query.obb_overlap(sg, gc, gu, 8, count=True, stream=side)      # issued from the default stream's context, onto `side`
    b = query.obb_overlap_at(sg, gc, gu, _gpu(rows[:, 0], dev, np.int32), stream=side.cuda_stream)   # a raw handle
    side.synchronize()
    assert np.array_equal(a.tri.cpu().numpy(), rows[:, :8]) and np.array_equal(a.n_overlap.cpu().numpy(), count)
    assert np.array_equal(b.cpu().numpy(), rows[:, 0] >= 0)


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, nodes, c, u, kind, (rows, count), _ = _case("bunny", hip, bunny_small)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    gc, gu = _gpu(c, dev), _gpu(u, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    query.obb_overlap(sg, gc, gu, 8, count=True)
    query.obb_overlap_at(sg, gc, gu, _gpu(rows[:, 0], dev, np.int32))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.obb_overlap(sg, gc, gu, 8, count=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), alone.cpu().numpy().view(np.uint32))
    assert np.array_equal(got.tri.cpu().numpy(), rows[:, :8]) and np.array_equal(got.n_overlap.cpu().numpy(), count)


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, c, u, kind, (rows, count), sg = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n, k = 500, 4
    gc, gu = _gpu(c[:n], dev), _gpu(u[:n], dev)
    ids = torch.zeros((n, k), dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    one = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)
    host_f = u[:n].copy()                                              # a copy of its own; compared on the bits, some boxes hold NaN
    host_i = np.zeros((n, k), np.int32)
    host_b = np.zeros(n, np.uint8)
    P = C.c_void_p
    f, g = lib.ezrt_query_obb_overlap_device, lib.ezrt_obb_overlap_at_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("c", P(gc.data_ptr())), kw.get("u", P(gu.data_ptr())), kw.get("n", n), kw.get("k", k),
                       kw.get("tri", P(ids.data_ptr())), kw.get("cnt", P(cnt.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("c", P(gc.data_ptr())), kw.get("u", P(gu.data_ptr())), kw.get("tri", P(one.data_ptr())),
                       kw.get("n", n), kw.get("out", P(out.data_ptr())), None]
    err = lambda: lib.ezrt_last_error()
    assert f(*fa()) == 0 and g(*ga()) == 0
    for bad in (-1, 65, 1000):
        assert f(*fa(k=bad)) == EZRT_ERR_INVALID and b"max_k out of range [0,64]" in err()
    assert f(*fa(tri=None)) == EZRT_ERR_INVALID and b"tri_id is required when max_k > 0" in err()
    assert f(*fa(k=0, cnt=None)) == EZRT_ERR_INVALID and b"n_overlap is required when max_k == 0" in err()
    assert f(*fa(k=0, tri=None)) == 0 and f(*fa(cnt=None)) == 0
    assert f(*fa(k=0, tri=P(host_i.ctypes.data))) == 0                 # with max_k == 0 tri_id is ignored, whatever it is
    # host memory is rejected, never read or written
    for kw in (dict(c=P(host_f.ctypes.data)), dict(u=P(host_f.ctypes.data)), dict(tri=P(host_i.ctypes.data)), dict(cnt=P(host_i.ctypes.data))):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    for kw in (dict(c=P(host_f.ctypes.data)), dict(u=P(host_f.ctypes.data)), dict(tri=P(host_i.ctypes.data)), dict(out=P(host_b.ctypes.data))):
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    assert not host_i.any() and not host_b.any() and np.array_equal(host_f.view(np.uint32), u[:n].view(np.uint32))
    # NULL, n < 0, n == 0
    for kw in (dict(s=None), dict(c=None), dict(u=None), dict(n=-1)):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    assert g(*ga(tri=None)) == EZRT_ERR_INVALID and g(*ga(out=None)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err()
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0
    # the rejected calls left no HIP error behind: the next call works
    got = _overlap(sg, c[:n], u[:n], dev, 8)
    assert np.array_equal(got[0], rows[:n, :8]) and np.array_equal(got[1], count[:n])
    # the wrapper
    with pytest.raises(ValueError, match="max_k must be an int"):
        query.obb_overlap(sg, gc, gu, 65)
    with pytest.raises(ValueError, match="count=True"):
        query.obb_overlap(sg, gc, gu, 0)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.obb_overlap(sg, torch.from_numpy(c[:n].copy()), gu)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.obb_overlap_at(sg, gc, gu, torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError, match="HIP library"):
        query.obb_overlap(bunny_small.upload(oracle), gc, gu)
    with pytest.raises(TypeError, match="HIP library"):
        query.obb_overlap_at(bunny_small.upload(oracle), gc, gu, one)
    with pytest.raises(ValueError, match="axes must have shape"):
        query.obb_overlap(sg, gc, gu[:10])
    with pytest.raises(ValueError, match="axes must have shape"):
        query.obb_overlap(sg, gc, gu.reshape(n, 9))
    with pytest.raises(ValueError, match=r"must have shape \[\.\.\., 3\]"):
        query.obb_overlap(sg, torch.zeros((4, 6), device=dev), torch.zeros((4, 6, 3), device=dev))
    with pytest.raises(TypeError, match="tri must be int32"):
        query.obb_overlap_at(sg, gc, gu, torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="tri must have shape"):
        query.obb_overlap_at(sg, gc, gu, torch.zeros(n + 1, dtype=torch.int32, device=dev))


# ---- every tree shape a caller can pass (tests/tree_shapes.py): nothing depends on the tree
SHAPES = [(name, None) for name in T.HOST_SHAPES + T.LBVH_SHAPES if name != "chain"] + [("chain", 0), ("chain", 1)]


@pytest.mark.parametrize("name,retree", SHAPES, ids=["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in SHAPES])
def test_every_tree_shape_gives_the_same_rows(hip, dev, name, retree):
    tri, nodes, expect = T.shape(name)
    old = os.environ.get("EZRT_RETREE")
    try:
        if retree is not None:
            os.environ["EZRT_RETREE"] = str(retree)                    # read at scene creation
        sg = hip.scene_create(tri, nodes)
    finally:
        if retree is not None:
            os.environ.pop("EZRT_RETREE", None) if old is None else os.environ.__setitem__("EZRT_RETREE", old)
    assert (sg.prune_info()["mode"] != -1) == expect["walk"]
    c, u, kind = OS.boxes_for(tri, nodes, SEED + 50 + T.SEEDS[name], n=420)
    over = OE.overlaps(c, u, tri)
    if "uncovered" in expect:                                          # the triangles that only the sweep behind the walk reaches are met
        assert over[:, expect["uncovered"]].any()
    count = over.sum(1)
    assert (count[kind == OS.WHOLE] == tri.shape[0]).all() and (count == 0).any() and (count[kind != OS.WHOLE] > 0).any()
    assert tri.shape[0] == 1 or ((count > 0) & (count < tri.shape[0])).any()
    for k in (0, 8, 64):
        want = OE.lowest(over, k)
        got = _overlap(sg, c, u, dev, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, k)
    at = query.obb_overlap_at(sg, _gpu(c, dev), _gpu(u, dev), _gpu(want[0][:, :8], dev, np.int32))
    torch.cuda.synchronize()
    assert np.array_equal(at.cpu().numpy(), want[0][:, :8] >= 0)

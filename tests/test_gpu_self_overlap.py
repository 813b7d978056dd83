"""Self-overlap queries on device tensors (include/ezrt_self_overlap.h, ezrt_amd/query.py: self_overlap, self_overlap_at).

`tri` and `n_overlap` are compared on the bits with tests/self_overlap_expected.py -- the header's rule restated in numpy over
triangles x ALL triangles, pinned to exact arithmetic by tests/test_self_overlap_expected.py:

* on the voxel solid and the Bunny scene (which cross themselves nowhere), the defect scene of tests/self_overlap_scenes.py (a translated copy, a
  duplicated face, a fold, a piercing fan, two blades with rows of more than 64), adversarial geometry (slivers, a coplanar grid,
  duplicates, a far cluster) and two scenes that do not prune (the sweep route); all triangles; K = 1, 8, 64 and count only;
* the walk against the sweep, `ids` (a shuffled subset, ids outside the scene, repeats, a 2-D shape), the `_at` call, batches of 1,
  63, 64, 65 and CP_BLOCK +- 1 ids, n == 0, NULL outputs and guard words;
* a refit that moves the copy clear and back, stream order, a render call beside it, untouched counters, the error contract.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import inside_scenes as IS  # noqa: E402
import self_overlap_expected as SE  # noqa: E402
import self_overlap_scenes as SS  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = ("voxel_solid", "defects", "defects_swept", "bunny", "nasty", "not_nested")
SWEPT = ("defects_swept", "not_nested")                            # created so that pruning is unavailable: the sweep route
CLEAN = ("voxel_solid", "bunny", "not_nested")                     # meshes that cross themselves nowhere
CP_BLOCK = 64                                                      # the kernels' workgroup: one wave


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def host_case(name, bunny_small):
    """(tri, nodes, the restatement's matrix of crossings): needs no device"""
    if name == "voxel_solid":
        v = IS.voxel_solid()
        tri, nodes = v["tri"], v["nodes"]
    elif name == "defects":
        v = SS.defect_scene()
        tri, nodes = v["tri"], v["nodes"]
    elif name == "defects_swept":                                      # the defect scene with a leaf that has two parents
        tri, nodes = A.not_nested(types.SimpleNamespace(**SS.defect_scene()))
    else:
        tri, nodes, _ = A.scene(name, bunny_small)
    return tri, nodes, SE.crosses(tri)


def _case(name, hip, bunny_small):
    """host_case, its 64-rows and counts, and the device scene, computed once and shared"""
    if name not in _cache:
        tri, nodes, cross = host_case(name, bunny_small)
        _cache[name] = (tri, nodes, cross, SE.rows_of(cross, None, 64), hip.scene_create(tri, nodes))
    return _cache[name]


def _gpu(x, dev, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _self(sg, ids, dev, k, count=True, **kw):
    t = None if ids is None else _gpu(ids, dev)
    r = query.self_overlap(sg, t, k, count=count, **kw)
    torch.cuda.synchronize()
    lead = (sg.stats()["n_tri"],) if ids is None else tuple(np.shape(ids))
    assert isinstance(r, query.SelfOverlap) and r.tri.dtype == torch.int32 and tuple(r.tri.shape) == lead + (k,)
    if not count:
        assert r.n_overlap is None
        return r.tri.cpu().numpy(), None
    assert r.n_overlap.dtype == torch.int32 and tuple(r.n_overlap.shape) == lead
    return r.tri.cpu().numpy(), r.n_overlap.cpu().numpy()


def test_the_defect_scene_is_no_comparison_of_zeros(bunny_small):
    tri, nodes, cross = host_case("defects", bunny_small)             # on the CPU, before any device call
    count = cross.sum(1)
    assert (count > 64).any() and (count == 0).any() and ((count >= 1) & (count <= 64)).any()
    i, k = np.nonzero(cross)
    P = TE.vertices(tri)
    assert set(SE.shared_count(P[i], P[k]).tolist()) == {0, 1, 2, 3}   # every case contributes a true pair
    _cache.setdefault("defects_host", (tri, nodes, cross))


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_counts_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, cross, (rows, count), sg = _case(name, hip, bunny_small)
    if name in SWEPT:
        assert sg.prune_info()["mode"] == -1                           # pruning is unavailable: the sweep route runs
    else:
        assert sg.prune_info()["mode"] != -1                           # the walk
    if name in CLEAN:
        assert not count.any()
    else:
        assert (count > 0).sum() > 100 and (count == 0).any()
    m = cross.shape[0]
    for k in (1, 8, 64):
        got, cnt = _self(sg, None, dev, k)
        bad = cnt != count
        assert not bad.any(), "%s K = %d: %d of %d counts differ, first at triangle %d (%d, not %d)" % (
            name, k, int(bad.sum()), bad.size, np.argmax(bad), cnt[np.argmax(bad)], count[np.argmax(bad)])
        bad = (got != rows[:, :k]).any(1)
        assert not bad.any(), "%s K = %d: %d of %d rows differ, first at triangle %d" % (name, k, int(bad.sum()), bad.size, np.argmax(bad))
        only, none = _self(sg, None, dev, k, count=False)              # without n_overlap: the same rows
        assert np.array_equal(only, got)
    empty, cnt = _self(sg, None, dev, 0)                               # count only
    assert empty.shape == (m, 0) and np.array_equal(cnt, count)
    got, cnt = _self(sg, np.arange(m), dev, 8)                         # ids given: the same answer
    assert np.array_equal(got, rows[:, :8]) and np.array_equal(cnt, count)


def test_routes_agree(hip, bunny_small, dev):
    tri, nodes, cross, (rows, count), sg = _case("bunny", hip, bunny_small)
    swept = hip.scene_create(*A.not_nested(bunny_small))               # the same triangles, created so that pruning is unavailable
    assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    for k in (0, 5, 64):
        a, b = _self(sg, None, dev, k), _self(swept, None, dev, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
    assert np.array_equal(a[0], rows) and np.array_equal(a[1], count)


def test_ids(hip, bunny_small, dev):
    tri, nodes, cross, (rows, count), sg = _case("defects", hip, bunny_small)
    m = cross.shape[0]
    rng = np.random.default_rng(5)
    ids = rng.permutation(m)[:200].astype(np.int32)                    # a shuffled subset
    ids[::10] = np.resize(np.int32([-1, m, m + 64, -2 ** 31, 2 ** 31 - 1]), ids[::10].size)   # ids outside the scene
    ids[5::10] = ids[4::10]                                            # repeated ids
    want = SE.rows_of(cross, ids, 8)
    got = _self(sg, ids, dev, 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0][::10] == -1).all() and not got[1][::10].any() and got[1].any()
    assert np.array_equal(got[0][5::10], got[0][4::10])
    two = _self(sg, ids.reshape(4, 50), dev, 3)                        # a 2-D shape
    assert np.array_equal(two[0].reshape(200, 3), want[0][:, :3]) and np.array_equal(two[1].reshape(-1), want[1])


@pytest.mark.parametrize("name", ("defects", "nasty"))
def test_at_call(hip, bunny_small, dev, name):
    tri, nodes, cross, (rows, count), sg = _case(name, hip, bunny_small)
    m = cross.shape[0]
    r = query.self_overlap(sg, None, 8)
    block = query.self_overlap_at(sg, torch.arange(m, dtype=torch.int32, device=dev)[:, None].expand(m, 8).contiguous(), r.tri)
    torch.cuda.synchronize()
    assert np.array_equal(r.tri.cpu().numpy(), rows[:, :8])
    assert block.dtype == torch.bool and tuple(block.shape) == (m, 8)
    assert np.array_equal(block.cpu().numpy(), rows[:, :8] >= 0) and block.any() and not block.all()   # every id true, every -1 false
    rng = np.random.default_rng(32)
    n = 4000
    i, k = np.nonzero(cross)
    pick = rng.integers(0, i.size, n // 4)
    a = np.concatenate([rng.integers(0, m, n // 2), i[pick], np.resize(np.int32([m, -1, 3, 2 ** 31 - 1, -2 ** 31, 0]), n // 4)]).astype(np.int32)
    b = np.concatenate([rng.integers(0, m, n // 4), a[n // 4:n // 2], k[pick], np.resize(np.int32([0, 5, m, -1, 7, m + 64]), n // 4)]).astype(np.int32)
    want = SE.at(tri, a, b)                                            # random pairs, a == b, crossing pairs, ids outside the scene
    got = query.self_overlap_at(sg, _gpu(a, dev), _gpu(b, dev))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want.astype(bool))
    assert not want[n // 4:n // 2].any() and want[n // 2:3 * n // 4].all() and not want[3 * n // 4:].any()
    assert np.array_equal(want, cross[np.clip(a, 0, m - 1), np.clip(b, 0, m - 1)] & (a >= 0) & (a < m) & (b >= 0) & (b < m))


def test_batch_sizes_null_outputs_and_guards(hip, bunny_small, dev):
    tri, nodes, cross, (rows, count), sg = _case("defects", hip, bunny_small)
    m = cross.shape[0]
    order = (np.arange(m) * 7 % m).astype(np.int32)
    for n in (1, 63, 64, 65, CP_BLOCK - 1, CP_BLOCK + 1, 2 * CP_BLOCK + 1):
        for k in (3, 64):
            got, cnt = _self(sg, order[:n], dev, k)
            assert np.array_equal(got, rows[order[:n], :k]) and np.array_equal(cnt, count[order[:n]]), (n, k)
    P = C.c_void_p
    lib = hip.lib
    GUARD = 0x5a5a5a5a
    for n, k, given in ((257, 5, True), (65, 64, False), (63, 1, True), (130, 0, False)):
        sel = order[:n] if given else np.arange(n)
        t = _gpu(sel, dev)
        ids = torch.full((n * k + 64 * max(k, 1),), GUARD, dtype=torch.int32, device=dev)
        cnt = torch.full((n + 64,), GUARD, dtype=torch.int32, device=dev)
        assert lib.ezrt_query_self_overlap_device(sg._h, P(t.data_ptr()) if given else None, n, k, P(ids.data_ptr()) if k else None,
                                                  P(cnt.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy()[:n * k].reshape(n, k), rows[sel, :k]) and bool((ids[n * k:] == GUARD).all()), (n, k)
        assert np.array_equal(cnt.cpu().numpy()[:n], count[sel]) and bool((cnt[n:] == GUARD).all()), (n, k)
        if k:                                                          # n_overlap NULL with max_k > 0
            ids.fill_(GUARD)
            assert lib.ezrt_query_self_overlap_device(sg._h, P(t.data_ptr()) if given else None, n, k, P(ids.data_ptr()), None, None) == 0
            torch.cuda.synchronize()
            assert np.array_equal(ids.cpu().numpy()[:n * k].reshape(n, k), rows[sel, :k]) and bool((ids[n * k:] == GUARD).all()), (n, k)
    out = torch.full((257 + 64,), 9, dtype=torch.uint8, device=dev)
    a, b = _gpu(order[:257], dev), _gpu(rows[order[:257], 0], dev)
    assert lib.ezrt_self_overlap_at_device(sg._h, P(a.data_ptr()), P(b.data_ptr()), 257, P(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:257], (rows[order[:257], 0] >= 0).astype(np.uint8)) and bool((out[257:] == 9).all())
    e = query.self_overlap(sg, torch.empty((0,), dtype=torch.int32, device=dev), 4, count=True)       # n == 0
    assert tuple(e.tri.shape) == (0, 4) and tuple(e.n_overlap.shape) == (0,)
    assert tuple(query.self_overlap_at(sg, e.n_overlap, e.n_overlap).shape) == (0,)


def test_a_refit_moves_the_copy_clear_and_back(hip, bunny_small, dev):
    d = SS.defect_scene()
    tri, nodes, cross, (rows, count), _ = _case("defects", hip, bunny_small)
    plain, copy = d["plain"], d["copy"]
    moved = SS.moved_clear()
    clear = SE.crosses(moved)
    want = SE.rows_of(clear, None, 8)
    assert cross[np.ix_(plain, copy)].any() and not clear[np.ix_(plain, copy)].any() and clear.any()
    sg = hip.scene_create(tri, nodes)
    first = _self(sg, None, dev, 8)
    assert np.array_equal(first[0], rows[:, :8]) and np.array_equal(first[1], count)
    refit.refit(sg, moved)
    assert sg.prune_info()["mode"] != -1
    got = _self(sg, None, dev, 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1][plain] < count[plain]).any() and not (got[1] > count).any()
    held = query.self_overlap_at(sg, torch.arange(len(count), dtype=torch.int32, device=dev)[:, None].expand(-1, 8).contiguous(),
                                 _gpu(rows[:, :8], dev))               # the rows held from before the refit, narrowed
    torch.cuda.synchronize()
    a = np.repeat(np.arange(len(count)), 8)
    assert np.array_equal(held.cpu().numpy().reshape(-1), SE.at(moved, a, rows[:, :8].reshape(-1)).astype(bool))
    refit.refit(sg, tri)                                               # back: the crossings return
    got = _self(sg, None, dev, 8)
    assert np.array_equal(got[0], rows[:, :8]) and np.array_equal(got[1], count)


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, cross, (rows, count), sg = _case("defects", hip, bunny_small)
    m = cross.shape[0]
    src = torch.arange(m, dtype=torch.int32, device=dev)
    t = torch.full_like(src, -1)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        t.copy_(src)                                                   # the ids are written on `side`, behind the sleep
    a = query.self_overlap(sg, t, 8, count=True, stream=side)          # issued from the default stream's context, onto `side`
    b = query.self_overlap_at(sg, t, _gpu(rows[:, 0], dev), stream=side.cuda_stream)   # a raw handle
    side.synchronize()
    assert np.array_equal(a.tri.cpu().numpy(), rows[:, :8]) and np.array_equal(a.n_overlap.cpu().numpy(), count)
    assert np.array_equal(b.cpu().numpy(), rows[:, 0] >= 0)


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, nodes, cross, (rows, count), _ = _case("bunny", hip, bunny_small)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    query.self_overlap(sg, None, 8, count=True)
    query.self_overlap_at(sg, _gpu(np.arange(len(count)), dev), _gpu(rows[:, 0], dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.self_overlap(sg, None, 8, count=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), alone.cpu().numpy().view(np.uint32))
    assert np.array_equal(got.tri.cpu().numpy(), rows[:, :8]) and np.array_equal(got.n_overlap.cpu().numpy(), count)


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, cross, (rows, count), sg = _case("defects", hip, bunny_small)
    m = cross.shape[0]
    lib = hip.lib
    n, k = 500, 4
    t = _gpu(np.arange(n), dev)
    ids = torch.zeros((n, k), dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)
    host_i = np.zeros((n, k), np.int32)
    host_b = np.zeros(n, np.uint8)
    P = C.c_void_p
    f, g = lib.ezrt_query_self_overlap_device, lib.ezrt_self_overlap_at_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("ids", P(t.data_ptr())), kw.get("n", n), kw.get("k", k),
                       kw.get("tri", P(ids.data_ptr())), kw.get("cnt", P(cnt.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("a", P(t.data_ptr())), kw.get("b", P(cnt.data_ptr())),
                       kw.get("n", n), kw.get("out", P(out.data_ptr())), None]
    err = lambda: lib.ezrt_last_error()
    assert f(*fa()) == 0 and g(*ga()) == 0
    for bad in (-1, 65, 1000):
        assert f(*fa(k=bad)) == EZRT_ERR_INVALID and b"max_k out of range [0,64]" in err()
    assert f(*fa(tri=None)) == EZRT_ERR_INVALID and b"tri_id is required when max_k > 0" in err()
    assert f(*fa(k=0, cnt=None)) == EZRT_ERR_INVALID and b"n_overlap is required when max_k == 0" in err()
    assert f(*fa(k=0, tri=None)) == 0 and f(*fa(cnt=None)) == 0
    assert f(*fa(k=0, tri=P(host_i.ctypes.data))) == 0                 # with max_k == 0 tri_id is ignored, whatever it is
    assert f(*fa(ids=None)) == 0                                       # NULL ids: the first n triangles
    assert f(*fa(ids=None, n=m + 1, k=0)) == EZRT_ERR_INVALID and b"exceeds the scene's" in err()
    # host memory is rejected, never read or written
    for kw in (dict(ids=P(host_i.ctypes.data)), dict(tri=P(host_i.ctypes.data)), dict(cnt=P(host_i.ctypes.data))):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    for kw in (dict(a=P(host_i.ctypes.data)), dict(b=P(host_i.ctypes.data)), dict(out=P(host_b.ctypes.data))):
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"device memory of the scene's device" in err(), kw
    assert not host_i.any() and not host_b.any()
    # NULL, n < 0, n == 0
    for kw in (dict(s=None), dict(n=-1)):
        assert f(*fa(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    for kw in (dict(a=None), dict(b=None), dict(out=None)):
        assert g(*ga(**kw)) == EZRT_ERR_INVALID and b"NULL argument or n < 0" in err(), kw
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0
    # the rejected calls left no HIP error behind: the next call works
    got = _self(sg, np.arange(n), dev, 8)
    assert np.array_equal(got[0], rows[:n, :8]) and np.array_equal(got[1], count[:n])
    # the wrapper
    with pytest.raises(ValueError, match="max_k must be an int"):
        query.self_overlap(sg, t, 65)
    with pytest.raises(ValueError, match="count=True"):
        query.self_overlap(sg, None, 0)
    with pytest.raises(TypeError, match="GPU tensor"):
        query.self_overlap(sg, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="ids must be int32"):
        query.self_overlap(sg, torch.zeros(4, device=dev))
    with pytest.raises(TypeError, match="HIP library"):
        query.self_overlap(bunny_small.upload(oracle), t)
    with pytest.raises(TypeError, match="HIP library"):
        query.self_overlap_at(bunny_small.upload(oracle), t, t)
    with pytest.raises(TypeError, match="b must be int32"):
        query.self_overlap_at(sg, t, torch.zeros(n, device=dev))
    with pytest.raises(ValueError, match="b must have shape"):
        query.self_overlap_at(sg, t, torch.zeros(n + 1, dtype=torch.int32, device=dev))

"""Winding-number queries on device tensors (include/ezrt_winding.h, ezrt_amd/query.py: winding_number, winding_number_at).

`fixed` is compared ON THE BITS with tests/winding_expected.py -- the header's rule restated in numpy over all triangles, held to the
real-number value by tests/test_winding_expected.py -- and `winding` on the bits with the restatement's float:

* on the voxel solid, the same with faces removed, the Bunny scene (64 points), adversarial geometry (slivers, a coplanar grid,
  duplicates, a far cluster) and a scene that does not prune, with tests/winding_scenes.py's points: non-finite ones and points
  exactly on vertices, edges and faces included;
* every way of slicing the triangle range (chunks = 1, 2, 7, n_tri, n_tri + 5, and the library's own choice on both sides of its
  rule), batches of 1 .. 4000 points, a [2, 3, 5, 3] shape, winding = NULL over a poisoned accumulator;
* every tree shape a caller can pass (the tree cannot matter: nothing reads it);
* winding_number_at for rows of ids, -1 and ids outside the scene included, and its sum over all ids against winding_number;
* a refit, stream order, a render call beside it, untouched counters, the error contract, and agreement with `inside` on the
  closed solid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import tree_shapes as T  # noqa: E402
import winding_expected as WE  # noqa: E402
import winding_scenes as WS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = WS.GPU_NAMES
WN_FILL, WN_BLOCK, WN_MIN_SLICE = 8192, 64, 256                        # ezrt_queries.hip: the rule of chunks == 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, nodes, points, S int64 [n] by the restatement, the device scene), computed once and shared"""
    if name not in _cache:
        tri, nodes, pts = WS.inputs(name, bunny_small)
        if name in ("bunny", "not_nested"):                            # 5 300 triangles: 64 points, evenly taken from every kind
            pts = np.ascontiguousarray(pts[np.linspace(0, pts.shape[0] - 1, 64).astype(np.int64)])
        _cache[name] = (tri, nodes, pts, WE.fixed(pts, tri), hip.scene_create(tri, nodes))
    return _cache[name]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _winding(sg, pts, dev, **kw):
    """(fixed int64, winding float32) as numpy, after the checks of the shapes and types"""
    w, f = query.winding_number(sg, _gpu(pts, dev), fixed=True, **kw)
    torch.cuda.synchronize()
    assert w.dtype == torch.float32 and f.dtype == torch.int64 and tuple(w.shape) == tuple(f.shape) == tuple(pts.shape[:-1])
    return f.cpu().numpy(), w.cpu().numpy()


def _same(got, S, what=""):
    f, w = got
    bad = f.reshape(-1) != S.reshape(-1)
    assert not bad.any(), "%s: %d of %d sums differ, first at %d: %d against %d" % (what, int(bad.sum()), bad.size, int(np.argmax(bad)),
                                                                                   f.reshape(-1)[np.argmax(bad)], S.reshape(-1)[np.argmax(bad)])
    assert np.array_equal(_bits(w).reshape(-1), _bits(WE.winding_of(S)).reshape(-1)), what


@pytest.mark.parametrize("name", NAMES)
def test_fixed_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, pts, want, sg = _case(name, hip, bunny_small)
    assert (sg.prune_info()["mode"] == -1) == (name == "not_nested")   # (a scene that does not prune is summed like any other)
    _same(_winding(sg, pts, dev), want, name)
    finite = np.isfinite(pts).all(1)
    assert not want[~finite].any() and (~finite).any() and np.count_nonzero(want) > 0.8 * finite.sum()
    w = WE.winding_of(want)
    assert w.max() > 0.9 and np.abs(w).min() < 0.01                    # the comparison is not of zeros


def test_every_slicing_gives_the_same_bits(hip, bunny_small, dev):
    lib = hip.lib
    for name in ("nasty", "open_solid"):
        tri, nodes, pts, want, sg = _case(name, hip, bunny_small)
        n_tri = tri.shape[0]
        for chunks in (1, 2, 7, n_tri, n_tri + 5, None):
            _same(_winding(sg, pts, dev, chunks=chunks), want, "%s chunks=%r" % (name, chunks))
    # the library's own choice, on both sides of its rule: a pure function of n and n_tri
    tri, nodes, pts, want, sg = _case("nasty", hip, bunny_small)
    n, n_tri = pts.shape[0], tri.shape[0]
    blocks = (n + WN_BLOCK - 1) // WN_BLOCK
    assert blocks < WN_FILL and n_tri // WN_MIN_SLICE == 10 < (WN_FILL + blocks - 1) // blocks
    assert lib.ezrt_winding_chunks(n, n_tri) == 10                     # few points: ten slices of at least 256 triangles
    big = WN_FILL * WN_BLOCK                                           # 524 288 points fill the device: one slice
    assert lib.ezrt_winding_chunks(big, n_tri) == 1 and lib.ezrt_winding_chunks(big - WN_BLOCK, n_tri) == 2
    sel = np.arange(big) % n
    _same(_winding(sg, pts[sel], dev), want[sel], "one slice by the rule")
    _same(_winding(sg, pts[sel[:big - WN_BLOCK]], dev), want[sel[:big - WN_BLOCK]], "two slices by the rule")
    small = _case("voxel_solid", hip, bunny_small)                     # 288 triangles: never more than one slice
    assert lib.ezrt_winding_chunks(small[2].shape[0], small[0].shape[0]) == 1


def test_batch_sizes_and_shapes(hip, bunny_small, dev):
    for name in ("nasty", "voxel_solid"):                              # 2 812 and 288 triangles: no multiple of 64; sliced and not
        tri, nodes, pts, want, sg = _case(name, hip, bunny_small)
        assert tri.shape[0] % 64 != 0
        for n in (1, 63, 64, 65, 255, 256, 257, 4000):
            sel = np.arange(n) * 7 % pts.shape[0]
            _same(_winding(sg, pts[sel], dev), want[sel], "%s n=%d" % (name, n))
            _same(_winding(sg, pts[sel], dev, chunks=1), want[sel], "%s n=%d, one slice" % (name, n))
        lead = pts[:30].reshape(2, 3, 5, 3)
        f, w = _winding(sg, lead, dev)
        assert f.shape == (2, 3, 5)
        _same((f, w), want[:30], name)
        only = query.winding_number(sg, _gpu(lead, dev))               # without fixed=True: one tensor
        assert isinstance(only, torch.Tensor) and only.dtype == torch.float32 and tuple(only.shape) == (2, 3, 5)
        e = query.winding_number(sg, torch.empty((0, 3), device=dev), fixed=True)
        assert tuple(e[0].shape) == (0,) == tuple(e[1].shape) and e[1].dtype == torch.int64


def test_null_winding_over_a_poisoned_accumulator(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("nasty", hip, bunny_small)
    lib, P = hip.lib, C.c_void_p
    n = 257
    p = _gpu(pts[:n], dev)
    for chunks in (0, 1, 3, 10 ** 6):
        acc = torch.full((n,), -0x1234567890ABCDE, dtype=torch.int64, device=dev)
        assert lib.ezrt_query_winding_device(sg._h, P(p.data_ptr()), n, chunks, P(acc.data_ptr()), None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(acc.cpu().numpy(), want[:n]), chunks     # the library's zeroing covers the garbage
        w = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        acc.fill_(0x7FFFFFFFFFFFFFFF)
        assert lib.ezrt_query_winding_device(sg._h, P(p.data_ptr()), n, chunks, P(acc.data_ptr()), P(w.data_ptr()), None) == 0
        torch.cuda.synchronize()
        _same((acc.cpu().numpy(), w.cpu().numpy()), want[:n], "chunks=%d" % chunks)


@pytest.mark.parametrize("name", T.HOST_SHAPES + T.LBVH_SHAPES)
def test_every_tree_shape(hip, dev, name):
    tri, nodes, expect = T.shape(name)
    pts = T.shape_queries(name)["points"]
    want = WE.fixed(pts, tri)
    sg = hip.scene_create(tri, nodes)
    for chunks in (None, 1, 3):
        _same(_winding(sg, pts, dev, chunks=chunks), want, "%s chunks=%r" % (name, chunks))
    assert np.count_nonzero(want) > 0.5 * want.size


def test_winding_number_at(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    rng = np.random.default_rng(31)
    n, m = pts.shape[0], tri.shape[0]
    p = _gpu(pts, dev)
    ids = rng.integers(0, m, n).astype(np.int32)
    ids[::9], ids[1::9], ids[2::9] = -1, m, 2 ** 31 - 1
    w, f = query.winding_number_at(sg, p, _gpu(ids, dev, np.int32))
    rows = rng.integers(-2, m + 2, (n, 5)).astype(np.int32)
    wr, fr = query.winding_number_at(sg, p, _gpu(rows, dev, np.int32))
    torch.cuda.synchronize()
    assert f.dtype == torch.int64 and w.dtype == torch.float32 and tuple(f.shape) == (n,) and tuple(fr.shape) == tuple(wr.shape) == (n, 5)
    q, qr = WE.terms_at(pts, tri, ids), WE.terms_at(pts, tri, rows)
    _same((f.cpu().numpy(), w.cpu().numpy()), q, "[n]")
    _same((fr.cpu().numpy(), wr.cpu().numpy()), qr, "[n, K]")
    assert not q[::9].any() and not q[1::9].any() and not q[2::9].any() and np.count_nonzero(q) > n // 2
    # the terms of all ids sum to winding_number's fixed
    k = 200
    every = torch.arange(m, dtype=torch.int32, device=dev)[None, :].expand(k, m).contiguous()
    _, terms = query.winding_number_at(sg, p[:k].contiguous(), every)
    _, total = query.winding_number(sg, p[:k].contiguous(), fixed=True)
    torch.cuda.synchronize()
    assert torch.equal(terms.sum(1), total) and np.array_equal(total.cpu().numpy(), want[:k])
    e = query.winding_number_at(sg, torch.empty((0, 3), device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev))
    assert tuple(e[0].shape) == (0, 4) == tuple(e[1].shape)


def test_after_a_refit(hip, bunny_small, dev):
    v = IS.voxel_solid()
    tri, nodes, pts = v["tri"], v["nodes"], v["points"]
    moved = tri.copy()
    shift = np.float32([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + shift
    q = pts * np.float32(2) + shift
    sg = hip.scene_create(tri, nodes)
    first = _winding(sg, q, dev)
    refit.refit(sg, moved)
    want = WE.fixed(q, moved)
    _same(_winding(sg, q, dev), want, "after the refit")
    _same(_winding(sg, q, dev, chunks=4), want, "after the refit, sliced")
    assert not np.array_equal(first[0], want)
    inside = v["kept"] & v["truth"]
    assert np.all(WE.winding_of(want)[inside] > 0.5) and np.all(WE.winding_of(want)[v["kept"] & ~v["truth"]] < 0.5)


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("nasty", hip, bunny_small)
    src = _gpu(pts, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                   # the points are written on `side`, behind the sleep
    a = query.winding_number(sg, p, fixed=True, stream=side)           # issued from the default stream's context, onto `side`
    b = query.winding_number(sg, p, fixed=True, chunks=1, stream=side.cuda_stream)   # a raw handle
    ids = torch.zeros(pts.shape[0], dtype=torch.int32, device=dev)
    c = query.winding_number_at(sg, p, ids, stream=side)
    side.synchronize()
    _same((a[1].cpu().numpy(), a[0].cpu().numpy()), want, "sliced")
    _same((b[1].cpu().numpy(), b[0].cpu().numpy()), want, "one slice")
    assert np.array_equal(c[1].cpu().numpy(), WE.terms_at(pts, tri, np.zeros(pts.shape[0], np.int32)))


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, nodes, pts, want, _ = _case("bunny", hip, bunny_small)
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
    query.winding_number(sg, p)
    query.winding_number(sg, p, chunks=1)
    query.winding_number_at(sg, p, torch.zeros(pts.shape[0], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.winding_number(sg, p, fixed=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(frame.cpu().numpy()), _bits(alone.cpu().numpy()))
    _same((got[1].cpu().numpy(), got[0].cpu().numpy()), want, "beside a render call")


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = 500
    p = _gpu(pts[:n], dev)
    acc = torch.zeros(n, dtype=torch.int64, device=dev)
    w = torch.zeros(n, dtype=torch.float32, device=dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    host_pts = np.ascontiguousarray(pts[:n])
    host_q, host_w, host_i = np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, np.int32)
    P = C.c_void_p
    f, g = lib.ezrt_query_winding_device, lib.ezrt_winding_at_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("n", n), kw.get("chunks", 0), kw.get("fixed", P(acc.data_ptr())),
                       kw.get("winding", P(w.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("tri", P(ids.data_ptr())), kw.get("n", n),
                       kw.get("fixed", P(acc.data_ptr())), kw.get("winding", P(w.data_ptr())), None]
    assert f(*fa()) == 0 and g(*ga()) == 0 and f(*fa(winding=None)) == 0 and g(*ga(winding=None)) == 0
    for chunks in (-1, -2 ** 31):
        assert f(*fa(chunks=chunks)) == EZRT_ERR_INVALID and b"chunks" in lib.ezrt_last_error()
    # host memory is rejected, never read or written
    assert f(*fa(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*fa(fixed=P(host_q.ctypes.data))) == EZRT_ERR_INVALID and f(*fa(winding=P(host_w.ctypes.data))) == EZRT_ERR_INVALID
    assert g(*ga(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID and g(*ga(tri=P(host_i.ctypes.data))) == EZRT_ERR_INVALID
    assert g(*ga(fixed=P(host_q.ctypes.data))) == EZRT_ERR_INVALID and g(*ga(winding=P(host_w.ctypes.data))) == EZRT_ERR_INVALID
    assert not host_q.any() and not host_w.any() and not host_i.any()
    # NULL, n < 0, n == 0
    assert f(*fa(fixed=None)) == EZRT_ERR_INVALID and f(*fa(s=None)) == EZRT_ERR_INVALID and f(*fa(pts=None)) == EZRT_ERR_INVALID
    assert g(*ga(fixed=None)) == EZRT_ERR_INVALID and g(*ga(s=None)) == EZRT_ERR_INVALID and g(*ga(pts=None)) == EZRT_ERR_INVALID
    assert g(*ga(tri=None)) == EZRT_ERR_INVALID
    assert f(*fa(n=-1)) == EZRT_ERR_INVALID and g(*ga(n=-1)) == EZRT_ERR_INVALID
    acc.fill_(5)
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0 and f(*fa(n=0, chunks=4)) == 0
    torch.cuda.synchronize()
    assert bool((acc == 5).all())                                      # n == 0 launches nothing, the zeroing included
    # the rejected calls left no HIP error behind: the next call works
    _same(_winding(sg, pts[:n], dev), want[:n], "after the rejected calls")
    # the wrapper
    with pytest.raises(ValueError):
        query.winding_number(sg, p, chunks=0)
    with pytest.raises(TypeError):
        query.winding_number(sg, torch.from_numpy(host_pts))
    with pytest.raises(TypeError):
        query.winding_number(bunny_small.upload(oracle), p)
    with pytest.raises(TypeError):
        query.winding_number_at(bunny_small.upload(oracle), p, ids)
    with pytest.raises(ValueError):
        query.winding_number(sg, torch.zeros((4, 6), device=dev))
    with pytest.raises(ValueError):
        query.winding_number_at(sg, p, torch.zeros((n + 1,), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        query.winding_number_at(sg, p, torch.zeros((n,), dtype=torch.int64, device=dev))


def test_agrees_with_inside_on_the_closed_solid(hip, bunny_small, dev):
    v = IS.voxel_solid()
    sg = _case("voxel_solid", hip, bunny_small)[4]
    pts, kept, truth = v["points"], v["kept"], v["truth"]
    p = _gpu(pts, dev)
    w = query.winding_number(sg, p)
    torch.cuda.synchronize()
    by_winding = (w > 0.5).cpu().numpy()
    assert kept.sum() >= 500 and np.array_equal(by_winding[kept], truth[kept])
    for axis in range(6):
        ins = query.inside(sg, p, axis)
        torch.cuda.synchronize()
        assert np.array_equal(ins.cpu().numpy()[kept], by_winding[kept]), axis

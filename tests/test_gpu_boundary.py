"""Boundary loops and caps on device tensors (include/ezrt_boundary.h, ezrt_amd/query.py: mesh_boundary, boundary_points, loop_area,
cap_rows).

Every output of both calls -- next, loop, pos, order, loop_offsets, lflags, area2, summary; cap, cap_valid -- is compared EXACTLY with
tests/boundary_expected.py, the header's rule restated on the host and held to its properties by tests/test_boundary_expected.py.
There is no tolerance anywhere, area2 included.

* every case of tests/boundary_scenes.py, with and without the area group, over poisoned buffers with room behind them: what the call
  must not touch (order at and beyond B, loop_offsets beyond L, lflags at and beyond L, area2 at and beyond 3 L, cap rows at and beyond
  B, the room, the bytes behind `work`, the guard entries behind the inputs) still holds the poison;
* `work` pre-filled with zeros, with 0xFF and with random bytes; two calls on two streams with two `work` buffers;
* B2's robustness: random twin and edge_class, and a truthful topology with 1 % of its entries overwritten, against the restatement
  on the same arrays;
* the loop this is for: boundary, cap_rows, a new scene of the rows and the cap, topology closed and consistently wound, orientation
  one closed orientable patch per component;
* the wrappers, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_expected as BE  # noqa: E402
import boundary_scenes as BS  # noqa: E402
import orient_expected as OE  # noqa: E402
import orient_scenes as OS  # noqa: E402
import topology_expected as TE  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
POISON = -7
POISON8 = 249
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip):
    """(tri, the device scene, the restatement's topology, its boundary), computed once and shared"""
    if name not in _cache:
        tri, nodes = BS.scene(name)
        t = TE.topology(tri, components=False)
        _cache[name] = (tri, hip.scene_create(tri, nodes), t, BE.boundary(tri, t.twin, t.edge_class))
    return _cache[name]


def _g(x, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _sizes(n_tri):
    H = 3 * n_tri
    return (("next", torch.int32, H), ("loop", torch.int32, H), ("pos", torch.int32, H), ("order", torch.int32, H),
            ("loop_offsets", torch.int32, H + 1), ("lflags", torch.uint8, H), ("area2", torch.int64, 3 * H), ("summary", torch.int64, 8))


def _raw(lib, sg, n_tri, dev, twin, cls, area=True, work_fill=FILL, stream=None, sync=True):
    """the C call itself over poisoned buffers, each with ROOM entries behind its stated size: (dict of device tensors, a check to run
    after the synchronisation)"""
    out = {k: torch.full((size + ROOM,), POISON8 if dt == torch.uint8 else POISON, dtype=dt, device=dev) for k, dt, size in _sizes(n_tri)}
    d_twin = _g(np.concatenate([np.asarray(twin, np.int32).ravel(), np.full(ROOM, POISON, np.int32)]), dev, np.int32)
    d_cls = _g(np.concatenate([np.asarray(cls, np.uint8).ravel(), np.full(ROOM, 1, np.uint8)]), dev, np.uint8)   # a guard that says BOUNDARY
    keep = (d_twin.clone(), d_cls.clone())
    wb = lib.ezrt_boundary_work_bytes(n_tri)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:                                                                      # a generator: random bytes
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))                     # (the fills above; an earlier call on another stream goes on)
    else:
        torch.cuda.synchronize()
    d = lambda k: P(out[k].data_ptr())
    got = lib.ezrt_mesh_boundary_device(sg._h, P(d_twin.data_ptr()), P(d_cls.data_ptr()), d("next"), d("loop"), d("pos"), d("order"),
                                        d("loop_offsets"), d("lflags"), d("area2") if area else None, d("summary"), P(work.data_ptr()), wb,
                                        P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((work[wb // 8:] == tail).all())                            # nothing behind the stated bytes of work
        assert bool((d_twin == keep[0]).all()) and bool((d_cls == keep[1]).all())   # the inputs and their guards
        return {k: v.cpu().numpy() for k, v in out.items()}
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same(got, want, n_tri, area=True, what=""):
    """every output against the restatement's, and the poison wherever the call must not write"""
    B, L = int(want.summary[0]), int(want.summary[1])
    used = {"next": 3 * n_tri, "loop": 3 * n_tri, "pos": 3 * n_tri, "order": B, "loop_offsets": L + 1, "lflags": L, "area2": 3 * L if area else 0,
            "summary": 8}
    for name, dt, _ in _sizes(n_tri):
        size = used[name]
        poison = POISON8 if dt == torch.uint8 else POISON
        if name == "area2":
            w = want.area2.reshape(-1) if area else np.zeros(0, np.int64)
        elif name == "summary":
            w = want.summary if area else np.where(np.arange(8) == 5, 0, want.summary)
        else:
            w = getattr(want, name)
        assert w.shape[0] == size, name
        diff = got[name][:size] != w
        assert not diff.any(), "%s: %s differs at %d entries, first at %d: %r, not %r" % (
            what, name, int(diff.sum()), int(np.argmax(diff)), got[name][:size][diff][:4], w[diff][:4])
        assert (got[name][size:] == poison).all(), "%s: %s was written at or beyond %d" % (what, name, size)


@pytest.mark.parametrize("area", (True, False))
@pytest.mark.parametrize("name", BS.NAMES)
def test_boundary_on_the_bits(hip, dev, name, area):
    tri, sg, t, want = _case(name, hip)
    n = tri.shape[0]
    assert sg.stats()["n_tri"] == n
    _same(_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, area), want, n, area, name)
    if name in BS.COUNTS:
        assert (int(want.summary[0]), np.diff(want.loop_offsets).tolist(), int(want.summary[2])) == BS.COUNTS[name]


@pytest.mark.parametrize("name", ("strip", "strip_rev", "islands", "bunny", "half_fan300"))
def test_what_work_holds_means_nothing(hip, dev, name):
    tri, sg, t, want = _case(name, hip)
    n = tri.shape[0]
    for what, fill in (("zeros", 0), ("0xFF", -1), ("random", np.random.default_rng(BS.SEED + 11))):
        _same(_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, True, work_fill=fill), want, n, True, "%s work=%s" % (name, what))
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    a1 = _raw(hip.lib, sg, n, dev, t.twin, t.edge_class, True, work_fill=-1, stream=s1, sync=False)
    a2 = _raw(hip.lib, sg, n, dev, t.twin, t.edge_class, True, work_fill=0, stream=s2, sync=False)
    torch.cuda.synchronize()
    r1, r2 = a1(), a2()
    _same(r1, want, n, True, "%s on a side stream" % name)
    assert all(np.array_equal(r1[k], r2[k]) for k in r1)


@pytest.mark.parametrize("name", ("strip", "dead", "bunny"))
def test_arrays_that_are_no_topology(hip, dev, name):
    """B2 as a contract: whatever twin and edge_class hold, the call answers as the restatement does on the same arrays, reads nothing
    out of bounds and leaves the poison round every output"""
    tri, sg, t, _ = _case(name, hip)
    n = tri.shape[0]
    H = 3 * n
    rng = np.random.default_rng(BS.SEED + 13)
    i32 = np.int32
    k = max(H // 100, 2)
    cases = []
    cases.append(("random", rng.integers(-2 ** 31, 2 ** 31 - 1, H).astype(i32), rng.integers(0, 256, H).astype(np.uint8)))
    cases.append(("random twin in range, classes 1 and 2", rng.integers(0, H, H).astype(i32), rng.choice(np.array([1, 2, 2, 2], np.uint8), H)))
    p = rng.permutation(H)                                                     # mutual pairs at random: long walks, cycles of any shape
    tw = np.empty(H, i32)
    tw[p[0::2][:H // 2]], tw[p[1::2][:H // 2]] = p[1::2][:H // 2], p[0::2][:H // 2]
    tw[p[2 * (H // 2):]] = -1
    cases.append(("random pairs", tw, rng.choice(np.array([1, 2, 2, 2, 2], np.uint8), H)))
    tw = t.twin.copy()
    tw[rng.integers(0, H, k)] = rng.integers(-5, H + 5, k)
    cases.append(("1 % of twin overwritten", tw, t.edge_class))
    tw = t.twin.copy()
    tw[rng.integers(0, H, k)] = rng.choice(i32([-2 ** 31, 2 ** 31 - 1, H, -1, -2]), k)
    cases.append(("twin INT32_MIN / INT32_MAX", tw, t.edge_class))
    cl = t.edge_class.copy()
    cl[rng.integers(0, H, k)] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 255], np.uint8), k)
    cases.append(("1 % of edge_class overwritten", t.twin, cl))
    cases.append(("all BOUNDARY", t.twin, np.ones(H, np.uint8)))
    for i, (what, tw, cl) in enumerate(cases):
        want = BE.boundary(tri, tw, cl)
        _same(_raw(hip.lib, sg, n, dev, tw, cl, i % 3 != 2), want, n, i % 3 != 2, "%s: %s" % (name, what))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN (the normal of a fan triangle along a straight rim: the sign and payload that x86 and the
    device give the NaN of 0 * inf are not pinned, as in tests/test_gpu_weld.py)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()


def _cap_raw(lib, sg, tri, dev, b, stream=None):
    n = tri.shape[0]
    H = 3 * n
    full = lambda x, size, dt, fill: _g(np.concatenate([np.asarray(x, dt).ravel(), np.full(size - np.asarray(x).size, fill, dt)]), dev, dt)
    d_order, d_offsets = full(b.order, H, np.int32, POISON), full(b.loop_offsets, H + 1, np.int32, POISON)
    d_lflags = full(b.lflags, H, np.uint8, 1)                                  # beyond L it says CLOSED
    d_loop, d_pos, d_sum, d_tri = _g(b.loop, dev, np.int32), _g(b.pos, dev, np.int32), _g(b.summary, dev, np.int64), _g(tri, dev, np.float32)
    cap = torch.full((H + 1, 36), 12345.0, dtype=torch.float32, device=dev)
    valid = torch.full((H + ROOM,), POISON8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    d = lambda x: P(x.data_ptr())
    got = lib.ezrt_cap_rows_device(sg._h, d(d_tri), n, d(d_order), d(d_loop), d(d_pos), d(d_offsets), d(d_lflags), d(d_sum), d(cap), d(valid),
                                   P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_tri.cpu().numpy()), bits(tri))
    return cap.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("name", BS.NAMES)
def test_cap_on_the_bits(hip, dev, name):
    tri, sg, t, b = _case(name, hip)
    B = int(b.summary[0])
    want, want_valid = BE.cap(tri, b)
    cap, valid = _cap_raw(hip.lib, sg, tri, dev, b, torch.cuda.Stream(dev) if name == "tube" else None)
    assert np.array_equal(valid[:B], want_valid) and (valid[B:] == POISON8).all()
    assert same_rows(cap[:B], want) and (cap[B:] == 12345.0).all()   # rows at and beyond B are not touched
    lens = np.diff(b.loop_offsets)
    assert want_valid.sum() == (lens[(b.lflags & 1) != 0] - 2).clip(0).sum()
    if name == "bunny":
        assert want_valid.sum() == 34


@pytest.mark.parametrize("name", ("bunny", "tube", "cube_open"))
def test_boundary_cap_new_scene(hip, dev, name):
    """the loop this is for: boundary, cap, a new scene of the rows and the cap -- closed, consistently wound, orientable"""
    tri, sg, t, want = _case(name, hip)
    n = tri.shape[0]
    d_tri = torch.from_numpy(tri).to(dev)
    topo = query.mesh_topology(sg)
    assert not topo.closed and topo.summary.tolist()[2] == want.summary[0]
    b = query.mesh_boundary(sg, topo)
    assert b.closed and b.n_boundary == want.summary[0] and b.n_loops == want.summary[1]
    cap = query.cap_rows(sg, d_tri, b)
    n_cap = cap.shape[0]
    assert n_cap == b.n_boundary - 2 * b.n_loops and cap.dtype == torch.float32 and cap.shape[1] == 36
    if name == "bunny":
        assert n_cap == 34
    full = torch.cat([d_tri, cap]).cpu().numpy()
    assert same_rows(full, BE.capped(tri, want))
    whole = hip.scene_create(full, BS.proxy_nodes(n + n_cap))
    topo2 = query.mesh_topology(whole)
    assert topo2.closed and topo2.oriented and topo2.summary.tolist()[2] == 0 and topo2.summary.tolist()[4] == 0
    o = query.mesh_orient(whole, topo2, outward=False)
    pf = o.pflags.cpu().numpy()
    assert o.n_patch == topo2.summary.tolist()[6] and o.orientable and not (pf & (_abi.PATCH_OPEN | _abi.PATCH_NONORIENTABLE)).any()
    assert not bool(o.flip.any())
    b2 = query.mesh_boundary(whole, topo2)
    assert b2.n_boundary == 0 and b2.n_loops == 0 and b2.closed and b2.order.numel() == 0 and b2.loop_offsets.tolist() == [0]
    if name == "cube_open":
        cube = OS.rows("cube_pow2")
        tc = TE.topology(cube)
        ref = OE.orient(cube, tc.twin, tc.edge_class, False)
        assert o.vol6.tolist() == ref.vol6.tolist() and o.scale == ref.scale and query.patch_volume(o).tolist() == [64.0]
        assert query.loop_area(b).tolist() == [[0.0, 0.0, -16.0]]              # the hole, seen from +z, is run through clockwise


def test_the_wrappers(hip, dev):
    for name in ("lone", "grid_holes", "strip_rev", "pinched", "moebius", "dead", "tetra"):
        tri, sg, t, want = _case(name, hip)
        n = tri.shape[0]
        d_tri = torch.from_numpy(tri).to(dev)
        topo = query.mesh_topology(sg, components=False)
        for kw in ({}, {"topo": topo}, {"topo": topo, "area": False}, {"stream": torch.cuda.Stream(dev)}):
            b = query.mesh_boundary(sg, **kw)
            torch.cuda.synchronize()
            area = kw.get("area", True)
            assert b.next.dtype == b.loop.dtype == b.pos.dtype == b.order.dtype == b.loop_offsets.dtype == torch.int32 and b.lflags.dtype == torch.uint8
            assert tuple(b.next.shape) == (3 * n,) and b.n_boundary == want.summary[0] == b.order.shape[0] and b.n_loops == want.summary[1]
            for k in ("next", "loop", "pos", "order", "loop_offsets", "lflags"):
                assert np.array_equal(getattr(b, k).cpu().numpy(), getattr(want, k)), (name, k)
            assert b.closed is bool(want.summary[2] == want.summary[1]) and b.scale == (want.scale if area else 0)
            if area:
                assert b.area2.dtype == torch.int64 and np.array_equal(b.area2.cpu().numpy(), want.area2)
                assert np.array_equal(b.summary.cpu().numpy(), want.summary)
                la = query.loop_area(b)
                assert la.dtype == torch.float64 and np.array_equal(la.cpu().numpy(), BE.loop_area(want))
            else:
                assert b.area2 is None
        pts = query.boundary_points(b, d_tri)
        assert pts.dtype == torch.float32 and np.array_equal(bits(pts.cpu().numpy()), bits(tri[:, :9].reshape(-1, 3)[want.order]))
        wc, wv = BE.cap(tri, want)
        for kw in ({}, {"stream": torch.cuda.Stream(dev)}):
            cap = query.cap_rows(sg, d_tri, b, **kw)
            torch.cuda.synchronize()
            assert same_rows(cap.cpu().numpy(), wc[wv != 0])
        cut = b._replace(order=b.order.clone(), loop_offsets=b.loop_offsets.clone(), lflags=b.lflags.clone())   # tensors of their own, cut to size
        assert same_rows(query.cap_rows(sg, d_tri, cut).cpu().numpy(), wc[wv != 0])


def test_untouched_state(hip, bunny_small, dev):
    from ezrt_amd import scene as S
    from ezrt_amd import scenes, trace
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    b = query.mesh_boundary(sg)
    query.cap_rows(sg, torch.from_numpy(np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)).to(dev), b)
    torch.cuda.synchronize()
    assert b.n_boundary == 42 and (sg.counters(), sg.last_render_ms()) == before


def test_errors(hip, oracle, bunny_small, dev):
    tri, sg, t, want = _case("grid_holes", hip)
    lib = hip.lib
    n = tri.shape[0]
    H = 3 * n
    f = lib.ezrt_mesh_boundary_device
    wb = lib.ezrt_boundary_work_bytes(n)
    full = lambda k, dt: torch.full((k,), 5, dtype=dt, device=dev)
    bufs = dict(twin=_g(t.twin, dev, np.int32), edge_class=_g(t.edge_class, dev, np.uint8), next=full(H, torch.int32), loop=full(H, torch.int32),
                pos=full(H, torch.int32), order=full(H, torch.int32), loop_offsets=full(H + 1, torch.int32), lflags=full(H, torch.uint8),
                area2=full(3 * H, torch.int64), summary=full(8, torch.int64), work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    keys = list(bufs)
    outs = keys[2:-1]
    host = np.zeros(max(wb // 8 + 1, 36 * H), np.int64)
    torch.cuda.synchronize()
    hp = P(host.ctypes.data)

    def fa(**kw):
        args = [kw.get("s", sg._h)] + [kw[k] if k in kw else P(bufs[k].data_ptr()) for k in keys]
        return args + [kw.get("work_bytes", wb), None]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((bufs[k] == 5).all()) for k in outs)
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + keys:                                                     # any NULL pointer but area2's
        if k != "area2":
            assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in keys:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert not host.any() and untouched()
    # the cap
    g = lib.ezrt_cap_rows_device
    d = lambda x: P(x.data_ptr())
    pad = lambda x, size, dt: _g(np.concatenate([np.asarray(x, dt), np.zeros(size - len(x), dt)]), dev, dt)
    cb = dict(tri36=_g(tri, dev, np.float32), order=pad(want.order, H, np.int32), loop=_g(want.loop, dev, np.int32), pos=_g(want.pos, dev, np.int32),
              loop_offsets=pad(want.loop_offsets, H + 1, np.int32), lflags=pad(want.lflags, H, np.uint8), summary=_g(want.summary, dev, np.int64),
              cap=torch.full((H, 36), 5.0, dtype=torch.float32, device=dev), cap_valid=full(H, torch.uint8))
    ck = list(cb)

    def ga(**kw):
        return [kw.get("s", sg._h), kw.get("tri36", d(cb["tri36"])), kw.get("n_tri", n)] + [kw[k] if k in kw else d(cb[k]) for k in ck[1:]] + [None]
    for k in ["s"] + ck:
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
        if k != "s":
            assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    for bad in (n - 1, n + 1, 0, -1):
        assert g(*ga(n_tri=bad)) == EZRT_ERR_INVALID and b"n_tri" in lib.ezrt_last_error(), bad
    torch.cuda.synchronize()
    assert bool((cb["cap"] == 5.0).all()) and bool((cb["cap_valid"] == 5).all()) and not host.any()
    # the rejected calls left no HIP error behind: the next call works
    _same(_raw(lib, sg, n, dev, t.twin, t.edge_class, True), want, n, True, "after the rejected calls")
    # the wrappers
    with pytest.raises(TypeError):
        query.mesh_boundary(bunny_small.upload(oracle))
    with pytest.raises(ValueError):
        query.mesh_boundary(sg, area=1)
    topo = query.mesh_topology(sg, components=False)
    with pytest.raises(TypeError):
        query.mesh_boundary(sg, topo._replace(twin=topo.twin.to(torch.int64)))
    with pytest.raises(TypeError):
        query.mesh_boundary(sg, topo._replace(edge_class=topo.edge_class.cpu()))
    with pytest.raises(ValueError):
        query.mesh_boundary(sg, query.mesh_topology(_case("tetra", hip)[1]))
    b = query.mesh_boundary(sg, topo)
    rows = cb["tri36"]
    with pytest.raises(ValueError):
        query.cap_rows(sg, rows[:-1], b)
    with pytest.raises(TypeError):
        query.cap_rows(sg, rows.to(torch.float64), b)
    with pytest.raises(ValueError):
        query.cap_rows(sg, rows, b._replace(order=b.order[:-1]))
    with pytest.raises(TypeError):
        query.cap_rows(sg, rows, b._replace(loop=b.loop.to(torch.int64)))
    with pytest.raises(TypeError):
        query.cap_rows(sg, rows, None)
    with pytest.raises(ValueError):
        query.boundary_points(b, rows[:-1])

"""Plane loops on device tensors (include/ezrt_plane_loops.h, ezrt_amd/query.py: plane_loops, plane_loops_of, loop_measures).

Every integer output -- next, order, plane_loops, loop_offsets, closed -- is compared EXACTLY with tests/plane_loops_expected.py, the
header's rule restated with dictionaries and held to its properties by tests/test_plane_loops_expected.py; there is no tolerance:

* the five scenes of tests/plane_scenes.py with its planes, over poisoned buffers with room behind them: what the call must not
  touch still holds the poison; tile_rows at the library's choice, 8, 64 and 2^30 (clamped): the same bits, and with 8 the Bunny's
  planes of up to 341 rows take the route through global memory;
* a generated ring of 10 000 rows per plane in shuffled order (one closed loop, beyond any tile, 14 rounds) and the same ring with
  a triangle removed (one open chain that starts behind the gap);
* batches of 1 .. 200 planes, a [2, 3, 4] shape, n == 0; a section capacity of total - 1; loop capacities 0, L - 1, L, L + 5;
  next = NULL and closed = NULL; offsets that no count call writes;
* the call twice and on two streams, behind a section on the same stream, after a refit, beside a render call with untouched
  counters, the error contract, the wrappers end to end, loop_measures on the voxel solid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import plane_expected as PE  # noqa: E402
import plane_loops_expected as LE  # noqa: E402
import plane_scenes as PS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = PS.GPU_NAMES
P = C.c_void_p
POISON = -7
POISON8 = 249                                                                  # ... of the uint8 output
ROOM = 8                                                                       # entries behind every output, so that a stray store shows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _case(name, hip, bunny_small, dev):
    """(tri, planes, the device scene, the DEVICE's section (offsets, seg) as tensors and as numpy, the restatement's loops of it),
    computed once and shared"""
    if name not in _cache:
        tri, nodes, planes, kind = PS.inputs(name, bunny_small)
        sg = hip.scene_create(tri, nodes)
        o, t, s = query.plane_section(sg, _gpu(planes, dev))
        torch.cuda.synchronize()
        on, sn = o.cpu().numpy(), s.cpu().numpy()
        _cache[name] = (tri, planes, sg, o, s, on, sn, LE.loops(on, sn, tri.shape[0]))
    return _cache[name]


def _raw(lib, sg, off_t, seg_t, capacity=None, tile_rows=0, loop_capacity=None, want_next=True, want_closed=True):
    """the C call itself over poisoned buffers: dict of numpy arrays, each with ROOM entries behind its stated size"""
    dev = off_t.device
    n = off_t.shape[0] - 1
    cap = seg_t.shape[0] if capacity is None else capacity
    lcap = cap if loop_capacity is None else loop_capacity
    full = lambda k, dt: torch.full((k + ROOM,), POISON8 if dt == torch.uint8 else POISON, dtype=dt, device=dev)
    out = dict(next=full(cap, torch.int64), order=full(cap, torch.int64), plane_loops=full(n + 1, torch.int64),
               loop_offsets=full(lcap + 1, torch.int64), closed=full(lcap, torch.uint8))
    wb = lib.ezrt_plane_loops_work_bytes(cap)
    work = torch.full((wb // 8 + ROOM,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)   # what work holds means nothing
    got = lib.ezrt_plane_loops_device(sg._h, P(off_t.data_ptr()), n, P(seg_t.data_ptr()), cap, tile_rows,
                                      P(out["next"].data_ptr()) if want_next else None, P(out["order"].data_ptr()), P(out["plane_loops"].data_ptr()),
                                      lcap, P(out["loop_offsets"].data_ptr()), P(out["closed"].data_ptr()) if want_closed else None,
                                      P(work.data_ptr()), wb, None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((work[wb // 8:] == 0x5A5A5A5A5A5A5A5A).all())                  # nothing behind the stated bytes of work
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["cap"], res["lcap"] = cap, lcap
    return res


def _same(got, want, what="", want_next=True, want_closed=True):
    """every output against the restatement's, and the poison wherever the call must not write"""
    cap, lcap = got["cap"], got["lcap"]
    nxt = np.where(want.next == -9, POISON, want.next) if want_next else np.full(cap, POISON)
    assert np.array_equal(got["next"][:cap], nxt), "%s: next differs, first at row %d" % (what, int(np.argmax(got["next"][:cap] != nxt)))
    R, L = want.order.size, want.closed.size
    assert np.array_equal(got["order"][:R], want.order), "%s: order differs, first at %d" % (what, int(np.argmax(got["order"][:R] != want.order)))
    assert (got["order"][R:] == POISON).all() and (got["next"][cap:] == POISON).all(), what
    assert np.array_equal(got["plane_loops"][:-ROOM], want.plane_loops) and (got["plane_loops"][-ROOM:] == POISON).all(), what
    k = min(L, lcap)
    assert np.array_equal(got["loop_offsets"][:k], want.loop_offsets[:k]), what
    if L <= lcap:
        assert got["loop_offsets"][L] == want.loop_offsets[L] == R and (got["loop_offsets"][L + 1:] == POISON).all(), what
    else:
        assert (got["loop_offsets"][k:] == POISON).all(), what                # the overflow shows in plane_loops[n] alone
    closed = want.closed[:k] if want_closed else np.full(k, POISON8, np.uint8)
    assert np.array_equal(got["closed"][:k], closed) and (got["closed"][k:] == (POISON8)).all(), what


@pytest.mark.parametrize("name", NAMES)
def test_loops_on_the_bits(hip, bunny_small, dev, name):
    tri, planes, sg, o, s, on, sn, want = _case(name, hip, bunny_small, dev)
    tile_max = _abi.plane_loops_limits()
    rows = np.diff(on)
    assert want.order.size > 100 and want.closed.size > 10
    for tile_rows in (0, 8, 64, 2 ** 30):
        _same(_raw(hip.lib, sg, o, s, tile_rows=tile_rows), want, "%s tile_rows=%d" % (name, tile_rows))
        eff = tile_max if tile_rows in (0, 2 ** 30) else tile_rows
        if tile_rows == 8:
            assert (rows > eff).sum() > 20                                      # planes on the global route
        assert tile_rows == 8 or (rows[rows > 0] <= eff).any()                 # ... and planes in LDS
    if name == "bunny":
        assert rows.max() == 341
    if name == "voxel_solid":
        assert want.closed.all()
    if name == "nasty":
        assert LE.multiplicity(on, sn) > 100 and not want.closed.any()
    if name == "open_solid":
        assert 0 < want.closed.sum() < want.closed.size


def _prism(n_sides):
    """the wall of an n-sided prism between z = 0 and z = 1: 2 n triangles, vertices [2 n, 3, 3], in the order of the sides"""
    th = 2 * np.pi * np.arange(n_sides) / n_sides
    xy = np.stack([np.cos(th), np.sin(th)], 1).astype(np.float32)
    b = np.concatenate([xy, np.zeros((n_sides, 1), np.float32)], 1)
    t = np.concatenate([xy, np.ones((n_sides, 1), np.float32)], 1)
    b1, t1 = np.roll(b, -1, 0), np.roll(t, -1, 0)
    return np.stack([np.stack([b, b1, t1], 1), np.stack([b, t1, t], 1)], 1).reshape(-1, 3, 3)


def _ring(n_sides, seed, drop=None):
    """the prism's triangles in shuffled order; drop: the position (before the shuffle) of a triangle that is left out"""
    V = _prism(n_sides)
    perm = np.random.default_rng(seed).permutation(V.shape[0])
    if drop is not None:
        perm = perm[perm != drop]
    return V[perm]


_rings = {}


def _ring_scene(hip, drop):
    if drop not in _rings:
        V = _ring(5000, 27, drop)
        tri, nodes = IS.build(IS.tri36(V))                                     # (the scene gives n_tri; the loops read no geometry)
        _rings[drop] = (V, hip.scene_create(tri, nodes))
    return _rings[drop]


def test_a_ring_longer_than_any_tile(hip, dev):
    planes = np.float32([[0, 0, 1, 0.25], [0, 0, -2, -1.5]])
    V, sg = _ring_scene(hip, None)
    on, ids, sn, _ = PE.section(planes, V)                                     # the section of the SHUFFLED triangles, uploaded
    assert list(on) == [0, 10000, 20000] and _abi.plane_loops_limits() < 10000 and sg.stats()["n_tri"] == 10000
    want = LE.loops(on, sn, 10000)
    assert list(want.plane_loops) == [0, 1, 2] and list(want.loop_offsets) == [0, 10000, 20000] and want.closed.all()
    assert (want.next[:10000] == np.arange(10000) + 1).mean() < 0.01           # chain order is unrelated to row order
    o, s = _gpu(on, dev, np.int64), _gpu(sn, dev)
    for tile_rows in (0, 64):
        _same(_raw(hip.lib, sg, o, s, tile_rows=tile_rows), want, "ring tile_rows=%d" % tile_rows)
    # one triangle less: an open chain per plane, whose head is the row behind the gap
    drop = 4321
    missing_q1 = LE.bits(PE.section(planes, _prism(5000)[drop:drop + 1])[2])[:, 1]   # the missing triangle's rows, one per plane
    Vg, sgg = _ring_scene(hip, drop)
    og, _, sgn, _ = PE.section(planes, Vg)
    assert list(og) == [0, 9999, 19998] and sgg.stats()["n_tri"] == 9999
    wg = LE.loops(og, sgn, 9999)
    assert list(wg.plane_loops) == [0, 1, 2] and list(wg.loop_offsets) == [0, 9999, 19998] and not wg.closed.any()
    heads = wg.order[wg.loop_offsets[:2]]
    assert np.array_equal(LE.bits(sgn)[heads, 0], missing_q1)                     # the head starts where the missing segment ended
    _same(_raw(hip.lib, sgg, _gpu(og, dev, np.int64), _gpu(sgn, dev)), wg, "ring with a gap")


def test_batch_sizes_and_shapes(hip, bunny_small, dev):
    for name in ("nasty", "voxel_solid"):
        tri, planes, sg, o, s, on, sn, want = _case(name, hip, bunny_small, dev)
        for n in (1, 63, 64, 65, 200):
            sel = np.arange(n) * 7 % planes.shape[0]                           # misses and planes that are not live among them
            oo, tt, ss = query.plane_section(sg, _gpu(planes[sel], dev))
            torch.cuda.synchronize()
            w = LE.loops(oo.cpu().numpy(), ss.cpu().numpy(), tri.shape[0])
            assert n < 63 or (np.diff(w.plane_loops) == 0).any()
            _same(_raw(hip.lib, sg, oo, ss), w, "%s n=%d" % (name, n))
        lead = planes[10:34].reshape(2, 3, 4, 4)
        got = query.plane_loops(sg, _gpu(lead, dev))
        oo, tt, ss = query.plane_section(sg, _gpu(lead, dev))
        torch.cuda.synchronize()
        w = LE.loops(oo.cpu().numpy(), ss.cpu().numpy(), tri.shape[0])
        assert tuple(got.plane_loops.shape) == (25,) and np.array_equal(got.plane_loops.cpu().numpy(), w.plane_loops)
        assert np.array_equal(got.row.cpu().numpy(), w.order) and np.array_equal(got.loop_offsets.cpu().numpy(), w.loop_offsets)
        # n == 0: nothing is launched, nothing is written
        e = _raw(hip.lib, sg, o[:1], s)
        assert all((e[k] == (POISON8 if k == "closed" else POISON)).all() for k in ("next", "order", "plane_loops", "loop_offsets", "closed"))
        g = query.plane_loops(sg, torch.empty((0, 4), device=dev))
        assert list(g.plane_loops.cpu().numpy()) == [0] and list(g.loop_offsets.cpu().numpy()) == [0] and g.closed.shape[0] == 0
        assert tuple(g.row.shape) == (0,) and tuple(g.tri.shape) == (0,) and tuple(g.seg.shape) == (0, 2, 3)


def test_a_section_that_did_not_fit(hip, bunny_small, dev):
    tri, planes, sg, o, s, on, sn, want = _case("open_solid", hip, bunny_small, dev)
    total = int(on[-1])
    last = int(np.nonzero(np.diff(on) > 0)[0][-1])
    w = LE.loops(on, sn, tri.shape[0], capacity=total - 1)
    assert np.array_equal(w.plane_loops[:last + 1], want.plane_loops[:last + 1]) and w.order.size < want.order.size
    for tile_rows in (0, 8):
        got = _raw(hip.lib, sg, o, s, capacity=total - 1, tile_rows=tile_rows)
        _same(got, w, "capacity = total - 1")
        assert (got["next"][on[last]:] == POISON).all() and np.array_equal(got["next"][:on[last]], want.next[:on[last]])
    z = _raw(hip.lib, sg, o, s, capacity=0)                                    # no row counts: only the empty planes are chained
    _same(z, LE.loops(on, sn, tri.shape[0], capacity=0), "capacity = 0")
    assert not z["plane_loops"][:-ROOM].any() and z["loop_offsets"][0] == 0


def test_loop_capacity_and_null_outputs(hip, bunny_small, dev):
    for name in ("open_solid", "bunny"):
        tri, planes, sg, o, s, on, sn, want = _case(name, hip, bunny_small, dev)
        L = want.closed.size
        for lcap in (0, L - 1, L, L + 5):
            for tile_rows in (0, 8):
                _same(_raw(hip.lib, sg, o, s, loop_capacity=lcap, tile_rows=tile_rows), want, "%s loop_capacity=%d" % (name, lcap))
        _same(_raw(hip.lib, sg, o, s, want_next=False), want, "next = NULL", want_next=False)
        _same(_raw(hip.lib, sg, o, s, want_closed=False, loop_capacity=L - 1), want, "closed = NULL", want_closed=False)
        # the wrapper: given capacities never synchronise and return them; entries past the loops hold -1 and 0
        got = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=L + 5, want_next=True)
        torch.cuda.synchronize()
        assert np.array_equal(got.next.cpu().numpy(), want.next) and np.array_equal(got.order.cpu().numpy()[:want.order.size], want.order)
        assert np.array_equal(got.loop_offsets.cpu().numpy(), np.concatenate([want.loop_offsets, np.full(5, -1)]))
        assert np.array_equal(got.closed.cpu().numpy(), np.concatenate([want.closed, np.zeros(5, np.uint8)]))
        assert (got.order.cpu().numpy()[want.order.size:] == -1).all()
        short = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=L - 1)
        torch.cuda.synchronize()
        assert short.next is None and int(short.plane_loops[-1]) == L and np.array_equal(short.loop_offsets.cpu().numpy()[:L - 1], want.loop_offsets[:L - 1])
        assert int(short.loop_offsets[L - 1]) == -1


def test_offsets_that_no_count_call_writes(hip, bunny_small, dev):
    """L2's guard: planes whose offsets descend, are negative, lie beyond the capacity or span more than n_tri rows have no loops and
    keep their rows; the call returns 0.  The values are made so that the planes that stay chained keep their own rows."""
    for name in ("open_solid", "bunny"):
        tri, planes, sg, o, s, on, sn, want = _case(name, hip, bunny_small, dev)
        m, total = tri.shape[0], int(on[-1])
        bad = LE.hostile_offsets(on, total, m)
        ok = LE.chained(bad, total, m)
        assert list(np.nonzero(~ok)[0]) == [4, 5, 12, 13, 29, 30, 49, 50]
        w = LE.loops(bad, sn, m)
        for tile_rows in (0, 8):
            got = _raw(hip.lib, sg, _gpu(bad, dev, np.int64), s, tile_rows=tile_rows)
            _same(got, w, "%s hostile offsets" % name)
            assert (np.diff(got["plane_loops"][:-ROOM])[~ok] == 0).all()
            gone = np.concatenate([np.arange(on[i], on[i + 1]) for i in np.nonzero(~ok)[0]])
            assert gone.size > 50 and (got["next"][gone] == POISON).all()
        # every plane hostile: nothing but plane_loops (zeros) and loop_offsets[0] is written
        none = np.full_like(on, -3)
        none[::2] = total + 1
        got = _raw(hip.lib, sg, _gpu(none, dev, np.int64), s)
        assert not got["plane_loops"][:-ROOM].any() and got["loop_offsets"][0] == 0 and (got["loop_offsets"][1:] == POISON).all()
        assert (got["next"] == POISON).all() and (got["order"] == POISON).all() and (got["closed"] == (POISON8)).all()


def test_twice_and_on_two_streams(hip, bunny_small, dev):
    tri, planes, sg, o, s, on, sn, want = _case("bunny", hip, bunny_small, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    r1 = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=want.closed.size, want_next=True, stream=a)
    r2 = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=want.closed.size, want_next=True, tile_rows=8, stream=b)
    r3 = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=want.closed.size, want_next=True, stream=a.cuda_stream)
    torch.cuda.synchronize()
    for r in (r1, r2, r3):
        assert np.array_equal(r.next.cpu().numpy(), want.next) and np.array_equal(r.order.cpu().numpy()[:want.order.size], want.order)
        assert np.array_equal(r.plane_loops.cpu().numpy(), want.plane_loops) and np.array_equal(r.loop_offsets.cpu().numpy(), want.loop_offsets)
        assert np.array_equal(r.closed.cpu().numpy(), want.closed)


def test_stream_order_behind_a_section(hip, bunny_small, dev):
    tri, planes, sg, o, s, on, sn, want = _case("nasty", hip, bunny_small, dev)
    src = _gpu(planes, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                           # the planes are written on `side`, behind the sleep
    total = int(on[-1])
    oo, tt, ss = query.plane_section(sg, p, capacity=total, stream=side)        # no synchronisation
    got = query.plane_loops_of(sg, oo, ss, capacity=total, loop_capacity=want.closed.size, want_next=True, stream=side)
    side.synchronize()
    assert np.array_equal(got.next.cpu().numpy(), want.next) and np.array_equal(got.order.cpu().numpy()[:want.order.size], want.order)
    assert np.array_equal(got.loop_offsets.cpu().numpy(), want.loop_offsets) and np.array_equal(got.closed.cpu().numpy(), want.closed)


def _wrapper_same(got, off, ids, seg, w, what):
    assert np.array_equal(got.plane_loops.cpu().numpy(), w.plane_loops) and np.array_equal(got.loop_offsets.cpu().numpy(), w.loop_offsets), what
    assert np.array_equal(got.closed.cpu().numpy(), w.closed) and np.array_equal(got.row.cpu().numpy(), w.order), what
    assert np.array_equal(got.tri.cpu().numpy(), ids[w.order]) and np.array_equal(LE.bits(got.seg.cpu().numpy()), LE.bits(seg)[w.order]), what
    assert got.plane_loops.dtype == torch.int64 and got.closed.dtype == torch.uint8 and got.tri.dtype == torch.int32 and got.seg.dtype == torch.float32


def test_after_a_refit(hip, dev):
    v = IS.voxel_solid()
    tri, nodes = v["tri"], v["nodes"]
    planes, _ = PS.planes_for(tri, 3)
    moved = tri.copy()
    shift = np.float32([3, -5, 11])
    for k in range(3):
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + shift
    q = planes.copy()
    with np.errstate(all="ignore"):
        q[:, 3] = (2 * planes[:, 3].astype(np.float64) + planes[:, :3].astype(np.float64) @ shift).astype(np.float32)
    sg = hip.scene_create(tri, nodes)
    first = query.plane_loops(sg, _gpu(q, dev))
    off0, ids0, seg0, _ = PE.section(q, tri)
    _wrapper_same(first, off0, ids0, seg0, LE.loops(off0, seg0, tri.shape[0]), "before the refit")
    refit.refit(sg, moved)
    off, ids, seg, _ = PE.section(q, moved)
    w = LE.loops(off, seg, tri.shape[0])
    _wrapper_same(query.plane_loops(sg, _gpu(q, dev)), off, ids, seg, w, "after the refit")
    assert w.closed.size > 50 and w.closed.all() and not np.array_equal(off, off0)


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, planes, _, o, s, on, sn, want = _case("bunny", hip, bunny_small, dev)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0 and sg.stats()["n_tri"] >= tri.shape[0]
    query.plane_loops_of(sg, o, s, tile_rows=8)
    query.plane_loops(sg, _gpu(planes, dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.plane_loops_of(sg, o, s, capacity=int(on[-1]), loop_capacity=want.closed.size, want_next=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), alone.cpu().numpy().view(np.uint32))
    assert np.array_equal(got.next.cpu().numpy(), want.next) and np.array_equal(got.order.cpu().numpy()[:want.order.size], want.order)
    assert np.array_equal(got.loop_offsets.cpu().numpy(), want.loop_offsets) and np.array_equal(got.closed.cpu().numpy(), want.closed)


def test_end_to_end_and_measures(hip, bunny_small, dev):
    for name in ("voxel_solid", "open_solid"):
        tri, planes, sg, o, s, on, sn, want = _case(name, hip, bunny_small, dev)
        off, ids, seg, _ = PE.section(planes, tri)
        for kw in ({}, {"slices": 3, "tile_rows": 8}):
            _wrapper_same(query.plane_loops(sg, _gpu(planes, dev), **kw), off, ids, seg, want, "%s %r" % (name, kw))
    # two cubes touching along an edge: a key of multiplicity two
    tri, nodes = IS.build(IS.tri36(LE.two_cubes()[:, :9]))
    plane = np.float32([[0, 0, 1, 0.5]])
    off, ids, seg, _ = PE.section(plane, tri)
    w = LE.loops(off, seg, tri.shape[0])
    assert LE.multiplicity(off, seg) == 1 and w.closed.all()
    _wrapper_same(query.plane_loops(hip.scene_create(tri, nodes), _gpu(plane, dev)), off, ids, seg, w, "two cubes")
    # measures on the voxel solid: coordinates are small half-integers, every term and every sum is exact in float64
    tri, planes, sg, o, s, on, sn, want = _case("voxel_solid", hip, bunny_small, dev)
    z = np.float32([[0, 0, 1, 1.5], [0, 0, -1, -1.5], [0, 2, 0, 5], [1, 0, 0, 2.5]])
    off, ids, seg, _ = PE.section(z, tri)
    w = LE.loops(off, seg, tri.shape[0])
    zt = _gpu(z, dev)
    got = query.plane_loops(sg, zt)
    _wrapper_same(got, off, ids, seg, w, "axis planes")
    length, area = query.loop_measures(got, zt)
    torch.cuda.synchronize()
    wl, wa = LE.measures(w, seg, z)
    assert length.dtype == torch.float64 and tuple(length.shape) == tuple(area.shape) == (w.closed.size,)
    assert np.array_equal(length.cpu().numpy(), wl) and np.array_equal(area.cpu().numpy(), wa)
    assert wa[w.plane_loops[0]:w.plane_loops[1]].sum() == 8.0 == wa[w.plane_loops[1]:w.plane_loops[2]].sum()


def test_errors(hip, oracle, bunny_small, dev):
    tri, planes, sg, o, s, on, sn, want = _case("voxel_solid", hip, bunny_small, dev)
    lib = hip.lib
    n, cap, L = on.size - 1, int(on[-1]), want.closed.size
    f = lib.ezrt_plane_loops_device
    wb = lib.ezrt_plane_loops_work_bytes(cap)
    nxt = torch.zeros(cap, dtype=torch.int64, device=dev)
    order = torch.zeros(cap, dtype=torch.int64, device=dev)
    pl = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    lo = torch.zeros(L + 1, dtype=torch.int64, device=dev)
    cl = torch.zeros(L, dtype=torch.uint8, device=dev)
    work = torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev)
    host_i64, host_f, host_u8 = np.zeros(max(cap, n + 1, wb // 8) + 1, np.int64), np.zeros(cap * 6, np.float32), np.zeros(L, np.uint8)
    torch.cuda.synchronize()
    d = lambda t: P(t.data_ptr())
    hp = lambda a: P(a.ctypes.data)
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("offsets", d(o)), kw.get("n", n), kw.get("seg", d(s)), kw.get("capacity", cap),
                       kw.get("tile_rows", 0), kw.get("next", d(nxt)), kw.get("order", d(order)), kw.get("plane_loops", d(pl)),
                       kw.get("loop_capacity", L), kw.get("loop_offsets", d(lo)), kw.get("closed", d(cl)), kw.get("work", d(work)),
                       kw.get("work_bytes", wb), None]
    assert f(*fa()) == 0 and f(*fa(next=None, closed=None)) == 0 and f(*fa(capacity=0, seg=None, order=None, next=None)) == 0
    torch.cuda.synchronize()
    # work too small, or misaligned
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(work.data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    # negative counts
    assert f(*fa(n=-1)) == EZRT_ERR_INVALID and f(*fa(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert f(*fa(loop_capacity=-1)) == EZRT_ERR_INVALID and f(*fa(tile_rows=-1)) == EZRT_ERR_INVALID and b"tile_rows" in lib.ezrt_last_error()
    assert f(*fa(capacity=2 ** 62)) == EZRT_ERR_INVALID
    # NULL pointers
    for k in ("s", "offsets", "seg", "order", "plane_loops", "loop_offsets", "work"):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID, k
    # host memory is rejected, never read or written
    assert f(*fa(offsets=hp(host_i64))) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error()
    for k in ("next", "order", "plane_loops", "loop_offsets", "work"):
        assert f(*fa(**{k: hp(host_i64)})) == EZRT_ERR_INVALID, k
    assert f(*fa(seg=hp(host_f))) == EZRT_ERR_INVALID and f(*fa(closed=hp(host_u8))) == EZRT_ERR_INVALID
    assert not host_i64.any() and not host_f.any() and not host_u8.any()
    # n == 0 launches nothing
    pl.fill_(5), order.fill_(5), lo.fill_(5)
    assert f(*fa(n=0)) == 0
    torch.cuda.synchronize()
    assert bool((pl == 5).all()) and bool((order == 5).all()) and bool((lo == 5).all())
    # the rejected calls left no HIP error behind: the next call works
    _same(_raw(lib, sg, o, s), want, "after the rejected calls")
    # the wrappers
    with pytest.raises(ValueError):
        query.plane_loops_of(sg, o, s, capacity=cap + 1)
    with pytest.raises(ValueError):
        query.plane_loops_of(sg, o, s.reshape(-1, 6))
    with pytest.raises(TypeError):
        query.plane_loops_of(sg, o.to(torch.int32), s)
    with pytest.raises(TypeError):
        query.plane_loops_of(sg, o.cpu(), s)
    with pytest.raises(TypeError):
        query.plane_loops_of(bunny_small.upload(oracle), o, s)
    with pytest.raises(TypeError):
        query.plane_loops(bunny_small.upload(oracle), _gpu(planes, dev))
    with pytest.raises(ValueError):
        query.plane_loops(sg, torch.zeros((4, 3), device=dev))

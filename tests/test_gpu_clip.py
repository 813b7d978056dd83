"""Plane clipping on device tensors (include/ezrt_clip.h, ezrt_amd/query.py: clip_rows, cut_segments).

Every output of both calls -- offsets, summary; out, src, cut_edge -- is compared EXACTLY with tests/clip_expected.py, the header's rule
restated in numpy and held to its properties by tests/test_clip_expected.py.  There is no tolerance anywhere (a NaN normal is a NaN:
K5 leaves its sign and payload open).

* sizes that straddle wave, workgroup, fill tile, scan tile and the scan's second level, each under a plane that keeps everything, one
  that drops everything, one that cuts every row in two pieces and a generic one, over poisoned buffers with room behind them;
* the staged and the per-lane route of the fill (tri36 and out offset by one row, and by 4 bytes) give the same bits;
* capacity below T and offsets that no count call left: rows are whole or absent, nothing outside [0, capacity) is touched;
* `work` pre-filled with zeros, with 0xFF and with noise; two calls on two streams;
* six calls in a row trim the Bunny to a box;
* clip, a new scene, topology, boundary, cap, a new scene: closed, oriented, the volumes of the cube's halves, the torus's loops;
* the wrappers, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402
import clip_expected as CE  # noqa: E402
import clip_scenes as CS  # noqa: E402
import orient_scenes as OS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
F = np.float32
POISON = -7
POISON_F = 12345.0
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)
KEEP, DROP, TWO, GENERIC = "keeps everything", "drops everything", "two pieces of every row", "generic"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sg(hip):
    """a scene for the device and the error slot: the calls read none of its triangles"""
    return hip.scene_create(*OS.scene("cube_pow2", None))


_cache = {}


def _pool(bunny_small):
    """the rows of every scene of tests/clip_scenes.py in a seeded random order, so that a single row is as likely a NaN as a sliver"""
    if "pool" not in _cache:
        T = np.concatenate([CS.rows(name, bunny_small) for name in CS.NAMES])
        _cache["pool"] = np.ascontiguousarray(T[np.random.default_rng(CS.SEED + 21).permutation(T.shape[0])])
    return _cache["pool"]


def _case(bunny_small, n, what):
    """(rows [n, 36], plane [4], the restatement's Clip), computed once and shared"""
    key = (n, what)
    if key not in _cache:
        R = CS.resize(_pool(bunny_small), n)
        dead = CS.rows("dead")                                                 # NaN, infinities and degenerate rows at any size above 2
        for j in range(min(n // 3, dead.shape[0])):
            R[(7 * j + 1) % n] = dead[j]
        V = R[:, :9][np.isfinite(R[:, :9]).all(1)].reshape(-1, 3)
        far = float(np.abs(V).max()) * 3 + 10 if V.size else 10.0
        if what == KEEP:
            plane = F([0, 0, 1, -far])
        elif what == DROP:
            plane = F([0, 0, 1, far])
        elif what == TWO:
            R, plane = CS.two_piece_rows(R), F([0, 0, 1, 0])
        else:
            nrm = np.array([0.3, -0.2, 1.0])
            plane = np.append(nrm, np.median(V.astype(np.float64) @ nrm) if V.size else 0.0).astype(F)
        c = CE.clip(R, plane)
        fin = int(np.isfinite(R[:, :9]).all(1).sum())
        if what == KEEP:
            assert c.summary[1] == fin == c.summary[0]
        elif what == DROP:
            assert c.summary[0] == 0 and c.summary[3] == fin
        elif what == TWO:
            assert c.summary[0] == 2 * n and c.summary[2] == n                  # the output is twice the input
        _cache[key] = (R, plane, c)
    return _cache[key]


def _g(x, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _count(lib, sg, R, plane, dev, work_fill=FILL, stream=None, sync=True):
    """ezrt_clip_count_device over poisoned buffers with ROOM entries behind their stated size"""
    n = R.shape[0]
    d_rows = _g(np.concatenate([R, np.full((1, 36), 2.0, F)]), dev, F)          # a guard row that every plane here would keep
    d_plane = _g(plane, dev, F)
    offsets = torch.full((n + 1 + ROOM,), POISON, dtype=torch.int64, device=dev)
    summary = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_clip_work_bytes(n)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_clip_count_device(sg._h, P(d_rows.data_ptr()), n, P(d_plane.data_ptr()), P(offsets.data_ptr()), P(summary.data_ptr()),
                                     P(work.data_ptr()), wb, P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((work[wb // 8:] == tail).all())                            # nothing behind the stated bytes of work
        assert np.array_equal(CE.bits(d_rows[:n].cpu().numpy()), CE.bits(R))
        return offsets.cpu().numpy(), summary.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_count(got, c, n, what=""):
    offsets, summary = got
    assert np.array_equal(offsets[:n + 1], c.offsets), "%s: offsets differ first at %d" % (what, int(np.argmax(offsets[:n + 1] != c.offsets)))
    assert (offsets[n + 1:] == POISON).all() and np.array_equal(summary[:8], c.summary) and (summary[8:] == POISON).all(), what


def _fill(lib, sg, R, plane, offsets, capacity, dev, shift=0, ids=True, stream=None, sync=True, out_shift=None):
    """ezrt_clip_rows_device over poisoned buffers: tri36 starts `shift` floats and out `out_shift` floats (default: the same) into
    512-byte aligned allocations, and out, src and cut_edge have ROOM rows behind `capacity`.  Returns (out [capacity + ROOM, 36], src, cut_edge) as numpy arrays."""
    n = R.shape[0]
    oshift = shift if out_shift is None else out_shift
    d_in = torch.full((shift + n * 36 + 36,), 3.0, dtype=torch.float32, device=dev)
    d_in[shift:shift + n * 36] = _g(R, dev, F).reshape(-1)
    d_out = torch.full((oshift + (capacity + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    src = torch.full((capacity + ROOM,), POISON, dtype=torch.int32, device=dev)
    cut = torch.full((capacity + ROOM,), POISON, dtype=torch.int8, device=dev)
    d_plane = _g(plane, dev, F)
    d_off = _g(offsets, dev, np.int64)
    assert d_in.data_ptr() % 512 == 0 and d_out.data_ptr() % 512 == 0
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_clip_rows_device(sg._h, P(d_in.data_ptr() + 4 * shift), n, P(d_plane.data_ptr()), P(d_off.data_ptr()), capacity,
                                    P(d_out.data_ptr() + 4 * oshift), P(src.data_ptr()) if ids else None, P(cut.data_ptr()) if ids else None,
                                    P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((d_out[:oshift] == POISON_F).all()) and np.array_equal(CE.bits(d_in[shift:shift + n * 36].cpu().numpy().reshape(-1, 36)), CE.bits(R))
        return d_out[oshift:].cpu().numpy().reshape(-1, 36), src.cpu().numpy(), cut.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_fill(got, c, placed, capacity, ids=True, what=""):
    """`placed`: the (output row, piece) pairs of CE.candidates.  An output row with one candidate holds it; one with several (offsets
    that no count call left may send two source rows to one place, and which of them writes a word last is open) holds in every word
    the word of one of them; every other row holds the poison."""
    out, src, cut = got
    assert out.shape[0] == capacity + ROOM
    by_row = {}
    for r, p in placed:
        by_row.setdefault(r, []).append(p)
    assert all(0 <= r < capacity for r in by_row)
    rows = np.array(sorted(by_row), np.int64)
    single = np.array([len(by_row[r]) == 1 for r in rows], bool)
    one = rows[single]
    pc = np.array([by_row[r][0] for r in one], np.int64)
    bad = (CE.bits(out[one]) != CE.bits(c.out[pc])) & ~(np.isnan(out[one]) & np.isnan(c.out[pc]))
    assert not bad.any(), "%s: %d rows differ, first output row %d" % (what, int(bad.any(1).sum()), int(one[np.argmax(bad.any(1))]))
    if ids:
        assert np.array_equal(src[one], c.src[pc]) and np.array_equal(cut[one], c.cut_edge[pc]), what
    for r in rows[~single]:
        cand = c.out[by_row[r]]
        assert ((CE.bits(cand) == CE.bits(out[r])[None]) | (np.isnan(cand) & np.isnan(out[r])[None])).any(0).all(), (what, r)
        assert not ids or (src[r] in c.src[by_row[r]] and cut[r] in c.cut_edge[by_row[r]]), (what, r)
    rest = np.ones(capacity + ROOM, bool)
    rest[rows] = False
    assert (out[rest] == POISON_F).all(), "%s: a row that belongs to no source row was written" % what
    if ids:
        assert (src[rest] == POISON).all() and (cut[rest] == POISON).all(), what
    else:
        assert (src == POISON).all() and (cut == POISON).all(), what


@pytest.mark.parametrize("what", (KEEP, DROP, TWO, GENERIC))
@pytest.mark.parametrize("n", SIZES)
def test_clip_on_the_bits(hip, sg, dev, bunny_small, n, what):
    R, plane, c = _case(bunny_small, n, what)
    _same_count(_count(hip.lib, sg, R, plane, dev), c, n, "%d rows, %s" % (n, what))
    T = int(c.offsets[n])
    _same_fill(_fill(hip.lib, sg, R, plane, c.offsets, T, dev), c, [(r, r) for r in range(T)], T, True, "%d rows, %s" % (n, what))


@pytest.mark.parametrize("what", (KEEP, TWO, GENERIC))
@pytest.mark.parametrize("n", (257, 2049))
def test_both_routes_give_the_same_bits(hip, sg, dev, bunny_small, n, what):
    """one row in, tri36 and out are still 16-byte aligned and take the staged route; 4 bytes in they take the per-lane route, and so
    does a call with only one of the two off the 16 bytes"""
    R, plane, c = _case(bunny_small, n, what)
    T = int(c.offsets[n])
    all_rows = [(r, r) for r in range(T)]
    for shift, ids in ((36, True), (1, True), (37, False), (2, True), (3, True)):
        _same_fill(_fill(hip.lib, sg, R, plane, c.offsets, T, dev, shift=shift, ids=ids), c, all_rows, T, ids, "%d rows, %s, %d floats in" % (n, what, shift))
    for shift, oshift in ((0, 1), (3, 0), (36, 2), (1, 72)):                   # tri36 aligned and out not, and the other way round
        _same_fill(_fill(hip.lib, sg, R, plane, c.offsets, T, dev, shift=shift, out_shift=oshift), c, all_rows, T, True,
                   "%d rows, %s, tri36 %d and out %d floats in" % (n, what, shift, oshift))


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("what", (TWO, GENERIC))
def test_capacity_and_offsets_that_no_count_left(hip, sg, dev, bunny_small, what, shift):
    """K8: whatever offsets holds, a row is written whole or not at all and nothing outside [0, capacity) is touched"""
    n = 2049
    R, plane, c = _case(bunny_small, n, what)
    T = int(c.offsets[n])
    rng = np.random.default_rng(CS.SEED + 31)
    i64 = np.int64
    some = c.offsets.copy()
    k = rng.integers(0, n + 1, n // 20)
    some[k] = rng.choice(i64([-2 ** 63, 2 ** 63 - 1, -1, T, T + 1, 0, 1]), k.size)
    cases = [("capacity T - 1", c.offsets, T - 1), ("capacity T / 2", c.offsets, T // 2), ("capacity 1", c.offsets, 1), ("capacity 0", c.offsets, 0),
             ("negative", c.offsets - T - 5, T), ("descending", c.offsets[::-1].copy(), T), ("shifted by one", c.offsets + 1, T),
             ("shifted by one, room for it", c.offsets + 1, T + 1), ("random", rng.integers(-5, T + 5, n + 1).astype(i64), T),
             ("random bits", rng.integers(-2 ** 63, 2 ** 63 - 1, n + 1, dtype=i64), T), ("5 % overwritten", some, T),
             ("all zero", np.zeros(n + 1, i64), T), ("all INT64_MAX", np.full(n + 1, 2 ** 63 - 1, i64), T)]
    for name, off, cap in cases:
        placed = CE.candidates(c, off, cap)
        if name in ("capacity T / 2", "shifted by one, room for it", "5 % overwritten"):
            assert placed
        if name in ("negative", "capacity 0", "all INT64_MAX", "shifted by one"):
            assert len(placed) < T
        _same_fill(_fill(hip.lib, sg, R, plane, off, cap, dev, shift=shift), c, placed, cap, True, "%s, %s" % (what, name))


def test_what_work_holds_means_nothing_and_two_streams(hip, sg, dev, bunny_small):
    n = 4097
    R, plane, c = _case(bunny_small, n, GENERIC)
    T = int(c.offsets[n])
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(CS.SEED + 11))):
        _same_count(_count(hip.lib, sg, R, plane, dev, work_fill=fill), c, n, "work=%s" % what)
    R2, plane2, c2 = _case(bunny_small, 2049, TWO)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    a1 = _count(hip.lib, sg, R, plane, dev, work_fill=-1, stream=s1, sync=False)
    a2 = _count(hip.lib, sg, R2, plane2, dev, work_fill=0, stream=s2, sync=False)
    f1 = _fill(hip.lib, sg, R, plane, c.offsets, T, dev, stream=s1, sync=False)
    f2 = _fill(hip.lib, sg, R2, plane2, c2.offsets, 2 * 2049, dev, shift=1, stream=s2, sync=False)
    torch.cuda.synchronize()
    _same_count(a1(), c, n, "on a side stream")
    _same_count(a2(), c2, 2049, "on another side stream")
    _same_fill(f1(), c, [(r, r) for r in range(T)], T, True, "on a side stream")
    _same_fill(f2(), c2, [(r, r) for r in range(2 * 2049)], 2 * 2049, True, "on another side stream")


def test_six_calls_trim_the_bunny_to_a_box(hip, sg, dev, bunny_small):
    R = CS.rows("bunny", bunny_small)
    V = R[:, :9].reshape(-1, 3)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    planes = []                                                                # the middle half of the Bunny's box along every axis
    for axis in range(3):
        for sign, at in ((1.0, lo[axis] + 0.25 * (hi[axis] - lo[axis])), (-1.0, lo[axis] + 0.75 * (hi[axis] - lo[axis]))):
            p = np.zeros(4, F)
            p[axis], p[3] = sign, sign * at
            planes.append(p)
    want = np.array(R)
    rows = torch.from_numpy(want).to(dev)
    cut = 0
    for i, p in enumerate(planes):
        c = CE.clip(want, p)
        got = query.clip_rows(sg, rows, _g(p, dev, F) if i % 2 else [float(x) for x in p])
        torch.cuda.synchronize()
        assert got.n_rows == want.shape[0] and np.array_equal(got.summary.cpu().numpy(), c.summary)
        assert CE.same_rows(got.rows.cpu().numpy(), c.out) and np.array_equal(got.src.cpu().numpy(), c.src)
        assert np.array_equal(got.cut_edge.cpu().numpy(), c.cut_edge)
        assert np.array_equal(CE.bits(query.cut_segments(got).cpu().numpy()), CE.bits(CE.cut_segments(c)))
        cut += int(c.summary[2])
        want, rows = c.out, got.rows
    assert cut > 100 and 0 < want.shape[0] < R.shape[0]
    inside = want[:, :9].reshape(-1, 3)
    for p in planes:                                                           # P4's clamp: an axis plane is met exactly
        assert (inside.astype(np.float64) @ p[:3].astype(np.float64) >= np.float64(p[3])).all()


def _halves(hip, sg, dev, R, plane):
    """clip on the device, a new scene, topology, boundary, cap, a new scene: (clip, boundary of the clipped scene, its rows, the
    closed scene, its topology)"""
    d_rows = torch.from_numpy(np.array(R)).to(dev)
    clip = query.clip_rows(sg, d_rows, plane)
    want = CE.clip(R, F(plane))
    assert CE.same_rows(clip.rows.cpu().numpy(), want.out)
    n = clip.rows.shape[0]
    half = hip.scene_create(clip.rows.cpu().numpy(), BS.proxy_nodes(n))
    topo = query.mesh_topology(half)
    assert not topo.closed and topo.oriented
    b = query.mesh_boundary(half, topo)
    assert b.closed and b.n_loops >= 1 and b.n_boundary >= 3
    cap = query.cap_rows(half, clip.rows, b)
    full = torch.cat([clip.rows, cap])
    whole = hip.scene_create(full.cpu().numpy(), BS.proxy_nodes(full.shape[0]))
    topo2 = query.mesh_topology(whole)
    assert topo2.closed and topo2.oriented and topo2.summary.tolist()[6] == 1
    return clip, b, half, whole, topo2


@pytest.mark.parametrize("plane,volume", (((0, 0, 1, 1), 48.0), ((0, 0, -1, -1), 16.0)))
def test_the_halves_of_the_cube(hip, sg, dev, plane, volume):
    clip, b, half, whole, topo2 = _halves(hip, sg, dev, CS.rows("cube_pow2"), plane)
    assert b.n_loops == 1
    o = query.mesh_orient(whole, topo2, outward=True)
    assert o.n_patch == 1 and o.orientable and not bool(o.flip.any())
    assert not (o.pflags.cpu().numpy() & (_abi.PATCH_OPEN | _abi.PATCH_NONORIENTABLE | _abi.PATCH_INWARD)).any()
    assert query.patch_volume(o).tolist() == [volume]


@pytest.mark.parametrize("plane,loops", (((0.3, 0.2, 1, 0.1), None), ((0, 0, 1, 0), 2)))
def test_the_halves_of_the_torus(hip, sg, dev, plane, loops):
    R = CS.rows("torus32")
    clip, b, half, whole, topo2 = _halves(hip, sg, dev, R, plane)
    if loops is not None:
        assert b.n_loops == loops                                              # an annulus
    o = query.mesh_orient(whole, topo2, outward=True)
    assert o.n_patch == 1 and o.orientable and not bool(o.flip.any())
    assert not (o.pflags.cpu().numpy() & (_abi.PATCH_OPEN | _abi.PATCH_NONORIENTABLE | _abi.PATCH_INWARD)).any()
    # boundary_points of the clipped torus are plane_loops of the same plane on the torus, as cyclic sequences on the bits
    torus = hip.scene_create(np.array(R), BS.proxy_nodes(R.shape[0]))
    lp = query.plane_loops(torus, torch.tensor([plane], dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    assert bool(lp.closed.all()) and lp.closed.numel() == b.n_loops
    pts = query.boundary_points(b, clip.rows).cpu().numpy()
    assert CE.canonical_cycles(pts, b.loop_offsets.cpu().numpy()) == CE.canonical_cycles(lp.seg[:, 0].cpu().numpy(), lp.loop_offsets.cpu().numpy())


def test_the_wrappers(hip, sg, dev, bunny_small):
    for name in CS.NAMES:
        R = CS.rows(name, bunny_small)
        planes, kind = CS.planes(name, bunny_small, n_random=2, n_axis=1)
        d_rows = torch.from_numpy(np.array(R)).to(dev)
        for i, p in enumerate(planes[::2]):
            c = CE.clip(R, p)
            kw = ({}, {"stream": torch.cuda.Stream(dev)}, {"src": False})[i % 3]
            if "stream" in kw:
                kw["stream"].wait_stream(torch.cuda.current_stream(dev))
            got = query.clip_rows(sg, d_rows, _g(p, dev, F), **kw)
            torch.cuda.synchronize()
            assert isinstance(got, query.ClipRows) and got.n_rows == R.shape[0] and got.rows.dtype == torch.float32
            assert tuple(got.rows.shape) == (int(c.summary[0]), 36) and np.array_equal(got.summary.cpu().numpy(), c.summary), (name, p)
            assert CE.same_rows(got.rows.cpu().numpy(), c.out), (name, p)
            if kw.get("src", True):
                assert got.src.dtype == torch.int32 and got.cut_edge.dtype == torch.int8
                assert np.array_equal(got.src.cpu().numpy(), c.src) and np.array_equal(got.cut_edge.cpu().numpy(), c.cut_edge)
                seg = query.cut_segments(got)
                assert seg.dtype == torch.float32 and tuple(seg.shape) == (int(c.summary[5]), 2, 3)
                assert np.array_equal(CE.bits(seg.cpu().numpy()), CE.bits(CE.cut_segments(c)))
            else:
                assert got.src is None and got.cut_edge is None
    empty = query.clip_rows(sg, torch.zeros((0, 36), dtype=torch.float32, device=dev), (0, 0, 1, 0))
    assert tuple(empty.rows.shape) == (0, 36) and empty.summary.tolist() == [0] * 8 and empty.n_rows == 0 and empty.src.numel() == 0
    assert tuple(query.cut_segments(empty).shape) == (0, 2, 3)


def test_untouched_state(hip, bunny_small, dev):
    from ezrt_amd import scene as S
    from ezrt_amd import scenes, trace
    scn = bunny_small.upload(hip)
    tri = np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)
    rows, mid = torch.from_numpy(tri).to(dev), float(np.median(tri[:, 1]))     # (the inputs first: nothing but the call between the two reads)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    scn.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (scn.counters(), scn.last_render_ms())
    assert before[0]["rays"] > 0
    got = query.clip_rows(scn, rows, (0.0, 1.0, 0.0, mid))
    torch.cuda.synchronize()
    assert 0 < got.rows.shape[0] < 2 * rows.shape[0] and (scn.counters(), scn.last_render_ms()) == before


def test_errors(hip, sg, oracle, bunny_small, dev):
    lib = hip.lib
    n = 300
    R, plane, c = _case(bunny_small, 257, GENERIC)
    R = CS.resize(R, n)
    c = CE.clip(R, plane)
    T = int(c.offsets[n])
    wb = lib.ezrt_clip_work_bytes(n)
    full = lambda k, dt: torch.full((k,), 5, dtype=dt, device=dev)
    bufs = dict(tri36=_g(R, dev, F), plane4=_g(plane, dev, F), offsets=full(n + 1, torch.int64), summary=full(8, torch.int64),
                work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    host = np.zeros(max(36 * (n + T), 64), np.int64)
    hp = P(host.ctypes.data)
    torch.cuda.synchronize()
    f = lib.ezrt_clip_count_device
    d = lambda x: P(x.data_ptr())

    def fa(**kw):
        g = lambda k: kw[k] if k in kw else d(bufs[k])
        return [kw.get("s", sg._h), g("tri36"), kw.get("n_rows", n), g("plane4"), g("offsets"), g("summary"), g("work"), kw.get("work_bytes", wb), None]
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + list(bufs):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in bufs:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert f(*fa(n_rows=-1)) == EZRT_ERR_INVALID and f(*fa(n_rows=(2 ** 31 - 1) // 2 + 1, work_bytes=2 ** 40)) == EZRT_ERR_INVALID
    assert b"INT32_MAX / 2" in lib.ezrt_last_error()
    assert f(*fa(n_rows=0)) == 0                                               # launches nothing
    torch.cuda.synchronize()
    assert bool((bufs["offsets"] == 5).all()) and bool((bufs["summary"] == 5).all()) and not host.any()
    # the fill
    g = lib.ezrt_clip_rows_device
    fb = dict(tri36=bufs["tri36"], plane4=bufs["plane4"], offsets=_g(c.offsets, dev, np.int64), out=torch.full((T, 36), 5.0, dtype=torch.float32, device=dev),
              src=full(T, torch.int32), cut_edge=full(T, torch.int8))

    def ga(**kw):
        h = lambda k: kw[k] if k in kw else d(fb[k])
        return [kw.get("s", sg._h), h("tri36"), kw.get("n_rows", n), h("plane4"), h("offsets"), kw.get("capacity", T), h("out"), h("src"), h("cut_edge"), None]
    for k in ("s", "tri36", "plane4", "offsets", "out"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in fb:
        assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert g(*ga(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(capacity=2 ** 62)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(n_rows=-1)) == EZRT_ERR_INVALID and g(*ga(n_rows=(2 ** 31 - 1) // 2 + 1)) == EZRT_ERR_INVALID
    # out overlapping tri36: the same rows, rows that begin inside tri36, rows that end inside it
    both = torch.full((2 * n + T, 36), 5.0, dtype=torch.float32, device=dev)
    both[n:2 * n] = bufs["tri36"]
    torch.cuda.synchronize()
    at = lambda row: P(both.data_ptr() + 144 * row)
    for out_row, cap in ((n, T), (2 * n - 1, 1), (n - 1, 2), (n - T + 1 if T <= n else 0, T), (n, 1)):
        assert g(*ga(tri36=at(n), out=at(out_row), capacity=cap)) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error(), (out_row, cap)
    assert g(*ga(tri36=at(n), out=at(2 * n), capacity=T, src=None, cut_edge=None)) == 0   # behind it: no overlap
    assert g(*ga(tri36=at(n), out=at(n - 1), capacity=1, src=None, cut_edge=None)) == 0   # before it
    assert g(*ga(n_rows=0)) == 0 and g(*ga(capacity=0, out=None)) == 0
    torch.cuda.synchronize()
    assert bool((fb["out"] == 5.0).all()) and bool((fb["src"] == 5).all()) and bool((fb["cut_edge"] == 5).all()) and not host.any()
    first = c.out[:1] if CE.candidates(c, c.offsets, 1) else np.full((1, 36), 5.0, F)   # (a first row of two pieces does not fit capacity 1)
    assert CE.same_rows(both[2 * n:].cpu().numpy(), c.out) and CE.same_rows(both[n - 1:n].cpu().numpy(), first)
    # the rejected calls left no HIP error behind: the next call works
    _same_count(_count(lib, sg, R, plane, dev), c, n, "after the rejected calls")
    assert g(*ga(src=None, cut_edge=None)) == 0
    torch.cuda.synchronize()
    assert CE.same_rows(fb["out"].cpu().numpy(), c.out) and bool((fb["src"] == 5).all())
    # the wrappers
    rows = bufs["tri36"]
    with pytest.raises(TypeError):
        query.clip_rows(bunny_small.upload(oracle), rows, (0, 0, 1, 0))
    with pytest.raises(TypeError):
        query.clip_rows(sg, rows.cpu(), (0, 0, 1, 0))
    with pytest.raises(TypeError):
        query.clip_rows(sg, rows.to(torch.float64), (0, 0, 1, 0))
    with pytest.raises(ValueError):
        query.clip_rows(sg, rows[:, :35], (0, 0, 1, 0))
    with pytest.raises(ValueError):
        query.clip_rows(sg, rows.reshape(2, -1, 36), (0, 0, 1, 0))
    with pytest.raises(ValueError):
        query.clip_rows(sg, rows, (0, 0, 1))
    with pytest.raises(TypeError):
        query.clip_rows(sg, rows, torch.zeros(4, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        query.clip_rows(sg, rows, torch.zeros((1, 4), dtype=torch.float32, device=dev))
    with pytest.raises(TypeError):
        query.clip_rows(sg, rows, torch.zeros(4, dtype=torch.float32))

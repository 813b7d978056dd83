"""Mesh smoothing on device tensors (include/ezrt_smooth.h, ezrt_amd/query.py: smooth_rows).

Every float of out and every entry of the summary is compared EXACTLY with tests/smooth_expected.py, the header's rule restated in
numpy and held to its properties by tests/test_smooth_expected.py.  There is no tolerance anywhere (a NaN is a NaN).

* Taubin's pair at sizes that straddle wave, workgroup, fill tile and the LDS route's tile_rows_max, for 1, 2, 3 and 7 steps and both
  flag values, over poisoned buffers with room behind them; the arrays come from mesh_topology and mesh_weld on a scene of the rows;
* the LDS route against the global route (tile_rows 0, 1 and tile_rows_max) and the staged fill against the per-lane fill (tri36 and
  out offset by 4 bytes) give the same bits; in place (out == tri36) gives the bits of the out-of-place call on both fill routes;
* `work` pre-filled with zeros, with 0xFF and with noise; two calls on two streams; corrupted arrays match the restatement;
* chains: smooth, a scene of the rows, topology and weld on it: the closed scenes stay closed 2-manifolds with the same counts, the
  isosurface of a sphere stays closed, oriented and outward;
* the wrapper, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from ezrt_amd import _abi, query, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402
import orient_scenes as OS  # noqa: E402
import smooth_expected as SM  # noqa: E402
import smooth_scenes as MS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
F = np.float32
POISON = -7
POISON_F = 12345.0
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A
LAM, MU = MS.TAUBIN
ARRAYS = ("edge_class", "vertex", "star_offsets", "star", "vert_flags")
DTYPES = dict(edge_class=np.uint8, vertex=np.int32, star_offsets=np.int32, star=np.int32, vert_flags=np.uint8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sg(hip):
    """a scene for the device and the error slot: the calls read none of its triangles"""
    return hip.scene_create(*OS.scene("cube_pow2", None))


@pytest.fixture(scope="module")
def tile_max(hip):
    t = _abi.smooth_limits()
    assert t >= 64
    return t


_cache = {}


def _g(x, dev, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev)


def _padded(x, size, dtype):
    out = np.zeros(size, dtype)
    x = x.reshape(-1).cpu().numpy()
    out[:x.size] = x
    return out


def _device_arrays(hip, R):
    """the five arrays at their full sizes, from mesh_topology and mesh_weld on a scene of the rows R; what the weld leaves untouched is
    zero here.  Also the two results, for the wrapper."""
    n = R.shape[0]
    scene = hip.scene_create(np.array(R), BS.proxy_nodes(n))
    topo = query.mesh_topology(scene, components=False)
    weld = query.mesh_weld(scene)
    torch.cuda.synchronize()
    a = dict(edge_class=_padded(topo.edge_class, 3 * n, np.uint8), vertex=_padded(weld.vertex, 3 * n, np.int32),
             star_offsets=_padded(weld.star_offsets, 3 * n + 1, np.int32), star=_padded(weld.star, 3 * n, np.int32),
             vert_flags=_padded(weld.vert_flags, 3 * n, np.uint8))
    return a, topo, weld


def _case(hip, n):
    """(rows [n, 36], the five arrays), computed once and shared"""
    if n not in _cache:
        R = MS.sized(n)
        _cache[n] = (R, _device_arrays(hip, R)[0])
    return _cache[n]


def _want(hip, n, steps, flags=0, lam=LAM, mu=MU):
    """the restatement's (out, summary) of _case(n), computed once and shared"""
    key = ("want", n, steps, flags, lam, mu)
    if key not in _cache:
        R, a = _case(hip, n)
        _cache[key] = SM.smooth(R, steps=steps, lam=lam, mu=mu, flags=flags, **a)[:2]
    return _cache[key]


def _run(lib, sg, R, arrays, dev, steps=1, lam=LAM, mu=MU, flags=0, tile_rows=0, shift=0, out_shift=None, in_place=False, work_fill=FILL,
         stream=None, sync=True):
    """ezrt_smooth_rows_device over poisoned buffers: tri36 starts `shift` floats and out `out_shift` floats (default: the same) into
    512-byte aligned allocations; out has ROOM rows, summary and work ROOM words behind their stated sizes.  in_place: out is tri36.
    Returns (out [n + ROOM, 36], summary [8 + ROOM]) as numpy arrays."""
    n = R.shape[0]
    oshift = shift if out_shift is None else out_shift
    d_in = torch.full((shift + (n + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    d_in[shift:shift + n * 36] = _g(R, dev, F).reshape(-1)
    d_out = d_in if in_place else torch.full((oshift + (n + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    if in_place:
        oshift = shift
    summary = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_smooth_work_bytes(n)
    assert wb % 8 == 0 and wb == SM.work_bytes(n) and wb <= lib.ezrt_weld_work_bytes(n)
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    d_arr = [_g(arrays[k], dev, DTYPES[k]) for k in ARRAYS]
    assert d_in.data_ptr() % 512 == 0 and d_out.data_ptr() % 512 == 0
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_smooth_rows_device(sg._h, P(d_in.data_ptr() + 4 * shift), n, *[P(x.data_ptr()) for x in d_arr], steps, lam, mu, flags, tile_rows,
                                      P(d_out.data_ptr() + 4 * oshift), P(summary.data_ptr()), P(work.data_ptr()), wb,
                                      P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((work[wb // 8:] == tail).all())                            # nothing behind the stated bytes of work
        assert bool((d_out[:oshift] == POISON_F).all())
        if not in_place:
            assert np.array_equal(SM.bits(d_in[shift:shift + n * 36].cpu().numpy().reshape(-1, 36)), SM.bits(R))
            assert bool((d_in[shift + n * 36:] == POISON_F).all()) and bool((d_in[:shift] == POISON_F).all())
        for k, x in zip(ARRAYS, d_arr):
            assert np.array_equal(x.cpu().numpy(), arrays[k]), k                # the arrays are read only
        return d_out[oshift:].cpu().numpy().reshape(-1, 36), summary.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same(got, want, n, what=""):
    out, summary = got
    w_out, w_sum = want
    assert out.shape[0] == n + ROOM
    bad = (SM.bits(out[:n]) != SM.bits(w_out)) & ~(np.isnan(out[:n]) & np.isnan(w_out))
    assert not bad.any(), "%s: %d output rows differ, first %d (float %d)" % (what, int(bad.any(1).sum()), int(np.argmax(bad.any(1))),
                                                                              int(np.argmax(bad[np.argmax(bad.any(1))])))
    assert (out[n:] == POISON_F).all(), "%s: a row beyond n_rows was written" % what
    assert np.array_equal(summary[:8], w_sum) and (summary[8:] == POISON).all(), (what, summary[:8].tolist(), w_sum.tolist())


@pytest.mark.parametrize("n", MS.SIZES)
def test_smooth_on_the_bits(hip, sg, dev, n):
    R, a = _case(hip, n)
    for steps in MS.STEPS:
        for flags in (0, SM.PIN_BORDER):
            want = _want(hip, n, steps, flags)
            if n >= 255 and flags == 0:
                assert want[1][1] > 0 and want[1][2] > 0 and want[1][3] > 0 and want[1][4] > 0   # every rule is taken
            _same(_run(hip.lib, sg, R, a, dev, steps=steps, flags=flags), want, n, "%d rows, %d steps, flags %d" % (n, steps, flags))


@pytest.mark.parametrize("d", (-1, 0, 1))
def test_around_the_lds_tile(hip, sg, dev, tile_max, d):
    """tile_rows_max rows take the LDS route by default, one more takes the global one"""
    n = tile_max + d
    R, a = _case(hip, n)
    for steps in MS.STEPS:
        for flags in (0, SM.PIN_BORDER):
            _same(_run(hip.lib, sg, R, a, dev, steps=steps, flags=flags), _want(hip, n, steps, flags), n, "%d rows, %d steps, flags %d" % (n, steps, flags))


def test_sixty_four_steps(hip, sg, dev):
    n = 257
    R, a = _case(hip, n)
    want = _want(hip, n, 64)
    _same(_run(hip.lib, sg, R, a, dev, steps=64), want, n, "64 steps in LDS")
    _same(_run(hip.lib, sg, R, a, dev, steps=64, tile_rows=1), want, n, "64 steps, 64 launches")
    lam = _want(hip, n, 5, 0, 0.25, 0.25)                                      # the plain umbrella operator
    _same(_run(hip.lib, sg, R, a, dev, steps=5, lam=0.25, mu=0.25), lam, n, "mu == lambda")


def test_routes_give_the_same_bits(hip, sg, dev, tile_max):
    """the LDS route against the global route, the staged fill against the per-lane fill"""
    for n in (65, 257, tile_max):
        R, a = _case(hip, n)
        for steps in (1, 7):
            want = _want(hip, n, steps)
            for tile_rows in (0, 1, tile_max, n - 1, n, 2 ** 31 - 1):
                _same(_run(hip.lib, sg, R, a, dev, steps=steps, tile_rows=tile_rows), want, n, "%d rows, %d steps, tile_rows %d" % (n, steps, tile_rows))
    for n in (65, 2049):
        R, a = _case(hip, n)
        want = _want(hip, n, 3)
        for shift in (36, 1, 37, 2, 3):                                        # one row in is still 16-byte aligned; 4 bytes in is not
            _same(_run(hip.lib, sg, R, a, dev, steps=3, shift=shift), want, n, "%d rows, %d floats in" % (n, shift))
        for shift, oshift in ((0, 1), (3, 0), (36, 2), (1, 72)):               # tri36 aligned and out not, and the other way round
            _same(_run(hip.lib, sg, R, a, dev, steps=3, shift=shift, out_shift=oshift), want, n, "%d rows, tri36 %d and out %d floats in" % (n, shift, oshift))


@pytest.mark.parametrize("n", (65, 2049))
def test_in_place(hip, sg, dev, n):
    R, a = _case(hip, n)
    for steps in (1, 4):
        want = _want(hip, n, steps)
        for shift in (0, 1):                                                   # the staged and the per-lane fill
            for tile_rows in (0, 1):
                _same(_run(hip.lib, sg, R, a, dev, steps=steps, shift=shift, tile_rows=tile_rows, in_place=True), want, n,
                      "in place, %d rows, %d steps, %d floats in, tile_rows %d" % (n, steps, shift, tile_rows))


def test_what_work_holds_means_nothing_and_two_streams(hip, sg, dev):
    n = 4097
    R, a = _case(hip, n)
    want = _want(hip, n, 3)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(MS.SEED + 11))):
        _same(_run(hip.lib, sg, R, a, dev, steps=3, work_fill=fill), want, n, "work=%s" % what)
    R2, a2 = _case(hip, 257)
    want2 = _want(hip, 257, 7)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(MS.SEED + 12))):
        _same(_run(hip.lib, sg, R2, a2, dev, steps=7, work_fill=fill, shift=1), want2, 257, "work=%s, LDS route, per lane" % what)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    f1 = _run(hip.lib, sg, R, a, dev, steps=3, work_fill=-1, stream=s1, sync=False)
    f2 = _run(hip.lib, sg, R2, a2, dev, steps=7, work_fill=0, shift=1, stream=s2, sync=False)
    f3 = _run(hip.lib, sg, R2, a2, dev, steps=7, tile_rows=1, stream=s1, sync=False)
    torch.cuda.synchronize()
    _same(f1(), want, n, "on a side stream")
    _same(f2(), want2, 257, "on another side stream")
    _same(f3(), want2, 257, "behind the first")


def _corrupted(hip, n):
    """[(name, the five arrays with some of them damaged, the restatement's (out, summary))], computed once and shared"""
    key = ("corrupted", n)
    if key in _cache:
        return _cache[key]
    R, a = _case(hip, n)
    good = _want(hip, n, 3)
    H = 3 * n
    rng = np.random.default_rng(MS.SEED + 31)
    bad = np.array([-1, -2, H, H + 1, 2 ** 31 - 1, -2 ** 31, 0, 1, H - 1])
    cases = []
    for k in ("vertex", "star_offsets", "star"):
        some = a[k].copy()
        at = rng.integers(0, some.size, some.size // 20)
        some[at] = rng.choice(bad[:6] if k == "star_offsets" else bad, at.size)
        cases.append(("5 %% of %s overwritten" % k, {k: some}))
        if k != "star_offsets":
            cases.append(("%s random" % k, {k: rng.integers(-5, H + 5, a[k].size).astype(np.int32)}))
    lo = rng.integers(-5, H + 5, H + 1)                                        # short ranges anywhere: the stars of other vertices, or none
    cases.append(("star_offsets random", {"star_offsets": np.where(np.arange(H + 1) % 2, lo + rng.integers(-2, 9, H + 1), lo).astype(np.int32)}))
    for k in ("edge_class", "vert_flags"):
        some = a[k].copy()
        at = rng.integers(0, some.size, some.size // 20)
        some[at] = rng.integers(0, 256, at.size)
        cases.append(("5 %% of %s overwritten" % k, {k: some}))
        cases.append(("%s random" % k, {k: rng.integers(0, 4, a[k].size).astype(np.uint8)}))
    out = []
    for name, change in cases:
        b = dict(a)
        b.update(change)
        w = SM.smooth(R, steps=3, lam=LAM, mu=MU, **b)[:2]
        if name.startswith("5 %"):
            assert not np.array_equal(w[1], good[1]), name                      # the damage is seen
        out.append((name, b, w))
    _cache[key] = out
    return out


@pytest.mark.parametrize("shift,n", ((0, 2049), (1, 2049), (0, 257)))
def test_corrupted_arrays(hip, sg, dev, shift, n):
    """U2, U4: whatever the arrays hold, the answer is the restatement's and nothing out of bounds is touched"""
    R, a = _case(hip, n)
    for name, b, w in _corrupted(hip, n):
        _same(_run(hip.lib, sg, R, b, dev, steps=3, shift=shift), w, n, name)


@pytest.mark.parametrize("name", ("cube_pow2", "torus32"))
def test_closed_scenes_stay_closed_manifolds(hip, sg, dev, name):
    R = MS.rows(name)
    a, topo, weld = _device_arrays(hip, R)
    got = query.smooth_rows(sg, torch.from_numpy(np.array(R)).to(dev), topo, weld, steps=10, lam=LAM, mu=MU)
    torch.cuda.synchronize()
    want = SM.smooth(R, steps=10, lam=LAM, mu=MU, **a)
    rows = got.rows.cpu().numpy()
    assert SM.same_rows(rows, want[0]) and np.array_equal(got.summary.cpu().numpy(), want[1]) and want[1][1] == 3 * R.shape[0]
    scene = hip.scene_create(rows, BS.proxy_nodes(rows.shape[0]))
    t2, w2 = query.mesh_topology(scene), query.mesh_weld(scene)
    assert t2.summary.tolist()[:2] == topo.summary.tolist()[:2] and w2.n_vert == weld.n_vert and t2.closed and t2.oriented and w2.manifold_vertices
    assert query.euler_characteristic(w2, t2) == query.euler_characteristic(weld, topo)
    smooth = query.vertex_normals(scene, got.rows.clone(), w2)
    torch.cuda.synchronize()
    assert np.isfinite(smooth[:, 9:18].cpu().numpy()).all() and np.isfinite(rows).all()


def test_the_isosurface_chain(hip, sg, dev):
    V, g, R = MS.iso_sphere(13)
    iso = query.isosurface_rows(sg, torch.from_numpy(np.array(V, F)).to(dev), 0.0, (-1, -1, -1), 2.0 / 12)
    torch.cuda.synchronize()
    assert SM.same_rows(iso.rows.cpu().numpy(), R)
    n = R.shape[0]
    scene = hip.scene_create(np.array(R), BS.proxy_nodes(n))
    topo, weld = query.mesh_topology(scene), query.mesh_weld(scene)
    got = query.smooth_rows(scene, iso.rows, topo, weld, steps=6, lam=LAM, mu=MU)
    torch.cuda.synchronize()
    a = dict(edge_class=topo.edge_class.cpu().numpy(), vertex=weld.vertex.reshape(-1).cpu().numpy(), star_offsets=weld.star_offsets.cpu().numpy(),
             star=weld.star.cpu().numpy(), vert_flags=weld.vert_flags.cpu().numpy())
    want = SM.smooth(R, steps=6, lam=LAM, mu=MU, **a)
    rows = got.rows.cpu().numpy()
    assert SM.same_rows(rows, want[0]) and np.array_equal(got.summary.cpu().numpy(), want[1])
    scene2 = hip.scene_create(rows, BS.proxy_nodes(n))
    t2, w2 = query.mesh_topology(scene2), query.mesh_weld(scene2)
    assert t2.closed and t2.oriented and w2.n_vert == weld.n_vert and topo.closed
    orient = query.mesh_orient(scene2, t2, outward=True)
    torch.cuda.synchronize()
    assert orient.orientable and orient.summary.tolist()[4:6] == [0, 0] and not bool(orient.flip.any())   # no flip, no INWARD patch
    assert SM.shortest_edge(rows) > SM.shortest_edge(R)


def test_the_wrapper(hip, sg, dev, tile_max):
    for i, name in enumerate(MS.NAMES):
        R = MS.rows(name)
        n = R.shape[0]
        a, topo, weld = _device_arrays(hip, R)
        d_rows = torch.from_numpy(np.array(R)).to(dev)
        kw = ({}, {"stream": torch.cuda.Stream(dev)})[i % 2]
        if "stream" in kw:
            kw["stream"].wait_stream(torch.cuda.current_stream(dev))
        one = query.smooth_rows(sg, d_rows, topo, weld, **kw)                  # steps=1, lam=0.5, mu=None
        tb = query.smooth_rows(sg, d_rows, topo, weld, steps=4, lam=LAM, mu=MU, pin_border=bool(i & 2), tile_rows=(0, 1, tile_max)[i % 3], **kw)
        dst = torch.full((n, 36), POISON_F, dtype=torch.float32, device=dev)
        into = query.smooth_rows(sg, d_rows, topo, weld, steps=2, lam=0.25, out=dst, **kw)
        torch.cuda.synchronize()
        assert into.rows is dst
        for got, want in ((one, SM.smooth(R, steps=1, lam=0.5, mu=0.5, **a)), (into, SM.smooth(R, steps=2, lam=0.25, **a)),
                          (tb, SM.smooth(R, steps=4, lam=LAM, mu=MU, flags=SM.PIN_BORDER if i & 2 else 0, **a))):
            assert isinstance(got, query.SmoothRows) and got.n_rows == n and got.rows.dtype == torch.float32 and got.summary.dtype == torch.int64
            assert tuple(got.rows.shape) == (n, 36) and np.array_equal(got.summary.cpu().numpy(), want[1]), name
            assert SM.same_rows(got.rows.cpu().numpy(), want[0]), name
        assert np.array_equal(SM.bits(d_rows.cpu().numpy()), SM.bits(R))
        here = query.smooth_rows(sg, d_rows, topo, weld, steps=4, lam=LAM, mu=MU, out=d_rows, **kw)   # in place
        torch.cuda.synchronize()
        assert here.rows is d_rows and SM.same_rows(d_rows.cpu().numpy(), SM.smooth(R, steps=4, lam=LAM, mu=MU, **a)[0]), name
    none = lambda dtype, m=0: torch.zeros((m,), dtype=dtype, device=dev)
    topo0 = types.SimpleNamespace(edge_class=none(torch.uint8))
    weld0 = types.SimpleNamespace(vertex=none(torch.int32), star_offsets=none(torch.int32, 1), star=none(torch.int32), vert_flags=none(torch.uint8))
    empty = query.smooth_rows(sg, torch.zeros((0, 36), dtype=torch.float32, device=dev), topo0, weld0, steps=3, pin_border=True)
    assert tuple(empty.rows.shape) == (0, 36) and empty.summary.tolist() == [0] * 8 and empty.n_rows == 0


def test_untouched_state(hip, bunny_small, dev):
    from ezrt_amd import scene as S
    from ezrt_amd import trace
    scn = bunny_small.upload(hip)
    tri = np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)
    rows = torch.from_numpy(tri).to(dev)
    topo, weld = query.mesh_topology(scn, components=False), query.mesh_weld(scn)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    scn.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (scn.counters(), scn.last_render_ms())
    assert before[0]["rays"] > 0
    got = query.smooth_rows(scn, rows, topo, weld, steps=5, lam=LAM, mu=MU)
    torch.cuda.synchronize()
    assert got.rows.shape[0] == rows.shape[0] and (scn.counters(), scn.last_render_ms()) == before
    assert got.summary.tolist()[1] > 0 and got.summary.tolist()[2] > 0


def test_errors(hip, sg, oracle, bunny_small, dev):
    lib = hip.lib
    n = 300
    R = MS.sized(n)
    a, topo, weld = _device_arrays(hip, R)
    want = SM.smooth(R, steps=2, lam=LAM, mu=MU, **a)
    wb = lib.ezrt_smooth_work_bytes(n)
    bufs = dict(tri36=_g(R, dev, F), out=torch.full((n, 36), 5.0, dtype=torch.float32, device=dev),
                summary=torch.full((8,), 5, dtype=torch.int64, device=dev), work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    arr = {k: _g(a[k], dev, DTYPES[k]) for k in ARRAYS}
    host = np.zeros(36 * 2 * n, np.int64)
    hp = P(host.ctypes.data)
    torch.cuda.synchronize()
    f = lib.ezrt_smooth_rows_device
    d = lambda x: P(x.data_ptr())

    def fa(**kw):
        g = lambda k: kw[k] if k in kw else d(bufs[k] if k in bufs else arr[k])
        return [kw.get("s", sg._h), g("tri36"), kw.get("n_rows", n)] + [g(k) for k in ARRAYS] + [
            kw.get("steps", 2), kw.get("lam", LAM), kw.get("mu", MU), kw.get("flags", 0), kw.get("tile_rows", 0), g("out"), g("summary"), g("work"),
            kw.get("work_bytes", wb), None]
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID and b"ezrt_smooth_work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + list(bufs) + list(ARRAYS):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in list(bufs) + list(ARRAYS):                                        # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert f(*fa(n_rows=-1)) == EZRT_ERR_INVALID and b"n_rows < 0" in lib.ezrt_last_error()
    assert f(*fa(n_rows=(2 ** 31 - 1) // 3 + 1, work_bytes=2 ** 40)) == EZRT_ERR_INVALID and b"INT32_MAX / 3" in lib.ezrt_last_error()
    for steps in (0, -1, 1025, 2 ** 31 - 1):
        assert f(*fa(steps=steps)) == EZRT_ERR_INVALID and b"steps" in lib.ezrt_last_error(), steps
    for k in ("lam", "mu"):
        for x in (float("nan"), float("inf"), -float("inf")):
            assert f(*fa(**{k: x})) == EZRT_ERR_INVALID and b"not finite" in lib.ezrt_last_error(), (k, x)
    for flags in (2, 3, -1, 256):
        assert f(*fa(flags=flags)) == EZRT_ERR_INVALID and b"flags" in lib.ezrt_last_error(), flags
    assert f(*fa(tile_rows=-1)) == EZRT_ERR_INVALID and b"tile_rows" in lib.ezrt_last_error()
    assert f(*fa(n_rows=0)) == 0                                               # launches nothing
    torch.cuda.synchronize()
    assert bool((bufs["out"] == 5.0).all()) and bool((bufs["summary"] == 5).all()) and not host.any()
    # out overlapping tri36 in part: rows that begin inside tri36, rows that end inside it, a row or a float off
    both = torch.full((3 * n + 2, 36), 5.0, dtype=torch.float32, device=dev)
    both[n:2 * n] = bufs["tri36"]
    torch.cuda.synchronize()
    at = lambda row, off=0: P(both.data_ptr() + 144 * row + off)
    for out_row, off in ((n + 1, 0), (n - 1, 0), (2 * n - 1, 0), (1, 0), (n, 4), (n, -4)):
        assert f(*fa(tri36=at(n), out=at(out_row, off))) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error(), (out_row, off)
    torch.cuda.synchronize()
    assert bool((both[:n] == 5.0).all()) and bool((both[2 * n:] == 5.0).all()) and np.array_equal(SM.bits(both[n:2 * n].cpu().numpy()), SM.bits(R))
    assert f(*fa(tri36=at(n), out=at(0))) == 0 and f(*fa(tri36=at(n), out=at(2 * n))) == 0   # up to its first byte, from its last: no overlap
    torch.cuda.synchronize()
    assert SM.same_rows(both[:n].cpu().numpy(), want[0]) and SM.same_rows(both[2 * n:3 * n].cpu().numpy(), want[0]) and bool((both[3 * n:] == 5.0).all())
    assert f(*fa(tri36=at(n), out=at(n))) == 0                                 # the same rows exactly: in place
    torch.cuda.synchronize()
    assert SM.same_rows(both[n:2 * n].cpu().numpy(), want[0])
    bufs["summary"].fill_(5)
    # the rejected calls left no HIP error behind: the next call works
    assert f(*fa()) == 0
    torch.cuda.synchronize()
    assert SM.same_rows(bufs["out"].cpu().numpy(), want[0]) and np.array_equal(bufs["summary"].cpu().numpy(), want[1]) and not host.any()
    # the wrapper
    rows = bufs["tri36"]
    with pytest.raises(TypeError):
        query.smooth_rows(bunny_small.upload(oracle), rows, topo, weld)
    with pytest.raises(TypeError):
        query.smooth_rows(sg, rows.cpu(), topo, weld)
    with pytest.raises(TypeError):
        query.smooth_rows(sg, rows.to(torch.float64), topo, weld)
    with pytest.raises(TypeError):
        query.smooth_rows(sg, rows, topo, weld, out=torch.zeros((n, 36), dtype=torch.float64, device=dev))
    bad = [dict(steps=0), dict(steps=1025), dict(steps=2.0), dict(lam=float("nan")), dict(mu=float("inf")), dict(tile_rows=-1),
           dict(out=torch.zeros((n - 1, 36), dtype=torch.float32, device=dev)), dict(out=both[n - 1:2 * n - 1]),
           dict(out=torch.zeros((n, 72), dtype=torch.float32, device=dev)[:, :36])]
    for kw in bad:
        with pytest.raises(ValueError):
            query.smooth_rows(sg, both[n:2 * n], topo, weld, **kw)
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows[:, :35], topo, weld)
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows.reshape(2, -1, 36), topo, weld)
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows, None, weld)
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows, topo, None)
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows, topo, weld._replace(vert_flags=None, fans=None))   # a weld made with flags=False
    with pytest.raises(ValueError):
        query.smooth_rows(sg, rows[:100], topo, weld)                          # a topology of other rows

"""Subdivision on device tensors (include/ezrt_subdivide.h, ezrt_amd/query.py: subdivide_rows).

Every float of out and every entry of the summary is compared EXACTLY with tests/subdiv_expected.py, the header's rule restated in
numpy and held to its properties by tests/test_subdiv_expected.py.  There is no tolerance anywhere (a NaN is a NaN).

* both modes at sizes that straddle wave, workgroup and fill tile, and at one beyond which a workgroup takes a second tile, over
  poisoned buffers with room behind them; Loop mode takes its topology and weld from a scene of the same rows;
* the staged and the per-lane route of the fill (tri36 and out offset by one row, and by 4 bytes) give the same bits;
* `work` pre-filled with zeros, with 0xFF and with noise; two calls on two streams;
* corrupted twin, vertex, star_offsets and star match the restatement, and the run ends clean;
* chains: subdivide, a scene of the rows, topology and weld on it: the counts of a closed manifold on the cube and the torus, the
  Moebius band's FLIPPED edges, two Loop levels of the cube, the Bunny against scenes.subdivide, finite smooth normals;
* the wrapper, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402
import orient_scenes as OS  # noqa: E402
import subdiv_expected as SE  # noqa: E402
import subdiv_scenes as SS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
F = np.float32
POISON = -7
POISON_F = 12345.0
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A
MODES = (SE.MIDPOINT, SE.LOOP)
ARRAYS = ("twin", "edge_class", "vertex", "star_offsets", "star", "vert_flags")
DTYPES = dict(twin=np.int32, edge_class=np.uint8, vertex=np.int32, star_offsets=np.int32, star=np.int32, vert_flags=np.uint8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sg(hip):
    """a scene for the device and the error slot: the calls read none of its triangles"""
    return hip.scene_create(*OS.scene("cube_pow2", None))


_cache = {}


def _g(x, dev, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev)


def _padded(x, size, dtype):
    out = np.zeros(size, dtype)
    x = x.reshape(-1).cpu().numpy()
    out[:x.size] = x
    return out


def _device_arrays(hip, R):
    """the six arrays of Loop mode at their full sizes, from mesh_topology and mesh_weld on a scene of the rows R; what the weld leaves
    untouched is zero here.  Also the two results, for the wrapper."""
    n = R.shape[0]
    scene = hip.scene_create(np.array(R), BS.proxy_nodes(n))
    topo = query.mesh_topology(scene, components=False)
    weld = query.mesh_weld(scene)
    torch.cuda.synchronize()
    a = dict(twin=_padded(topo.twin, 3 * n, np.int32), edge_class=_padded(topo.edge_class, 3 * n, np.uint8),
             vertex=_padded(weld.vertex, 3 * n, np.int32), star_offsets=_padded(weld.star_offsets, 3 * n + 1, np.int32),
             star=_padded(weld.star, 3 * n, np.int32), vert_flags=_padded(weld.vert_flags, 3 * n, np.uint8))
    return a, topo, weld


def _case(hip, n):
    """(rows [n, 36], the six arrays, {mode: the restatement's (out, summary)}), computed once and shared"""
    if n not in _cache:
        R = SS.sized(n)
        a, _, _ = _device_arrays(hip, R)
        want = {SE.MIDPOINT: SE.subdivide(R, SE.MIDPOINT)[:2], SE.LOOP: SE.subdivide(R, SE.LOOP, **a)[:2]}
        _cache[n] = (R, a, want)
    return _cache[n]


def _run(lib, sg, R, mode, arrays, dev, shift=0, out_shift=None, work_fill=FILL, stream=None, sync=True):
    """ezrt_subdivide_rows_device over poisoned buffers: tri36 starts `shift` floats and out `out_shift` floats (default: the same)
    into 512-byte aligned allocations; out has ROOM rows, summary and work ROOM words behind their stated sizes.  Returns (out
    [4 n + ROOM, 36], summary [8 + ROOM]) as numpy arrays."""
    n = R.shape[0]
    oshift = shift if out_shift is None else out_shift
    d_in = torch.full((shift + n * 36 + 36,), 3.0, dtype=torch.float32, device=dev)
    d_in[shift:shift + n * 36] = _g(R, dev, F).reshape(-1)
    d_out = torch.full((oshift + (4 * n + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    summary = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_subdivide_work_bytes(n, mode)
    assert wb % 8 == 0 and wb == (48 * n + 8 if mode == SE.LOOP else 8)
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    d_arr = [_g(arrays[k], dev, DTYPES[k]) for k in ARRAYS] if mode == SE.LOOP else [None] * 6
    assert d_in.data_ptr() % 512 == 0 and d_out.data_ptr() % 512 == 0
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_subdivide_rows_device(sg._h, P(d_in.data_ptr() + 4 * shift), n, mode, *[P(x.data_ptr()) if x is not None else None for x in d_arr],
                                         P(d_out.data_ptr() + 4 * oshift), P(summary.data_ptr()), P(work.data_ptr()), wb,
                                         P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((work[wb // 8:] == tail).all())                            # nothing behind the stated bytes of work
        assert bool((d_out[:oshift] == POISON_F).all())
        assert np.array_equal(SE.bits(d_in[shift:shift + n * 36].cpu().numpy().reshape(-1, 36)), SE.bits(R))
        for k, x in zip(ARRAYS, d_arr):
            assert x is None or np.array_equal(x.cpu().numpy(), arrays[k]), k  # the arrays are read only
        return d_out[oshift:].cpu().numpy().reshape(-1, 36), summary.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same(got, want, n, what=""):
    out, summary = got
    w_out, w_sum = want
    assert out.shape[0] == 4 * n + ROOM
    bad = (SE.bits(out[:4 * n]) != SE.bits(w_out)) & ~(np.isnan(out[:4 * n]) & np.isnan(w_out))
    assert not bad.any(), "%s: %d output rows differ, first %d (float %d)" % (what, int(bad.any(1).sum()), int(np.argmax(bad.any(1))),
                                                                              int(np.argmax(bad[np.argmax(bad.any(1))])))
    assert (out[4 * n:] == POISON_F).all(), "%s: a row beyond 4 n_rows was written" % what
    assert np.array_equal(summary[:8], w_sum) and (summary[8:] == POISON).all(), (what, summary[:8].tolist(), w_sum.tolist())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SS.SIZES)
def test_subdivide_on_the_bits(hip, sg, dev, n, mode):
    R, a, want = _case(hip, n)
    if mode == SE.LOOP and n >= 255:
        assert want[mode][1][1] > 0 and want[mode][1][2] > 0 and want[mode][1][3] > 0 and want[mode][1][4] > 0   # every rule is taken
    _same(_run(hip.lib, sg, R, mode, a, dev), want[mode], n, "%d rows, mode %d" % (n, mode))


def test_more_tiles_than_workgroups(hip, sg, dev):
    """the staged fill has at most 2048 workgroups, which stride over tiles of 63 rows: beyond 129 024 rows a workgroup takes a second
    tile, and its counts run over both.  A torus of 131 072 triangles, with dead rows in the first and in the last tile."""
    import clip_scenes as CS
    import topology_scenes as TS
    R = CS.decorate(TS.torus(256), SS.SEED + 51)
    n = R.shape[0]
    assert n > 2048 * SS.SD_TILE
    dead = SS.rows("dead")
    R[5:5 + dead.shape[0]] = dead
    R[n - 40:n - 40 + dead.shape[0]] = dead
    a, _, _ = _device_arrays(hip, R)
    for mode in MODES:
        want = SE.subdivide(R, mode, **(a if mode == SE.LOOP else {}))[:2]
        if mode == SE.LOOP:
            assert want[1][1] > 3 * n - 2000 and want[1][2] > 0 and want[1][3] > 0
        _same(_run(hip.lib, sg, R, mode, a, dev), want, n, "%d rows, mode %d" % (n, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (65, 2049))
def test_both_routes_give_the_same_bits(hip, sg, dev, n, mode):
    """one row in, tri36 and out are still 16-byte aligned and take the staged route; 4 bytes in they take the per-lane route, and so
    does a call with only one of the two off the 16 bytes"""
    R, a, want = _case(hip, n)
    for shift in (36, 1, 37, 2, 3):
        _same(_run(hip.lib, sg, R, mode, a, dev, shift=shift), want[mode], n, "%d rows, mode %d, %d floats in" % (n, mode, shift))
    for shift, oshift in ((0, 1), (3, 0), (36, 2), (1, 72)):                   # tri36 aligned and out not, and the other way round
        _same(_run(hip.lib, sg, R, mode, a, dev, shift=shift, out_shift=oshift), want[mode], n,
              "%d rows, mode %d, tri36 %d and out %d floats in" % (n, mode, shift, oshift))


def test_what_work_holds_means_nothing_and_two_streams(hip, sg, dev):
    n = 4097
    R, a, want = _case(hip, n)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(SS.SEED + 11))):
        _same(_run(hip.lib, sg, R, SE.LOOP, a, dev, work_fill=fill), want[SE.LOOP], n, "work=%s" % what)
        _same(_run(hip.lib, sg, R, SE.LOOP, a, dev, work_fill=fill, shift=1), want[SE.LOOP], n, "work=%s, per lane" % what)
    R2, a2, want2 = _case(hip, 2049)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    f1 = _run(hip.lib, sg, R, SE.LOOP, a, dev, work_fill=-1, stream=s1, sync=False)
    f2 = _run(hip.lib, sg, R2, SE.LOOP, a2, dev, work_fill=0, shift=1, stream=s2, sync=False)
    f3 = _run(hip.lib, sg, R2, SE.MIDPOINT, a2, dev, stream=s1, sync=False)
    torch.cuda.synchronize()
    _same(f1(), want[SE.LOOP], n, "on a side stream")
    _same(f2(), want2[SE.LOOP], 2049, "on another side stream")
    _same(f3(), want2[SE.MIDPOINT], 2049, "midpoint on a side stream")


@pytest.mark.parametrize("shift", (0, 1))
def test_corrupted_arrays(hip, sg, dev, shift):
    """S3, S4, S7: whatever the arrays hold, the answer is the restatement's and nothing out of bounds is touched"""
    n = 2049
    R, a, want = _case(hip, n)
    for name, b, w in _corrupted(R, a, want):
        _same(_run(hip.lib, sg, R, SE.LOOP, b, dev, shift=shift), w, n, name)


def _corrupted(R, a, want):
    """[(name, the six arrays with some of them damaged, the restatement's (out, summary))], computed once and shared"""
    if "corrupted" in _cache:
        return _cache["corrupted"]
    n = R.shape[0]
    H = 3 * n
    rng = np.random.default_rng(SS.SEED + 31)
    bad = np.array([-1, -2, H, H + 1, 2 ** 31 - 1, -2 ** 31, 0, 1, H - 1])
    cases = []
    for k in ("twin", "vertex", "star_offsets", "star"):
        some = a[k].copy()
        at = rng.integers(0, some.size, some.size // 20)
        some[at] = rng.choice(bad[:6] if k == "star_offsets" else bad, at.size)
        cases.append(("5 %% of %s overwritten" % k, {k: some}))
        if k != "star_offsets":
            cases.append(("%s random" % k, {k: rng.integers(-5, H + 5, a[k].size).astype(np.int32)}))
    lo = rng.integers(-5, H + 5, H + 1)                                        # short ranges anywhere: the stars of other vertices, or none
    cases.append(("star_offsets random", {"star_offsets": np.where(np.arange(H + 1) % 2, lo + rng.integers(-2, 9, H + 1), lo).astype(np.int32)}))
    out = []
    for name, change in cases:
        b = dict(a)
        b.update(change)
        w = SE.subdivide(R, SE.LOOP, **b)[:2]
        if name.startswith("5 %"):
            assert not np.array_equal(w[1], want[SE.LOOP][1]), name             # the damage is seen
        out.append((name, b, w))
    _cache["corrupted"] = out
    return out


def _chain(hip, sg, dev, R, mode, topo=None, weld=None):
    """subdivide on the device with the wrapper, a scene of the rows, topology and weld on it"""
    d_rows = torch.from_numpy(np.array(R)).to(dev)
    if mode == "loop" and topo is None:
        _, topo, weld = _device_arrays(hip, R)
    got = query.subdivide_rows(sg, d_rows, mode, topo, weld) if mode == "loop" else query.subdivide_rows(sg, d_rows)
    torch.cuda.synchronize()
    rows = got.rows.cpu().numpy()
    scene = hip.scene_create(rows, BS.proxy_nodes(rows.shape[0]))
    t2 = query.mesh_topology(scene)
    w2 = query.mesh_weld(scene)
    return got, rows, scene, t2, w2, topo, weld


@pytest.mark.parametrize("mode", ("midpoint", "loop"))
@pytest.mark.parametrize("name", ("cube_pow2", "torus32"))
def test_closed_scenes_stay_closed_manifolds(hip, sg, dev, name, mode):
    R = SS.rows(name)
    a, topo, weld = _device_arrays(hip, R)
    Fc, Ec, Vc = topo.summary.tolist()[0], topo.summary.tolist()[1], weld.n_vert
    got, rows, scene, t2, w2, _, _ = _chain(hip, sg, dev, R, mode, topo, weld)
    want = SE.subdivide(R, SE.LOOP, **a) if mode == "loop" else SE.subdivide(R, SE.MIDPOINT)
    assert SE.same_rows(rows, want[0]) and np.array_equal(got.summary.cpu().numpy(), want[1])
    sm = t2.summary.tolist()
    assert sm[0] == 4 * Fc and sm[1] == 2 * Ec + 3 * Fc and w2.n_vert == Vc + Ec and t2.closed and t2.oriented and w2.manifold_vertices
    assert query.euler_characteristic(w2, t2) == query.euler_characteristic(weld, topo) == Vc - Ec + Fc
    assert sm[6] == 1
    if mode == "loop":                                                         # S8: smooth normals are a weld and vertex_normals on the output
        smooth = query.vertex_normals(scene, got.rows.clone(), w2)
        torch.cuda.synchronize()
        nrm = smooth[:, 9:18].cpu().numpy()
        assert np.isfinite(nrm).all() and np.isfinite(rows[:, 9:18]).all() and not np.array_equal(nrm, rows[:, 9:18])


def test_the_moebius_band_keeps_its_flipped_edges(hip, sg, dev):
    R = SS.rows("moebius")
    got, rows, scene, t2, w2, topo, weld = _chain(hip, sg, dev, R, "loop")
    a, b = topo.summary.tolist(), t2.summary.tolist()
    assert a[4] > 0 and b[4] == 2 * a[4] and b[2] == 2 * a[2] and b[5] == 0 and not t2.oriented and b[0] == 4 * a[0]


def test_two_loop_levels_of_the_cube(hip, sg, dev):
    R = SS.rows("cube_pow2")
    got, rows, scene, t2, w2, topo, weld = _chain(hip, sg, dev, R, "loop")
    a2 = dict(twin=_padded(t2.twin, 144, np.int32), edge_class=_padded(t2.edge_class, 144, np.uint8), vertex=_padded(w2.vertex, 144, np.int32),
              star_offsets=_padded(w2.star_offsets, 145, np.int32), star=_padded(w2.star, 144, np.int32), vert_flags=_padded(w2.vert_flags, 144, np.uint8))
    want = SE.subdivide(rows, SE.LOOP, **a2)
    got2, rows2, scene2, t3, w3, _, _ = _chain(hip, sg, dev, rows, "loop", t2, w2)
    assert SE.same_rows(rows2, want[0]) and np.array_equal(got2.summary.cpu().numpy(), want[1])
    assert want[1].tolist() == [192, 144, 0, 0, 144, 0, 1, 0]
    sm = t3.summary.tolist()
    assert sm[0] == 192 and sm[1] == 288 and w3.n_vert == 98 and t3.closed and t3.oriented and w3.manifold_vertices
    V = rows2[:, :9].reshape(-1, 3)
    assert V.min() > 0 and V.max() < 4                                         # the cube shrinks towards its limit surface


def test_midpoint_of_the_bunny_is_scenes_subdivide(hip, sg, dev):
    v, f = scenes.mesh("bunny")
    R = SS.rows("bunny")
    nf = f.shape[0]
    assert np.array_equal(SE.bits(R[:, :9].reshape(nf, 3, 3)), SE.bits(v[f]))
    got = query.subdivide_rows(sg, torch.from_numpy(np.array(R)).to(dev))
    torch.cuda.synchronize()
    v1, f1 = scenes.subdivide(v, f, 1)
    want = np.ascontiguousarray(v1[f1].reshape(4, nf, 9).transpose(1, 0, 2))  # face j * F + t
    assert np.array_equal(SE.bits(got.rows[:, :9].cpu().numpy().reshape(nf, 4, 9)), SE.bits(want))
    assert got.summary.tolist() == [4 * nf, 0, 0, 3 * nf, 0, 3 * nf, 0, 0] and got.n_rows == nf


def test_the_wrapper(hip, sg, dev):
    for i, name in enumerate(SS.NAMES):
        R = SS.rows(name)
        n = R.shape[0]
        a, topo, weld = _device_arrays(hip, R)
        d_rows = torch.from_numpy(np.array(R)).to(dev)
        kw = ({}, {"stream": torch.cuda.Stream(dev)})[i % 2]
        if "stream" in kw:
            kw["stream"].wait_stream(torch.cuda.current_stream(dev))
        mid = query.subdivide_rows(sg, d_rows, **kw)
        lp = query.subdivide_rows(sg, d_rows, "loop", topo, weld, **kw)
        torch.cuda.synchronize()
        for got, want in ((mid, SE.subdivide(R, SE.MIDPOINT)), (lp, SE.subdivide(R, SE.LOOP, **a))):
            assert isinstance(got, query.SubdivRows) and got.n_rows == n and got.rows.dtype == torch.float32 and got.summary.dtype == torch.int64
            assert tuple(got.rows.shape) == (4 * n, 36) and np.array_equal(got.summary.cpu().numpy(), want[1]), name
            assert SE.same_rows(got.rows.cpu().numpy(), want[0]), name
    empty = query.subdivide_rows(sg, torch.zeros((0, 36), dtype=torch.float32, device=dev))
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
    mid = query.subdivide_rows(scn, rows)
    lp = query.subdivide_rows(scn, rows, "loop", topo, weld)
    torch.cuda.synchronize()
    assert mid.rows.shape[0] == lp.rows.shape[0] == 4 * rows.shape[0] and (scn.counters(), scn.last_render_ms()) == before
    assert lp.summary.tolist()[1] > 0 and lp.summary.tolist()[2] > 0


def test_errors(hip, sg, oracle, bunny_small, dev):
    lib = hip.lib
    n = 300
    R = SS.sized(n)
    a, topo, weld = _device_arrays(hip, R)
    want = SE.subdivide(R, SE.LOOP, **a)
    wb = lib.ezrt_subdivide_work_bytes(n, SE.LOOP)
    bufs = dict(tri36=_g(R, dev, F), out=torch.full((4 * n, 36), 5.0, dtype=torch.float32, device=dev),
                summary=torch.full((8,), 5, dtype=torch.int64, device=dev), work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    arr = {k: _g(a[k], dev, DTYPES[k]) for k in ARRAYS}
    host = np.zeros(36 * 5 * n, np.int64)
    hp = P(host.ctypes.data)
    torch.cuda.synchronize()
    f = lib.ezrt_subdivide_rows_device
    d = lambda x: P(x.data_ptr())

    def fa(mode=SE.LOOP, **kw):
        g = lambda k: kw[k] if k in kw else d(bufs[k])
        h = lambda k: kw[k] if k in kw else (d(arr[k]) if mode == SE.LOOP else None)
        return [kw.get("s", sg._h), g("tri36"), kw.get("n_rows", n), mode] + [h(k) for k in ARRAYS] + [g("out"), g("summary"), g("work"),
                                                                                                         kw.get("work_bytes", wb), None]
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID and f(*fa(SE.MIDPOINT, work_bytes=7)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    assert f(*fa(SE.MIDPOINT, work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + list(bufs):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
        assert f(*fa(SE.MIDPOINT, **{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in ARRAYS:                                                           # a partly NULL group, in either mode
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"together" in lib.ezrt_last_error(), k
        assert f(*fa(SE.MIDPOINT, **{k: d(arr[k])})) == EZRT_ERR_INVALID and b"together" in lib.ezrt_last_error(), k
    assert f(*fa(**{k: None for k in ARRAYS})) == EZRT_ERR_INVALID and b"LOOP" in lib.ezrt_last_error()
    assert f(*fa(SE.MIDPOINT, **{k: d(arr[k]) for k in ARRAYS})) == EZRT_ERR_INVALID and b"MIDPOINT" in lib.ezrt_last_error()
    for mode in (-1, 2, 7):
        assert f(*fa(mode)) == EZRT_ERR_INVALID and b"mode" in lib.ezrt_last_error(), mode
    for k in list(bufs) + list(ARRAYS):                                        # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert f(*fa(n_rows=-1)) == EZRT_ERR_INVALID and f(*fa(n_rows=(2 ** 31 - 1) // 12 + 1, work_bytes=2 ** 40)) == EZRT_ERR_INVALID
    assert b"INT32_MAX / 12" in lib.ezrt_last_error()
    assert f(*fa(n_rows=0)) == 0 and f(*fa(SE.MIDPOINT, n_rows=0)) == 0         # launches nothing
    torch.cuda.synchronize()
    assert bool((bufs["out"] == 5.0).all()) and bool((bufs["summary"] == 5).all()) and not host.any()
    # out overlapping tri36: the same rows, rows that begin inside tri36, rows that end inside it
    both = torch.full((6 * n + 2, 36), 5.0, dtype=torch.float32, device=dev)
    both[4 * n:5 * n] = bufs["tri36"]
    torch.cuda.synchronize()
    at = lambda row: P(both.data_ptr() + 144 * row)
    for out_row in (4 * n, 5 * n - 1, 4 * n - 1, 1):
        assert f(*fa(tri36=at(4 * n), out=at(out_row))) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error(), out_row
    assert f(*fa(SE.MIDPOINT, tri36=at(4 * n), out=at(2 * n))) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((both[:4 * n] == 5.0).all()) and bool((both[5 * n:] == 5.0).all())
    assert f(*fa(tri36=at(4 * n), out=at(0))) == 0                             # before it, up to its first byte: no overlap
    torch.cuda.synchronize()
    assert SE.same_rows(both[:4 * n].cpu().numpy(), want[0]) and bool((both[5 * n:] == 5.0).all())
    assert np.array_equal(SE.bits(both[4 * n:5 * n].cpu().numpy()), SE.bits(R))
    bufs["summary"].fill_(5)
    # the rejected calls left no HIP error behind: the next call works
    assert f(*fa()) == 0
    torch.cuda.synchronize()
    assert SE.same_rows(bufs["out"].cpu().numpy(), want[0]) and np.array_equal(bufs["summary"].cpu().numpy(), want[1]) and not host.any()
    # the wrappers
    rows = bufs["tri36"]
    with pytest.raises(TypeError):
        query.subdivide_rows(bunny_small.upload(oracle), rows)
    with pytest.raises(TypeError):
        query.subdivide_rows(sg, rows.cpu())
    with pytest.raises(TypeError):
        query.subdivide_rows(sg, rows.to(torch.float64))
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows[:, :35])
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows.reshape(2, -1, 36))
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "smooth")
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "loop")
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "loop", topo)
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "loop", None, weld)
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "midpoint", topo, weld)
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows, "loop", topo, weld._replace(vert_flags=None, fans=None))   # a weld made with flags=False
    with pytest.raises(ValueError):
        query.subdivide_rows(sg, rows[:100], "loop", topo, weld)              # a topology of other rows

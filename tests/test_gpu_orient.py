"""Mesh orientation on device tensors (include/ezrt_orient.h, ezrt_amd/query.py: mesh_orient, rewind, patch_volume).

Every output of the call -- flip, patch_root, patch, proot, psize, pflags, vol6, summary -- is compared EXACTLY with
tests/orient_expected.py, the header's rule restated on the host and held to its properties by tests/test_orient_expected.py.  There is
no tolerance anywhere, vol6 included.

* every case of tests/orient_scenes.py, both values of `outward`, over poisoned buffers with room behind them: what the call must not
  touch (entries at and beyond P, the room, the bytes behind `work`, the guard entries behind the inputs) still holds the poison;
* `work` pre-filled with zeros, with 0xFF and with random bytes; a side stream; the same call three times gives the same bytes;
* O2's robustness: twin and edge_class overwritten with garbage, against the restatement on the same garbage;
* ezrt_rewind_device: the marked rows exactly exchanged, everything else and a guard row unchanged on the bits, twice is the identity;
* the loop this is for: topology, orient, rewind, refit, topology, orient -- and query.surface against a scene created from the
  restatement's re-wound rows;
* the error contract, the wrappers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
OUT = (("flip", torch.uint8), ("patch_root", torch.int32), ("patch", torch.int32), ("proot", torch.int32), ("psize", torch.int32),
       ("pflags", torch.uint8), ("vol6", torch.int64))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, the device scene, the restatement's topology, its orientation without and with `outward`), computed once and shared"""
    if name not in _cache:
        tri, nodes = OS.scene(name, bunny_small)
        t = TE.topology(tri)
        _cache[name] = (tri, hip.scene_create(tri, nodes), t, OE.orient(tri, t.twin, t.edge_class, False), OE.orient(tri, t.twin, t.edge_class, True))
    return _cache[name]


def _g(x, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _raw(lib, sg, n_tri, dev, twin, cls, outward, work_fill=FILL, stream=None):
    """the C call itself over poisoned buffers: dict of numpy arrays, each with ROOM entries behind its stated size"""
    out = {k: torch.full((n_tri + ROOM,), POISON8 if dt == torch.uint8 else POISON, dtype=dt, device=dev) for k, dt in OUT}
    out["summary"] = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    d_twin = _g(np.concatenate([np.asarray(twin, np.int32).ravel(), np.full(ROOM, POISON, np.int32)]), dev, np.int32)
    d_cls = _g(np.concatenate([np.asarray(cls, np.uint8).ravel(), np.full(ROOM, POISON8, np.uint8)]), dev, np.uint8)
    keep = (d_twin.clone(), d_cls.clone())
    wb = lib.ezrt_orient_work_bytes(n_tri)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:                                                                      # a generator: random bytes
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    torch.cuda.synchronize()
    d = lambda k: P(out[k].data_ptr())
    got = lib.ezrt_mesh_orient_device(sg._h, P(d_twin.data_ptr()), P(d_cls.data_ptr()), 1 if outward else 0, d("flip"), d("patch_root"), d("patch"),
                                      d("proot"), d("psize"), d("pflags"), d("vol6"), d("summary"), P(work.data_ptr()), wb,
                                      P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((work[wb // 8:] == tail).all())                                # nothing behind the stated bytes of work
    assert bool((d_twin == keep[0]).all()) and bool((d_cls == keep[1]).all())  # the inputs and their guards
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, n_tri, what=""):
    """every output against the restatement's, and the poison wherever the call must not write"""
    k = int(want.summary[1])
    for name, dt in OUT:
        size = n_tri if name in ("flip", "patch_root", "patch") else k
        w = getattr(want, name)
        poison = POISON8 if dt == torch.uint8 else POISON
        assert w.shape[0] == size
        diff = got[name][:size] != w
        assert not diff.any(), "%s: %s differs at %d entries, first at %d: %r, not %r" % (
            what, name, int(diff.sum()), int(np.argmax(diff)), got[name][:size][diff][:4], w[diff][:4])
        assert (got[name][size:] == poison).all(), "%s: %s was written at or beyond %d" % (what, name, size)
    assert np.array_equal(got["summary"][:8], want.summary), "%s: summary %r, not %r" % (what, got["summary"][:8], want.summary)
    assert (got["summary"][8:] == POISON).all(), what


@pytest.mark.parametrize("outward", (False, True))
@pytest.mark.parametrize("name", OS.NAMES)
def test_orient_on_the_bits(hip, bunny_small, dev, name, outward):
    tri, sg, t, o0, o1 = _case(name, hip, bunny_small)
    n = tri.shape[0]
    assert sg.stats()["n_tri"] == n
    want = o1 if outward else o0
    _same(_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, outward), want, n, name)
    if name == "bunny_rev_not_nested":                                         # nothing depends on the tree
        other = _case("bunny_rev", hip, bunny_small)[4 if outward else 3]
        assert all(np.array_equal(getattr(want, k), getattr(other, k)) for k, _ in OUT) and np.array_equal(want.summary, other.summary)
    if name == "tetra_flip" and outward:
        assert want.flip.sum() == 1


@pytest.mark.parametrize("name", ("torus_rev", "strip_rev", "islands_rev", "klein", "nested"))
def test_what_work_holds_means_nothing(hip, bunny_small, dev, name):
    tri, sg, t, o0, o1 = _case(name, hip, bunny_small)
    n = tri.shape[0]
    side = torch.cuda.Stream(dev)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("random", np.random.default_rng(OS.SEED + 11))):
        _same(_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, True, work_fill=fill), o1, n, "%s work=%s" % (name, what))
    _same(_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, False, work_fill=-1, stream=side), o0, n, "%s on a side stream" % name)
    runs = [_raw(hip.lib, sg, n, dev, t.twin, t.edge_class, True) for _ in range(3)]   # the same call three times: the same bytes
    assert all(np.array_equal(runs[0][k], r[k]) for r in runs[1:] for k in runs[0])


@pytest.mark.parametrize("name", ("torus_rev", "dead", "nested"))
def test_arrays_that_are_no_topology(hip, bunny_small, dev, name):
    """O2 as a contract: whatever twin and edge_class hold, the call answers as the restatement does on the same arrays and reads
    nothing out of bounds"""
    tri, sg, t, _, _ = _case(name, hip, bunny_small)
    n = tri.shape[0]
    H = 3 * n
    rng = np.random.default_rng(OS.SEED + 13)
    i32 = np.int32
    k = max(H // 10, 3)
    cases = []
    tw = t.twin.copy()
    tw[rng.integers(0, H, k)] = rng.integers(-5, H + 5, k)                     # ids out of range and one-sided pairs
    cases.append(("twin out of range", tw, t.edge_class))
    tw = t.twin.copy()
    tw[rng.integers(0, H, k)] = rng.choice(i32([-2 ** 31, 2 ** 31 - 1, H, -1, -2]), k)
    cases.append(("twin INT32_MIN / INT32_MAX", tw, t.edge_class))
    tw = t.twin.copy()
    sel = rng.integers(0, n, max(k // 3, 1))
    tw[3 * sel], tw[3 * sel + 1] = 3 * sel + 1, 3 * sel                        # self-pairs
    cases.append(("self-pairs", tw, np.where(np.isin(np.arange(H) // 3, sel), 2, t.edge_class).astype(np.uint8)))
    for bad in (0, 5, 255):
        cl = t.edge_class.copy()
        cl[rng.integers(0, H, k)] = bad
        cases.append(("edge_class = %d" % bad, t.twin, cl))
    cases.append(("random", rng.integers(-2 ** 31, 2 ** 31 - 1, H).astype(i32), rng.integers(0, 256, H).astype(np.uint8)))
    cases.append(("random twin, class 2", rng.integers(0, H, H).astype(i32), np.full(H, 2, np.uint8)))
    cases.append(("all FLIPPED", t.twin, np.where(t.edge_class == 2, 3, t.edge_class).astype(np.uint8)))
    for i, (what, tw, cl) in enumerate(cases):
        for outward in ((False, True) if n < 100 else (i % 2 == 0,)):         # (the restatement is slow on 8192 triangles)
            want = OE.orient(tri, tw, cl, outward)
            _same(_raw(hip.lib, sg, n, dev, tw, cl, outward), want, n, "%s: %s" % (name, what))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ("torus_rev", "dead", "tetra_flip"))
def test_rewind(hip, bunny_small, dev, name):
    tri, sg, t, o0, o1 = _case(name, hip, bunny_small)
    n = tri.shape[0]
    rng = np.random.default_rng(OS.SEED + 17)
    rows = np.concatenate([tri, np.full((1, 36), 12345.0, np.float32)])
    rows[:n, 9:18] = rng.standard_normal((n, 9)).astype(np.float32)            # three different normals a row
    side = torch.cuda.Stream(dev)
    for flip, st in ((o0.flip, None), (o1.flip, side), ((rng.random(n) < 0.5).astype(np.uint8) * 201, None), (np.zeros(n, np.uint8), None)):
        d_rows = torch.from_numpy(rows).to(dev)
        d_flip = _g(np.concatenate([flip, np.full(ROOM, 1, np.uint8)]), dev, np.uint8)   # a guard that says "reverse" behind the array
        torch.cuda.synchronize()
        f = lambda: hip.lib.ezrt_rewind_device(sg._h, P(d_rows.data_ptr()), n, P(d_flip.data_ptr()), P(st.cuda_stream) if st is not None else None)
        assert f() == 0, hip.lib.ezrt_last_error()
        torch.cuda.synchronize()
        out = d_rows.cpu().numpy()
        assert np.array_equal(bits(out), bits(np.concatenate([OE.rewind(rows[:n], flip), rows[n:]])))
        m = flip != 0
        keep = [0, 1, 2, 9, 10, 11] + list(range(18, 36))
        assert np.array_equal(bits(out[:n, keep]), bits(rows[:n, keep])) and np.array_equal(bits(out[:n][~m]), bits(rows[:n][~m]))
        assert np.array_equal(bits(out[n]), bits(rows[n]))                     # the guard row
        assert np.array_equal(bits(out[:n][m][:, 3:6]), bits(rows[:n][m][:, 6:9])) and np.array_equal(bits(out[:n][m][:, 15:18]), bits(rows[:n][m][:, 12:15]))
        assert f() == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_rows.cpu().numpy()), bits(rows))          # applied twice it restores the rows


@pytest.mark.parametrize("name", ("torus_rev", "bunny_rev", "nested"))
def test_orient_rewind_refit(hip, bunny_small, dev, name):
    """the loop this is for: topology, orient, rewind, refit -- against a scene created from the restatement's re-wound rows"""
    tri, nodes = OS.tree_scene(name, bunny_small)
    n = tri.shape[0]
    sg = hip.scene_create(tri, nodes)
    t = TE.topology(tri)
    want = OE.orient(tri, t.twin, t.edge_class, True)
    inside = torch.tensor([[2.0, 0.0, 0.0]], dtype=torch.float32, device=dev)  # a point inside the torus' tube
    if name == "torus_rev":
        before = float(query.winding_number(sg, inside)[0])
    topo = query.mesh_topology(sg)
    assert topo.oriented == (name == "nested")                                # (the inner cube is reversed as a whole: no FLIPPED edge)
    o = query.mesh_orient(sg, topo, outward=True)
    assert np.array_equal(o.flip.cpu().numpy(), want.flip) and o.orientable and o.summary.tolist() == want.summary.tolist()
    d_tri = torch.from_numpy(tri).to(dev)
    assert query.rewind(sg, d_tri, o) is d_tri
    refit.refit(sg, d_tri)
    want_rows = OE.rewind(tri, want.flip)
    assert np.array_equal(bits(d_tri.cpu().numpy()), bits(want_rows))
    topo2 = query.mesh_topology(sg)
    o2 = query.mesh_orient(sg, topo2, outward=True)
    t2 = TE.topology(want_rows)
    assert topo2.oriented == TE.oriented(t2) == bool(t2.summary[5] == 0) and topo2.summary.tolist()[4] == 0
    pf = o2.pflags.cpu().numpy()
    assert o2.summary.tolist()[4] == 0 and not (pf & _abi.PATCH_REWOUND).any() and not (pf & _abi.PATCH_INWARD).any() and not bool(o2.flip.any())
    assert np.array_equal(o2.vol6.cpu().numpy(), want.vol6) and o2.scale == want.scale
    fresh = hip.scene_create(want_rows, refit.refit_nodes(want_rows, nodes))   # what a refitted scene answers as (ezrt_refit.h)
    rng = np.random.default_rng(OS.SEED + 19)
    k = 300
    V = want_rows[:, :9].reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    og = rng.uniform(lo - 1.0, hi + 1.0, (k, 3))
    tg = rng.uniform(lo, hi, (k, 3))
    rays = torch.from_numpy(np.concatenate([og, tg - og], 1).astype(np.float32)).to(dev)
    a, b = query.surface(sg, rays), query.surface(fresh, rays)
    torch.cuda.synchronize()
    tid = a.tri.cpu().numpy()
    assert (tid >= 0).sum() > 50 and np.array_equal(tid, b.tri.cpu().numpy())
    for x, y in ((a.t, b.t), (a.point, b.point), (a.normal, b.normal), (a.inside, b.inside)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(x, y) or np.array_equal(bits(x), bits(y))
    if name == "torus_rev":
        after = float(query.winding_number(sg, inside)[0])
        assert abs(after - 1.0) < 1e-3 and abs(before - 1.0) > 0.1 and float(query.patch_volume(o)[0]) > 0
    if name == "nested":
        assert query.patch_volume(o).tolist() == [64.0, 1.0] and want.flip.sum() == 12


def test_the_wrappers(hip, bunny_small, dev):
    for name in ("tetra_flip", "moebius", "torus_rev", "book5", "dead", "nested"):
        tri, sg, t, o0, o1 = _case(name, hip, bunny_small)
        n = tri.shape[0]
        topo = query.mesh_topology(sg, components=False)
        for kw in ({}, {"topo": topo}, {"topo": topo, "outward": False}, {"stream": torch.cuda.Stream(dev)}):
            o = query.mesh_orient(sg, **kw)
            torch.cuda.synchronize()
            want = o1 if kw.get("outward", True) else o0
            assert o.flip.dtype == torch.uint8 and o.pflags.dtype == torch.uint8 and o.vol6.dtype == torch.int64 and o.patch.dtype == torch.int32
            assert tuple(o.flip.shape) == (n,) and o.n_patch == want.summary[1] == o.proot.shape[0] and o.scale == want.scale
            for k, _ in OUT:
                assert np.array_equal(getattr(o, k).cpu().numpy(), getattr(want, k)), (name, k)
            assert np.array_equal(o.summary.cpu().numpy(), want.summary) and o.orientable is bool(want.summary[2] == want.summary[1])
            vol = query.patch_volume(o)
            assert vol.dtype == torch.float64 and np.array_equal(vol.cpu().numpy(), OE.patch_volume(want))
        rows = torch.from_numpy(tri).to(dev)
        assert query.rewind(sg, rows, o) is rows
        torch.cuda.synchronize()
        assert query.rewind(sg, rows, o, stream=torch.cuda.Stream(dev)) is rows
        torch.cuda.synchronize()
        assert np.array_equal(bits(rows.cpu().numpy()), bits(tri))
    _, sg, _, _, o1 = _case("tetra_flip", hip, bunny_small)
    o = query.mesh_orient(sg)
    assert o.flip.tolist() == [1, 0, 0, 0] and float(query.patch_volume(o)[0]) > 0 and o.pflags.tolist() == [_abi.PATCH_REWOUND | _abi.PATCH_INWARD]


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
    o = query.mesh_orient(sg)
    query.rewind(sg, torch.from_numpy(np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)).to(dev), o)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before


def test_errors(hip, oracle, bunny_small, dev):
    tri, sg, t, o0, o1 = _case("nested", hip, bunny_small)
    lib = hip.lib
    n = tri.shape[0]
    H = 3 * n
    f = lib.ezrt_mesh_orient_device
    wb = lib.ezrt_orient_work_bytes(n)
    full = lambda k, dt: torch.full((k,), 5, dtype=dt, device=dev)
    bufs = dict(twin=_g(t.twin, dev, np.int32), edge_class=_g(t.edge_class, dev, np.uint8), flip=full(n, torch.uint8), patch_root=full(n, torch.int32),
                patch=full(n, torch.int32), proot=full(n, torch.int32), psize=full(n, torch.int32), pflags=full(n, torch.uint8),
                vol6=full(n, torch.int64), summary=full(8, torch.int64), work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    keys = list(bufs)
    outs = keys[2:-1]
    host = np.zeros(max(wb // 8 + 1, 36 * n), np.int64)
    torch.cuda.synchronize()
    hp = P(host.ctypes.data)

    def fa(**kw):
        args = [kw.get("s", sg._h)]
        args += [kw[k] if k in kw else P(bufs[k].data_ptr()) for k in keys[:2]] + [kw.get("outward", 1)]
        args += [kw[k] if k in kw else P(bufs[k].data_ptr()) for k in keys[2:]]
        return args + [kw.get("work_bytes", wb), None]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((bufs[k] == 5).all()) for k in outs)
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + keys:                                                     # any NULL pointer
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in keys:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert not host.any() and untouched()
    # the rewind
    g = lib.ezrt_rewind_device
    rows = torch.from_numpy(tri).to(dev)
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    d = lambda x: P(x.data_ptr())
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("tri36", d(rows)), kw.get("n_tri", n), kw.get("flip", d(ones)), None]
    for k in ("s", "tri36", "flip"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
        if k != "s":
            assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    for bad in (n - 1, n + 1, 0, -1):
        assert g(*ga(n_tri=bad)) == EZRT_ERR_INVALID and b"n_tri" in lib.ezrt_last_error(), bad
    torch.cuda.synchronize()
    assert np.array_equal(bits(rows.cpu().numpy()), bits(tri)) and not host.any()
    # the rejected calls left no HIP error behind: the next call works
    _same(_raw(lib, sg, n, dev, t.twin, t.edge_class, True), o1, n, "after the rejected calls")
    # the wrappers
    with pytest.raises(TypeError):
        query.mesh_orient(bunny_small.upload(oracle))
    with pytest.raises(ValueError):
        query.mesh_orient(sg, outward=1)
    topo = query.mesh_topology(sg, components=False)
    with pytest.raises(TypeError):
        query.mesh_orient(sg, topo._replace(twin=topo.twin.to(torch.int64)))
    with pytest.raises(TypeError):
        query.mesh_orient(sg, topo._replace(edge_class=topo.edge_class.cpu()))
    with pytest.raises(ValueError):
        query.mesh_orient(sg, query.mesh_topology(_case("tetra", hip, bunny_small)[1]))
    o = query.mesh_orient(sg, topo)
    with pytest.raises(ValueError):
        query.rewind(sg, rows[:-1], o)
    with pytest.raises(TypeError):
        query.rewind(sg, rows.to(torch.float64), o)
    with pytest.raises(ValueError):
        query.rewind(sg, rows, o._replace(flip=o.flip[:-1]))
    with pytest.raises(TypeError):
        query.rewind(sg, rows, o._replace(flip=o.flip.to(torch.int32)))

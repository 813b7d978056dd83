"""Vertex weld and smooth normals on device tensors (include/ezrt_vertices.h, ezrt_amd/query.py: mesh_weld, mesh_weld_at,
vertex_normals, indexed_mesh, euler_characteristic).

Every output of the weld -- vertex, vert_corner, star_offsets, star, fans, vert_flags, summary, and `same` of the rule for pairs -- is
compared EXACTLY with tests/weld_expected.py, the header's rule restated with dictionaries and held to its properties by
tests/test_weld_expected.py; the normals are compared ON THE BITS with its float32 numpy and, on the three meshes in the OBJ's order,
with the host's readObj.  There is no tolerance.  (A NaN is a NaN: the sign and payload that x86 and the device give the NaN of
0 * inf are no part of the rule.)

* every scene of tests/topology_scenes.py and tests/weld_scenes.py over poisoned buffers with room behind them: what the call must not
  touch (entries at and beyond V and L, the room, the bytes behind `work`) still holds the poison;
* the flags group, NULL and not; `work` pre-filled with zeros, with 0xFF and with random bytes; a side stream;
* the rule for pairs on random pairs and on ids out of range;
* the normals: floats 0-8 and 18-35 of every row and a guard row behind the array unchanged on the bits; weld arrays overwritten with
  ids out of range, descending offsets and INT32_MIN / INT32_MAX give the face normal at every corner (N4);
* the loop this is for: weld, deform, vertex_normals, refit, and query.surface against a scene created from the restatement's rows;
* the error contract, the wrappers, euler_characteristic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topology_expected as TE  # noqa: E402
import topology_scenes as TS  # noqa: E402
import weld_expected as WE  # noqa: E402
import weld_scenes as WS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
POISON = -7
POISON8 = 249
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A
OUT32 = ("vertex", "vert_corner", "star_offsets", "star", "fans")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, the device scene, the restatement's weld), computed once and shared"""
    if name not in _cache:
        tri, nodes = WS.scene(name, bunny_small)
        _cache[name] = (tri, hip.scene_create(tri, nodes), WE.weld(tri))
    return _cache[name]


def _raw(lib, sg, n_tri, dev, flags=True, work_fill=FILL, stream=None):
    """the C call itself over poisoned buffers: dict of numpy arrays, each with ROOM entries behind its stated size"""
    H = 3 * n_tri
    out = {k: torch.full((H + (1 if k == "star_offsets" else 0) + ROOM,), POISON, dtype=torch.int32, device=dev) for k in OUT32}
    out["vert_flags"] = torch.full((H + ROOM,), POISON8, dtype=torch.uint8, device=dev)
    out["summary"] = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_weld_work_bytes(n_tri)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:                                                                      # a generator: random bytes
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    torch.cuda.synchronize()
    d = lambda k, on=True: P(out[k].data_ptr()) if on else None
    got = lib.ezrt_mesh_weld_device(sg._h, d("vertex"), d("vert_corner"), d("star_offsets"), d("star"), d("fans", flags), d("vert_flags", flags),
                                    d("summary"), P(work.data_ptr()), wb, P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((work[wb // 8:] == tail).all())                                # nothing behind the stated bytes of work
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, n_tri, what="", flags=True):
    """every output against the restatement's, and the poison wherever the call must not write"""
    H = 3 * n_tri
    L, V = int(want.summary[0]), int(want.summary[1])
    exp = {"vertex": (want.vertex, H), "vert_corner": (want.vert_corner, V), "star_offsets": (want.star_offsets, V + 1), "star": (want.star, L),
           "fans": (want.fans if flags else None, V), "vert_flags": (want.vert_flags if flags else None, V)}
    for k, (w, size) in exp.items():
        poison = POISON8 if k == "vert_flags" else POISON
        if w is None:
            assert (got[k] == poison).all(), "%s: %s was written" % (what, k)
            continue
        assert w.shape[0] == size
        diff = got[k][:size] != w
        assert not diff.any(), "%s: %s differs at %d entries, first at %d: %r, not %r" % (
            what, k, int(diff.sum()), int(np.argmax(diff)), got[k][:size][diff][:4], w[diff][:4])
        assert (got[k][size:] == poison).all(), "%s: %s was written at or beyond %d" % (what, k, size)
    summary = want.summary.copy()
    if not flags:
        summary[3:6] = 0
    assert np.array_equal(got["summary"][:8], summary), "%s: summary %r, not %r" % (what, got["summary"][:8], summary)
    assert (got["summary"][8:] == POISON).all(), what


@pytest.mark.parametrize("name", WS.GPU_NAMES)
def test_weld_on_the_bits(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    assert sg.stats()["n_tri"] == n
    _same(_raw(hip.lib, sg, n, dev), want, n, name)
    if name == "two_discs":
        assert want.summary[2] == 600 and want.summary[5] == 1                  # one star across ten waves, two fans
    if name == "not_nested":
        assert np.array_equal(want.summary, _case("bunny", hip, bunny_small)[2].summary)   # nothing depends on the tree


@pytest.mark.parametrize("name", ("nasty", "dead", "bowtie_vertex", "torus", "two_discs"))
def test_the_flags_group_is_optional(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    for flags in (False, True):
        _same(_raw(hip.lib, sg, n, dev, flags=flags), want, n, "%s flags=%r" % (name, flags), flags=flags)


@pytest.mark.parametrize("name", ("torus", "strip", "dup200", "nasty", "disc300"))
def test_what_work_holds_means_nothing(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    side = torch.cuda.Stream(dev)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("random", np.random.default_rng(WS.SEED + 11))):
        _same(_raw(hip.lib, sg, n, dev, work_fill=fill), want, n, "%s work=%s" % (name, what))
    _same(_raw(hip.lib, sg, n, dev, work_fill=-1, stream=side), want, n, "%s on a side stream" % name)


def _g(x, dev, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


@pytest.mark.parametrize("name", ("nasty", "dead", "signed_zero", "two_discs", "voxel_solid"))
def test_the_rule_for_pairs(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    H = 3 * tri.shape[0]
    rng = np.random.default_rng(WS.SEED + 13)
    k = 4000
    a, b = rng.integers(-2, H + 2, k), rng.integers(-2, H + 2, k)
    a[:8], b[:8] = [-1, H, 0, 0, -2 ** 31, 2 ** 31 - 1, 0, 0], [0, 0, -1, H, 0, 0, -2 ** 31, 2 ** 31 - 1]
    star = want.star[:k // 2]                                                  # ... and pairs that are one vertex
    a[8:8 + star.size], b[8:8 + star.size] = star, np.roll(star, 1)
    same = query.mesh_weld_at(sg, _g(a, dev), _g(b, dev))
    torch.cuda.synchronize()
    assert same.dtype == torch.int8 and tuple(same.shape) == (k,)
    w = WE.at(tri, a, b)
    assert np.array_equal(same.cpu().numpy(), w) and (w[:8] == -1).all() and (w == 1).any() and (w == 0).any()
    va = np.concatenate([want.vertex, [-1, -1]])
    ai, bi = np.clip(a, -1, H), np.clip(b, -1, H)
    assert np.array_equal(w, np.where((va[ai] < 0) | (va[bi] < 0), -1, va[ai] == va[bi]))
    side = torch.cuda.Stream(dev)                                              # a [2, 3] shape on a side stream
    side.wait_stream(torch.cuda.current_stream(dev))
    a2 = (np.arange(6).reshape(2, 3) * 7) % H
    same = query.mesh_weld_at(sg, _g(a2, dev), _g((a2 + 3) % H, dev), stream=side)
    torch.cuda.synchronize()
    assert tuple(same.shape) == (2, 3) and np.array_equal(same.cpu().numpy().ravel(), WE.at(tri, a2.ravel(), ((a2 + 3) % H).ravel()))


# ---- the normals

def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_bits(got, want, what=""):
    """equal on the bits; a NaN is a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    diff = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), "%s: %d of %d floats differ, first at %r: %r, not %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0], got[diff][:4], want[diff][:4])


def _normals_raw(lib, sg, tri, dev, vertex, offsets, star, stream=None):
    """the C call over the rows `tri` with a guard row behind them and full-size weld arrays; the rows afterwards"""
    n = tri.shape[0]
    H = 3 * n
    full = lambda x, size: np.concatenate([np.asarray(x, np.int32).ravel(), np.zeros(size - np.size(x), np.int32)])
    rows = np.concatenate([tri, np.full((1, 36), 12345.0, np.float32)])
    rows[:n, 9:18] = 77.0                                                      # what the rows held as normals means nothing
    d_rows = torch.from_numpy(rows).to(dev)
    d_v, d_o, d_s = _g(full(vertex, H), dev), _g(full(offsets, H + 1), dev), _g(full(star, H), dev)
    wb = lib.ezrt_vertex_normals_work_bytes(n)
    work = torch.full((wb // 8 + ROOM,), FILL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    got = lib.ezrt_vertex_normals_device(sg._h, P(d_rows.data_ptr()), n, P(d_v.data_ptr()), P(d_o.data_ptr()), P(d_s.data_ptr()),
                                         P(work.data_ptr()), wb, P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((work[wb // 8:] == FILL).all())
    out = d_rows.cpu().numpy()
    assert np.array_equal(bits(out[:n, :9]), bits(tri[:, :9])) and np.array_equal(bits(out[:n, 18:]), bits(tri[:, 18:]))
    assert np.array_equal(bits(out[n]), bits(rows[n]))                         # the guard row
    return out[:n]


@pytest.mark.parametrize("name", WS.GPU_NAMES)
def test_normals_on_the_bits(hip, bunny_small, dev, name):
    tri, sg, w = _case(name, hip, bunny_small)
    want = WE.normals(tri, w.vertex, w.star_offsets, w.star)
    got = _normals_raw(hip.lib, sg, tri, dev, w.vertex, w.star_offsets, w.star)
    _same_bits(got[:, 9:18], want, name)
    if name in WS.OBJ:                                                         # the host's readObj, every corner
        assert np.array_equal(bits(got[:, 9:18]), bits(tri[:, 9:18])), name
    if name == "dead":
        assert np.isnan(got[TS.SLIVER_ID, 9:18]).all() and np.isfinite(got[2, 12:18]).all()   # (triangle 2: origin, P1, P2)


def test_normals_of_moved_rows_on_a_side_stream(hip, bunny_small, dev):
    """positions come from the caller's rows, not from the scene"""
    tri, sg, w = _case("obj_sphere", hip, bunny_small)
    moved = np.array(tri)
    P3 = moved[:, :9].reshape(-1, 3)                                           # (a copy: the columns are not contiguous)
    moved[:, :9] = (P3 * np.float32(1.25) + np.float32(0.125) * np.sin(P3[:, [1, 2, 0]] * np.float32(3.0))).astype(np.float32).reshape(-1, 9)
    assert np.array_equal(WE.weld(moved).vertex, w.vertex)                     # the deformation keeps which corners coincide
    want = WE.normals(moved, w.vertex, w.star_offsets, w.star)
    side = torch.cuda.Stream(dev)
    got = _normals_raw(hip.lib, sg, moved, dev, w.vertex, w.star_offsets, w.star, stream=side)
    _same_bits(got[:, 9:18], want, "moved")
    assert (bits(want) != bits(tri[:, 9:18])).any()


def test_weld_arrays_that_are_not_usable_give_the_face_normal(hip, bunny_small, dev):
    """N4 as a contract, on 64 triangles"""
    tri = np.array(WS.rows("obj_sphere")[:64])
    sg = hip.scene_create(tri, WS.proxy_nodes(64))
    n, H = 64, 192
    w = WE.weld(tri)
    fn = np.repeat(WE.face_normals(tri), 3, axis=0).reshape(n, 9)
    full = lambda x, size: np.concatenate([x, np.zeros(size - x.size, np.int32)])
    vertex, off, star = w.vertex, full(w.star_offsets, H + 1), full(w.star, H)
    good = _normals_raw(hip.lib, sg, tri, dev, vertex, off, star)[:, 9:18]
    _same_bits(good, WE.normals(tri, vertex, off, star), "usable")
    assert (bits(good) != bits(fn)).any()
    i32 = np.int32
    cases = [("vertex = %d" % b, np.full(H, b, i32), off, star) for b in (-1, -2, H, 2 ** 31 - 1, -2 ** 31)]
    cases += [("descending offsets", vertex, np.arange(H + 1, 0, -1, dtype=i32), star), ("offsets = -1", vertex, np.full(H + 1, -1, i32), star),
              ("offsets = INT32_MAX", vertex, np.full(H + 1, 2 ** 31 - 1, i32), star), ("offsets = INT32_MIN", vertex, np.full(H + 1, -2 ** 31, i32), star),
              ("offsets beyond 3 n_tri", vertex, off + i32(H), star)]
    cases += [("star = %d" % b, vertex, off, np.full(H, b, i32)) for b in (-1, H, 2 ** 31 - 1, -2 ** 31)]
    rng = np.random.default_rng(WS.SEED + 17)
    cases.append(("random", rng.integers(-2 ** 31, 2 ** 31 - 1, H).astype(i32), rng.integers(-2 ** 31, 2 ** 31 - 1, H + 1).astype(i32),
                  rng.integers(-2 ** 31, 2 ** 31 - 1, H).astype(i32)))
    for what, v, o, s in cases:
        got = _normals_raw(hip.lib, sg, tri, dev, v, o, s)[:, 9:18]            # (the guards are checked in there)
        _same_bits(got, WE.normals(tri, v, o, s), what)
        if what != "random":
            assert np.array_equal(bits(got), bits(fn)), what                   # every corner comes out as its face normal
    # one bad entry spoils exactly the corners of its vertex
    star2 = star.copy()
    star2[off[5]] = H
    got = _normals_raw(hip.lib, sg, tri, dev, vertex, off, star2)[:, 9:18]
    _same_bits(got, WE.normals(tri, vertex, off, star2), "one bad entry")
    spoiled = (vertex == 5).repeat(3).reshape(n, 9)
    assert np.array_equal(bits(got)[spoiled], bits(fn)[spoiled]) and np.array_equal(bits(got)[~spoiled], bits(good)[~spoiled])


def test_deform_normals_refit_render(hip, bunny_small, dev):
    """the loop this is for: weld once; per step deform, vertex_normals, refit -- against a scene created from the restatement's rows"""
    tri, nodes = bunny_small.tri, bunny_small.nodes
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
    sg = hip.scene_create(tri, nodes)
    weld = query.mesh_weld(sg)
    w = WE.weld(tri)
    assert weld.n_vert == w.summary[1] and np.array_equal(weld.vertex.cpu().numpy().ravel(), w.vertex)
    d_tri = torch.from_numpy(tri).to(dev)
    pos = d_tri[:, :9].reshape(-1, 3)                                          # (a copy: the columns are not contiguous)
    pos = pos + 0.03125 * torch.sin(pos[:, [1, 2, 0]] * 4.0)                   # a smooth function of position: equal vertices stay equal
    d_tri[:, :9] = pos.reshape(-1, 9)
    moved = d_tri.cpu().numpy()
    assert np.array_equal(WE.weld(moved).vertex, w.vertex) and (bits(moved[:, :9]) != bits(tri[:, :9])).any()
    out = query.vertex_normals(sg, d_tri, weld)
    assert out is d_tri
    refit.refit(sg, d_tri)
    want_rows = moved.copy()
    want_rows[:, 9:18] = WE.normals(moved, w.vertex, w.star_offsets, w.star)
    _same_bits(d_tri.cpu().numpy(), want_rows, "the rows that went into the refit")
    fresh = hip.scene_create(want_rows, refit.refit_nodes(want_rows, nodes))   # what a refitted scene answers as (ezrt_refit.h)
    rng = np.random.default_rng(WS.SEED + 19)
    k = 400
    lo, hi = moved[:, :9].reshape(-1, 3).min(0), moved[:, :9].reshape(-1, 3).max(0)
    o = rng.uniform(lo - 1.0, hi + 1.0, (k, 3))
    t = rng.uniform(lo, hi, (k, 3))
    rays = torch.from_numpy(np.concatenate([o, t - o], 1).astype(np.float32)).to(dev)
    a, b = query.surface(sg, rays), query.surface(fresh, rays)
    torch.cuda.synchronize()
    tid = a.tri.cpu().numpy()
    hit = tid >= 0
    assert hit.sum() > 100 and np.array_equal(tid, b.tri.cpu().numpy())
    got = a.normal.cpu().numpy()
    _same_bits(got, b.normal.cpu().numpy(), "shading normals")
    # smooth: at most hits the shading normal is not the flat normal (of either side) that the rows would carry without the call
    flat = WE.face_normals(moved)[tid[hit]]
    off_flat = np.minimum(np.abs(got[hit] - flat).max(1), np.abs(got[hit] + flat).max(1))
    assert (off_flat > 1e-4).mean() > 0.5


def test_the_wrappers(hip, bunny_small, dev):
    for name, chi, manifold in (("tetra", 2, True), ("torus", 0, True), ("bowtie_vertex", 3, False), ("voxel_solid", 0, True)):
        tri, sg, want = _case(name, hip, bunny_small)
        n = tri.shape[0]
        for kw in ({}, {"flags": False}, {"stream": torch.cuda.Stream(dev)}):
            w = query.mesh_weld(sg, **kw)
            torch.cuda.synchronize()
            flags = kw.get("flags", True)
            assert w.vertex.dtype == torch.int32 and tuple(w.vertex.shape) == (n, 3) and w.n_vert == want.summary[1]
            for k in ("vertex", "vert_corner", "star_offsets", "star"):
                assert np.array_equal(getattr(w, k).cpu().numpy().ravel(), getattr(want, k)), (name, k)
            if flags:
                assert np.array_equal(w.fans.cpu().numpy(), want.fans) and np.array_equal(w.vert_flags.cpu().numpy(), want.vert_flags)
                assert w.vert_flags.dtype == torch.uint8 and w.manifold_vertices is manifold
            else:
                assert w.fans is None and w.vert_flags is None and w.manifold_vertices is None
            summary = want.summary.copy()
            if not flags:
                summary[3:6] = 0
            assert np.array_equal(w.summary.cpu().numpy(), summary) and w.summary.dtype == torch.int64
        topo = query.mesh_topology(sg)
        assert query.euler_characteristic(w, topo) == chi, name
        assert (topo.closed and w.manifold_vertices) == (name != "bowtie_vertex")   # a closed 2-manifold
        # the indexed mesh gives the triangles back on the bits
        d_tri = torch.from_numpy(tri).to(dev)
        pos, faces = query.indexed_mesh(w, d_tri)
        assert tuple(pos.shape) == (w.n_vert, 3) and tuple(faces.shape) == (n, 3)
        back = pos[faces.to(torch.int64)].reshape(n, 9).cpu().numpy()
        V = tri[:, :9] + np.float32(0)                                         # (-0 is +0)
        assert np.array_equal(back + np.float32(0), V)
        # vertex_normals through the wrapper, with trimmed views and with trimmed copies
        want_n = WE.normals(tri, want.vertex, want.star_offsets, want.star)
        for weld in (w, query.MeshWeld(w.vertex.clone(), w.vert_corner.clone(), w.star_offsets.clone(), w.star.clone(), None, None, w.summary, w.n_vert, None)):
            rows = torch.from_numpy(tri).to(dev)
            assert query.vertex_normals(sg, rows, weld) is rows
            torch.cuda.synchronize()
            _same_bits(rows.cpu().numpy()[:, 9:18], want_n, name)


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
    w = query.mesh_weld(sg)
    query.mesh_weld_at(sg, torch.zeros(4, dtype=torch.int32, device=dev), torch.ones(4, dtype=torch.int32, device=dev))
    query.vertex_normals(sg, torch.from_numpy(np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)).to(dev), w)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    assert np.array_equal(w.summary.cpu().numpy(), _case("bunny", hip, bunny_small)[2].summary)


def test_errors(hip, oracle, bunny_small, dev):
    tri, sg, want = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = tri.shape[0]
    H = 3 * n
    f = lib.ezrt_mesh_weld_device
    wb = lib.ezrt_weld_work_bytes(n)
    i32 = lambda k: torch.full((k,), 5, dtype=torch.int32, device=dev)
    bufs = dict(vertex=i32(H), vert_corner=i32(H), star_offsets=i32(H + 1), star=i32(H), fans=i32(H),
                vert_flags=torch.full((H,), 5, dtype=torch.uint8, device=dev), summary=torch.full((8,), 5, dtype=torch.int64, device=dev),
                work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    keys = list(bufs)
    host = np.zeros(max(wb // 8 + 1, 36 * n), np.int64)
    torch.cuda.synchronize()
    hp = P(host.ctypes.data)

    def fa(**kw):
        args = [kw.get("s", sg._h)]
        args += [kw[k] if k in kw else P(bufs[k].data_ptr()) for k in keys]
        return args + [kw.get("work_bytes", wb), None]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((bufs[k] == 5).all()) for k in keys if k != "work")
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ("s", "vertex", "vert_corner", "star_offsets", "star", "summary", "work"):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID, k
    for k in ("fans", "vert_flags"):                                           # a half-NULL flags group
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"together" in lib.ezrt_last_error(), k
    for k in keys:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert not host.any() and untouched()
    # the rule for pairs
    g = lib.ezrt_mesh_weld_at_device
    ids = torch.zeros(16, dtype=torch.int32, device=dev)
    o8 = torch.full((16,), 5, dtype=torch.int8, device=dev)
    d = lambda t: P(t.data_ptr())
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("corner_a", d(ids)), kw.get("corner_b", d(ids)), kw.get("n", 16), kw.get("same", d(o8)), None]
    for k in ("s", "corner_a", "corner_b", "same"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID, k
        if k != "s":
            assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert g(*ga(n=-1)) == EZRT_ERR_INVALID and g(*ga(n=0)) == 0
    torch.cuda.synchronize()
    assert bool((o8 == 5).all()) and not host.any()
    # the normals
    h = lib.ezrt_vertex_normals_device
    nb = lib.ezrt_vertex_normals_work_bytes(n)
    rows = torch.from_numpy(tri).to(dev)
    nbufs = dict(tri36=rows, vertex=i32(H), star_offsets=i32(H + 1), star=i32(H), work=torch.zeros(nb // 8 + 1, dtype=torch.int64, device=dev))
    na = lambda **kw: [kw.get("s", sg._h), kw.get("tri36", d(nbufs["tri36"])), kw.get("n_tri", n), kw.get("vertex", d(nbufs["vertex"])),
                       kw.get("star_offsets", d(nbufs["star_offsets"])), kw.get("star", d(nbufs["star"])), kw.get("work", d(nbufs["work"])),
                       kw.get("work_bytes", nb), None]
    for k in ("s", "tri36", "vertex", "star_offsets", "star", "work"):
        assert h(*na(**{k: None})) == EZRT_ERR_INVALID, k
        if k != "s":
            assert h(*na(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    for bad in (n - 1, n + 1, 0, -1):
        assert h(*na(n_tri=bad)) == EZRT_ERR_INVALID and b"n_tri" in lib.ezrt_last_error(), bad
    assert h(*na(work_bytes=nb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert h(*na(work=P(nbufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bits(rows.cpu().numpy()), bits(tri)) and not host.any()
    # the rejected calls left no HIP error behind: the next call works
    _same(_raw(lib, sg, n, dev), want, n, "after the rejected calls")
    # the wrappers
    with pytest.raises(TypeError):
        query.mesh_weld(bunny_small.upload(oracle))
    with pytest.raises(TypeError):
        query.mesh_weld_at(sg, ids.to(torch.int64), ids)
    with pytest.raises(TypeError):
        query.mesh_weld_at(sg, ids.cpu(), ids)
    with pytest.raises(ValueError):
        query.mesh_weld_at(sg, ids, ids[:8])
    w = query.mesh_weld(sg)
    with pytest.raises(ValueError):
        query.vertex_normals(sg, rows[:-1], w)
    with pytest.raises(TypeError):
        query.vertex_normals(sg, rows.to(torch.float64), w)
    with pytest.raises(ValueError):
        query.euler_characteristic(w, query.mesh_topology(_case("tetra", hip, bunny_small)[1]))

"""Mesh topology on device tensors (include/ezrt_topology.h, ezrt_amd/query.py: mesh_topology, mesh_topology_at).

Every output -- twin, edge_class, mult, root, component, comp_root, comp_size, comp_flags, summary, and shared / opposite of the rule
for pairs -- is compared EXACTLY with tests/topology_expected.py, the header's rule restated with dictionaries and held to its
properties by tests/test_topology_expected.py; there is no tolerance:

* every scene of tests/topology_scenes.py, not_nested included, over poisoned buffers with room behind them: what the call must not
  touch (comp_* at and beyond C, the room, the bytes behind `work`) still holds the poison.  The torus' 24 576 half-edges are 96
  workgroups of one launch on every XCD; the strip is one component of large diameter under shuffled ids;
* mult and the component group, NULL and not;
* `work` pre-filled with zeros, with 0xFF and with random bytes, and a side stream;
* a refit that moves one vertex of one triangle of the tetrahedron, and back;
* the rule for pairs on random pairs, on all (h, twin[h]) and on ids out of range;
* the error contract, the wrappers, closed / oriented."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topology_expected as TE  # noqa: E402
import topology_scenes as TS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
POISON = -7
POISON8 = 249
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A
OUT32 = ("twin", "mult", "root", "component", "comp_root", "comp_size")
OUT8 = ("edge_class", "comp_flags")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, the device scene, the restatement's topology), computed once and shared"""
    if name not in _cache:
        tri, nodes = TS.scene(name, bunny_small)
        _cache[name] = (tri, hip.scene_create(tri, nodes), TE.topology(tri))
    return _cache[name]


def _raw(lib, sg, n_tri, dev, mult=True, components=True, work_fill=FILL, stream=None):
    """the C call itself over poisoned buffers: dict of numpy arrays, each with ROOM entries behind its stated size"""
    size = {"twin": 3 * n_tri, "edge_class": 3 * n_tri, "mult": 3 * n_tri}
    out = {k: torch.full((size.get(k, n_tri) + ROOM,), POISON, dtype=torch.int32, device=dev) for k in OUT32}
    out.update({k: torch.full((size.get(k, n_tri) + ROOM,), POISON8, dtype=torch.uint8, device=dev) for k in OUT8})
    out["summary"] = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_topology_work_bytes(n_tri)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        work = torch.full((wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:                                                                      # a generator: random bytes
        work = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, wb // 8 + ROOM, dtype=np.int64)).to(dev)
    tail = work[wb // 8:].clone()
    torch.cuda.synchronize()
    d = lambda k, on=True: P(out[k].data_ptr()) if on else None
    got = lib.ezrt_mesh_topology_device(sg._h, d("twin"), d("edge_class"), d("mult", mult), d("root", components), d("component", components),
                                        d("comp_root", components), d("comp_size", components), d("comp_flags", components), d("summary"),
                                        P(work.data_ptr()), wb, P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()
    torch.cuda.synchronize()
    assert bool((work[wb // 8:] == tail).all())                                # nothing behind the stated bytes of work
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want, n_tri, what="", mult=True, components=True):
    """every output against the restatement's, and the poison wherever the call must not write"""
    H = 3 * n_tri
    C_ = int(want.summary[6]) if components else 0
    exp = {"twin": (want.twin, H), "edge_class": (want.edge_class, H), "mult": (want.mult if mult else None, H),
           "root": (want.root if components else None, n_tri), "component": (want.component if components else None, n_tri),
           "comp_root": (want.comp_root if components else None, C_), "comp_size": (want.comp_size if components else None, C_),
           "comp_flags": (want.comp_flags if components else None, C_)}
    for k, (w, size) in exp.items():
        poison = POISON8 if k in OUT8 else POISON
        if w is None:
            assert (got[k] == poison).all(), "%s: %s was written" % (what, k)
            continue
        diff = got[k][:size] != w[:size]
        assert not diff.any(), "%s: %s differs at %d entries, first at %d: %r, not %r" % (
            what, k, int(diff.sum()), int(np.argmax(diff)), got[k][:size][diff][:4], w[:size][diff][:4])
        assert (got[k][size:] == poison).all(), "%s: %s was written at or beyond %d" % (what, k, size)
    summary = want.summary.copy()
    if not components:
        summary[6] = 0
    assert np.array_equal(got["summary"][:8], summary), "%s: summary %r, not %r" % (what, got["summary"][:8], summary)
    assert (got["summary"][8:] == POISON).all(), what


@pytest.mark.parametrize("name", TS.GPU_NAMES)
def test_topology_on_the_bits(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    assert sg.stats()["n_tri"] == n
    _same(_raw(hip.lib, sg, n, dev), want, n, name)
    if name == "torus":
        assert 3 * n == 96 * 256 and want.summary[6] == 1
    if name == "not_nested":
        assert np.array_equal(want.summary, _case("bunny", hip, bunny_small)[2].summary)   # nothing depends on the tree


@pytest.mark.parametrize("name", ("nasty", "dead", "bowtie_vertex", "torus"))
def test_optional_outputs(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    for mult in (False, True):
        for components in (False, True):
            _same(_raw(hip.lib, sg, n, dev, mult=mult, components=components), want, n, "%s mult=%r components=%r" % (name, mult, components),
                  mult=mult, components=components)


@pytest.mark.parametrize("name", ("torus", "strip", "dup200", "nasty"))
def test_what_work_holds_means_nothing(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    side = torch.cuda.Stream(dev)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("random", np.random.default_rng(TS.SEED + 11))):
        _same(_raw(hip.lib, sg, n, dev, work_fill=fill), want, n, "%s work=%s" % (name, what))
    _same(_raw(hip.lib, sg, n, dev, work_fill=-1, stream=side), want, n, "%s on a side stream" % name)


def test_after_a_refit(hip, dev):
    tri, nodes = TS.build(TS.tetra())
    sg = hip.scene_create(tri, nodes)
    n = tri.shape[0]
    before = TE.topology(tri)
    _same(_raw(hip.lib, sg, n, dev), before, n, "before the refit")
    moved = tri.copy()
    moved[2, 3:6] += np.float32(0.25)                                          # vertex 1 of triangle 2 leaves its two edges
    after = TE.topology(moved)
    assert list(before.summary) == [4, 6, 0, 6, 0, 0, 1, 2] and list(after.summary) == [4, 8, 4, 4, 0, 0, 1, 2]
    refit.refit(sg, moved)
    _same(_raw(hip.lib, sg, n, dev), after, n, "after the refit")
    topo = query.mesh_topology(sg)
    assert not topo.closed and topo.oriented
    refit.refit(sg, tri)
    _same(_raw(hip.lib, sg, n, dev), before, n, "refitted back")
    assert query.mesh_topology(sg).closed


def _at(sg, dev, a, e, b, stream=None):
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev)
    sh, op = query.mesh_topology_at(sg, g(a), g(e), g(b), stream=stream)
    torch.cuda.synchronize()
    assert sh.dtype == torch.int8 and op.dtype == torch.int8 and tuple(sh.shape) == tuple(np.shape(a))
    return sh.cpu().numpy(), op.cpu().numpy()


@pytest.mark.parametrize("name", ("nasty", "dead", "book5", "signed_zero", "moebius", "voxel_solid"))
def test_the_rule_for_pairs(hip, bunny_small, dev, name):
    tri, sg, want = _case(name, hip, bunny_small)
    n = tri.shape[0]
    rng = np.random.default_rng(TS.SEED + 13)
    # random pairs, ids and edges out of range among them
    k = 4000
    a, b, e = rng.integers(-2, n + 2, k), rng.integers(-2, n + 2, k), rng.integers(-1, 4, k)
    a[:8], b[:8] = [-1, n, 0, 0, -2 ** 31, 2 ** 31 - 1, 0, 0], [0, 0, -1, n, 0, 0, -2 ** 31, 2 ** 31 - 1]
    e[:8] = 0
    e[8:12], a[8:12], b[8:12] = [-1, 3, -2 ** 31, 2 ** 31 - 1], 0, 0
    sh, op = _at(sg, dev, a, e, b)
    wsh, wop = TE.at(tri, a, e, b)
    assert np.array_equal(sh, wsh) and np.array_equal(op, wop)
    assert (sh[:12] == -1).all() and (op[:12] == -1).all()
    # every pair the topology names
    h = np.nonzero(want.twin >= 0)[0]
    sh, op = _at(sg, dev, h // 3, h % 3, want.twin[h] // 3)
    wsh, wop = TE.at(tri, h // 3, h % 3, want.twin[h] // 3)
    assert np.array_equal(sh, wsh) and np.array_equal(op, wop) and np.array_equal(sh, want.twin[h] % 3) and h.size > 0
    manifold = want.edge_class[h] == TE.MANIFOLD
    assert (op[manifold] == 1).all() and (op[want.edge_class[h] == TE.FLIPPED] == 0).all()
    # neighbours across an edge, and triangles that share none; a [2, 3] shape on a side stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    a2 = np.arange(6).reshape(2, 3) % n
    sh, op = _at(sg, dev, a2, a2 % 3, (a2 + 1) % n, stream=side)
    wsh, wop = TE.at(tri, a2.ravel(), (a2 % 3).ravel(), ((a2 + 1) % n).ravel())
    assert np.array_equal(sh.ravel(), wsh) and np.array_equal(op.ravel(), wop)


def test_the_wrapper(hip, bunny_small, dev):
    for name, closed, oriented in (("voxel_solid", True, True), ("torus", True, True), ("bunny", False, True), ("tetra_flip", True, False),
                                   ("moebius", False, False), ("dead", False, False)):
        tri, sg, want = _case(name, hip, bunny_small)
        n = tri.shape[0]
        for kw in ({}, {"mult": True}, {"components": False}, {"stream": torch.cuda.Stream(dev), "mult": True}):
            topo = query.mesh_topology(sg, **kw)
            torch.cuda.synchronize()
            assert (topo.closed, topo.oriented) == (closed, oriented) == (TE.closed(want), TE.oriented(want)), name
            assert topo.twin.dtype == torch.int32 and tuple(topo.twin.shape) == (n, 3) and topo.edge_class.dtype == torch.uint8
            assert np.array_equal(topo.twin.cpu().numpy().ravel(), want.twin) and np.array_equal(topo.edge_class.cpu().numpy().ravel(), want.edge_class)
            assert np.array_equal(topo.neighbours.cpu().numpy().ravel(), np.where(want.twin >= 0, want.twin // 3, -1))
            assert tuple(topo.neighbours.shape) == (n, 3) and topo.neighbours.dtype == torch.int32
            if kw.get("mult"):
                assert np.array_equal(topo.mult.cpu().numpy().ravel(), want.mult)
            else:
                assert topo.mult is None
            summary = want.summary.copy()
            if kw.get("components", True):
                for k in ("root", "component", "comp_root", "comp_size", "comp_flags"):
                    assert np.array_equal(getattr(topo, k).cpu().numpy(), getattr(want, k)), (name, k)
                assert topo.comp_flags.dtype == torch.uint8 and tuple(topo.comp_root.shape) == (int(want.summary[6]),)
            else:
                assert topo.root is None and topo.component is None and topo.comp_root is None and topo.comp_size is None and topo.comp_flags is None
                summary[6] = 0
            assert np.array_equal(topo.summary.cpu().numpy(), summary) and topo.summary.dtype == torch.int64


def test_untouched_state(hip, bunny_small, dev):
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    topo = query.mesh_topology(sg, mult=True)
    query.mesh_topology_at(sg, torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev),
                           torch.ones(4, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    assert np.array_equal(topo.summary.cpu().numpy(), _case("bunny", hip, bunny_small)[2].summary)


def test_errors(hip, oracle, bunny_small, dev):
    tri, sg, want = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = tri.shape[0]
    f = lib.ezrt_mesh_topology_device
    wb = lib.ezrt_topology_work_bytes(n)
    i32 = lambda k: torch.full((k,), 5, dtype=torch.int32, device=dev)
    u8 = lambda k: torch.full((k,), 5, dtype=torch.uint8, device=dev)
    bufs = dict(twin=i32(3 * n), edge_class=u8(3 * n), mult=i32(3 * n), root=i32(n), component=i32(n), comp_root=i32(n), comp_size=i32(n),
                comp_flags=u8(n), summary=torch.full((8,), 5, dtype=torch.int64, device=dev),
                work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    keys = list(bufs)
    host = np.zeros(wb // 8 + 1, np.int64)
    torch.cuda.synchronize()
    hp = P(host.ctypes.data)

    def fa(**kw):
        args = [kw.get("s", sg._h)]
        args += [kw[k] if k in kw else P(bufs[k].data_ptr()) for k in keys]
        return args + [kw.get("work_bytes", wb), None]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((bufs[k] == 5).all()) for k in keys if k != "work")
    # work too small, or misaligned
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    # NULL pointers
    for k in ("s", "twin", "edge_class", "summary", "work"):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID, k
    # a partly NULL component group
    group = ("root", "component", "comp_root", "comp_size", "comp_flags")
    for k in group:
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"together" in lib.ezrt_last_error(), k
        assert f(*fa(**{g: None for g in group if g != k})) == EZRT_ERR_INVALID, k
    # host memory is rejected, never read or written
    for k in keys:
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert not host.any()
    assert untouched()
    # the rule for pairs
    g = lib.ezrt_mesh_topology_at_device
    ids = torch.zeros(16, dtype=torch.int32, device=dev)
    o8 = torch.full((16,), 5, dtype=torch.int8, device=dev)
    d = lambda t: P(t.data_ptr())
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("tri_a", d(ids)), kw.get("edge_a", d(ids)), kw.get("tri_b", d(ids)), kw.get("n", 16),
                       kw.get("shared", d(o8)), kw.get("opposite", d(o8)), None]
    for k in ("s", "tri_a", "edge_a", "tri_b", "shared", "opposite"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID, k
        if k != "s":
            assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert g(*ga(n=-1)) == EZRT_ERR_INVALID and g(*ga(n=0)) == 0
    torch.cuda.synchronize()
    assert bool((o8 == 5).all()) and not host.any()
    # the rejected calls left no HIP error behind: the next call works
    _same(_raw(lib, sg, n, dev), want, n, "after the rejected calls")
    # the wrappers
    with pytest.raises(TypeError):
        query.mesh_topology(bunny_small.upload(oracle))
    with pytest.raises(TypeError):
        query.mesh_topology_at(sg, ids.to(torch.int64), ids, ids)
    with pytest.raises(TypeError):
        query.mesh_topology_at(sg, ids.cpu(), ids, ids)
    with pytest.raises(ValueError):
        query.mesh_topology_at(sg, ids, ids[:8], ids)
    with pytest.raises(TypeError):
        query.mesh_topology_at(bunny_small.upload(oracle), ids, ids, ids)

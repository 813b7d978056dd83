"""Plane queries on device tensors (include/ezrt_plane.h, ezrt_amd/query.py: plane_count, plane_section, plane_section_at).

Everything -- offsets, ids, segments, `part`, sides -- is compared ON THE BITS with tests/plane_expected.py, the header's rule restated
in numpy over all triangles and held to exact rational arithmetic by tests/test_plane_expected.py:

* on the voxel solid, the same with faces removed, the Bunny scene, adversarial geometry and a scene that does not prune, with
  tests/plane_scenes.py's planes: through triangle centroids, axis planes exactly through vertex coordinates with both signs, planes
  that miss, planes that are not live (zero normals, NaN, infinities);
* every slicing (1, 2, 7, the clamp, the library's choice): the same answer, and `part` against the restatement's per-slice sums;
* batches of 1 .. 200 planes and a [2, 3, 4] shape; capacities 0, total - 1, total, total + 5 over poisoned rows; seg = NULL and
  offsets = NULL;
* every tree shape a caller can pass (the tree cannot matter: nothing reads it);
* plane_section_at for rows of ids, -1 and ids outside the scene included, and its sum over all ids against plane_count;
* a flipped copy of a scene (q0 and q1 swap, nothing else changes) and the loop guarantee on the closed solid, from device output;
* a refit, stream order, a render call beside it, untouched counters, the error contract."""
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
import plane_scenes as PS  # noqa: E402
import tree_shapes as T  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = PS.GPU_NAMES
P = C.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, planes, kind, want = (offsets, ids, seg, crossed) by the restatement, the device scene), computed once and shared"""
    if name not in _cache:
        tri, nodes, planes, kind = PS.inputs(name, bunny_small)
        _cache[name] = (tri, planes, kind, PE.section(planes, tri), hip.scene_create(tri, nodes))
    return _cache[name]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _section(sg, planes, dev, **kw):
    """(offsets, ids, seg) as numpy, after the checks of the shapes and types"""
    o, t, s = query.plane_section(sg, _gpu(planes, dev), **kw)
    torch.cuda.synchronize()
    n = int(np.prod(planes.shape[:-1]))
    assert o.dtype == torch.int64 and t.dtype == torch.int32 and s.dtype == torch.float32
    assert tuple(o.shape) == (n + 1,) and tuple(s.shape) == (t.shape[0], 2, 3)
    return o.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy()


def _same(got, want, what=""):
    o, t, s = got
    assert np.array_equal(o, want[0]), "%s: offsets differ, first at plane %d" % (what, int(np.argmax(o != want[0])))
    assert t.shape == want[1].shape and np.array_equal(t, want[1]), "%s: ids differ" % what
    bad = (_bits(s) != _bits(want[2])).reshape(-1, 6).any(1)
    assert not bad.any(), "%s: %d of %d rows differ, first at row %d" % (what, int(bad.sum()), bad.size, int(np.argmax(bad)))


def _raw(lib, sg, planes_t, slices, capacity=None, want_seg=True, want_offsets=True, poison=None):
    """the C calls themselves: (S, part, n_cross, offsets, tri_id, seg) as numpy; capacity None = the total"""
    n, dev = planes_t.shape[0], planes_t.device
    n_tri = sg.stats()["n_tri"]
    Sl = lib.ezrt_plane_slices(n, n_tri, slices)
    part = torch.full((n, Sl), -7, dtype=torch.int32, device=dev)
    n_cross = torch.full((n,), -7, dtype=torch.int32, device=dev)
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    assert lib.ezrt_query_plane_count_device(sg._h, P(planes_t.data_ptr()), n, slices, P(part.data_ptr()), P(n_cross.data_ptr()),
                                             P(offsets.data_ptr()) if want_offsets else None, None) == 0
    torch.cuda.synchronize()
    if not want_offsets:
        assert bool((offsets == -7).all())
        return Sl, part.cpu().numpy(), n_cross.cpu().numpy(), None, None, None
    total = int(offsets[n].item())
    cap = total if capacity is None else capacity
    room = max(cap, total) + 8                                          # rows past the capacity exist, so that a stray store would show
    tri_id = torch.full((room,), -9 if poison is None else poison, dtype=torch.int32, device=dev)
    seg = torch.full((room, 6), 123.0, dtype=torch.float32, device=dev)
    assert lib.ezrt_query_plane_section_device(sg._h, P(planes_t.data_ptr()), n, slices, P(part.data_ptr()), P(offsets.data_ptr()), cap,
                                               P(tri_id.data_ptr()), P(seg.data_ptr()) if want_seg else None, None) == 0
    torch.cuda.synchronize()
    return Sl, part.cpu().numpy(), n_cross.cpu().numpy(), offsets.cpu().numpy(), tri_id.cpu().numpy(), seg.cpu().numpy().reshape(-1, 2, 3)


@pytest.mark.parametrize("name", NAMES)
def test_sections_on_the_bits(hip, bunny_small, dev, name):
    tri, planes, kind, want, sg = _case(name, hip, bunny_small)
    assert (sg.prune_info()["mode"] == -1) == (name == "not_nested")   # (a scene that does not prune is swept like any other)
    _same(_section(sg, planes, dev), want, name)
    n_cross = query.plane_count(sg, _gpu(planes, dev))
    torch.cuda.synchronize()
    assert n_cross.dtype == torch.int32 and np.array_equal(n_cross.cpu().numpy(), np.diff(want[0]))
    # the comparison is not of nothing
    rows = np.diff(want[0])
    live = PE.live(planes)
    assert (~live).sum() == 10 and not rows[~live].any() and not rows[kind == PS.KIND_MISS].any()
    assert (rows[live] > 0).sum() >= 0.5 * live.sum()
    zero_len = (_bits(want[2][:, 0]) == _bits(want[2][:, 1])).all(1)
    assert zero_len.any() and not zero_len.all()
    if tri.shape[0] > 1000:
        assert rows.max() > 64                                          # more than any max_k list holds


def test_every_slicing_gives_the_same_bits(hip, bunny_small, dev):
    lib = hip.lib
    for name in ("nasty", "open_solid"):
        tri, planes, kind, want, sg = _case(name, hip, bunny_small)
        n, m = planes.shape[0], tri.shape[0]
        pt = _gpu(planes, dev)
        seen = set()
        for slices in (1, 2, 7, 10 ** 6, 0):
            Sl, part, n_cross, offsets, ids, seg = _raw(lib, sg, pt, slices)
            assert Sl == (PE.slices_of(n, m, slices) if slices else lib.ezrt_plane_slices(n, m, 0)) and part.shape == (n, Sl)
            seen.add(Sl)
            assert np.array_equal(part, PE.part_of(want[3], Sl)), (name, slices)
            assert np.array_equal(n_cross, np.diff(want[0]))
            total = int(want[0][-1])
            _same((offsets, ids[:total], seg[:total]), want, "%s slices=%d" % (name, slices))
            assert (ids[total:] == -9).all() and (seg[total:] == 123.0).all()
            _same(_section(sg, planes, dev, slices=slices if slices else None), want, "%s slices=%d, wrapper" % (name, slices))
        assert len(seen) >= 3 and -(-m // 64) in seen
    tri, planes, kind, want, sg = _case("nasty", hip, bunny_small)      # 2 812 triangles: the library's choice is ten slices of 320
    assert lib.ezrt_plane_slices(planes.shape[0], tri.shape[0], 0) == 10


def test_batch_sizes_and_shapes(hip, bunny_small, dev):
    for name in ("nasty", "voxel_solid"):                              # 2 812 and 288 triangles: no multiple of 64
        tri, planes, kind, want, sg = _case(name, hip, bunny_small)
        assert tri.shape[0] % 64 != 0
        cr = want[3]
        for n in (1, 63, 64, 65, _abi.PLANE_TILE + 1, 129, 200):
            sel = np.arange(n) * 7 % planes.shape[0]
            w = PE.section(planes[sel], tri)
            assert np.array_equal(w[3], cr[sel])
            _same(_section(sg, planes[sel], dev), w, "%s n=%d" % (name, n))
            _same(_section(sg, planes[sel], dev, slices=3), w, "%s n=%d, three slices" % (name, n))
        lead = planes[10:34].reshape(2, 3, 4, 4)
        w = PE.section(lead, tri)
        _same(_section(sg, lead, dev), w, name)
        c = query.plane_count(sg, _gpu(lead, dev))
        torch.cuda.synchronize()
        assert tuple(c.shape) == (2, 3, 4) and np.array_equal(c.cpu().numpy().reshape(-1), np.diff(w[0]))
        e = query.plane_section(sg, torch.empty((0, 4), device=dev))
        assert tuple(e[0].shape) == (1,) and int(e[0][0]) == 0 and tuple(e[1].shape) == (0,) and tuple(e[2].shape) == (0, 2, 3)
        assert tuple(query.plane_count(sg, torch.empty((3, 0, 4), device=dev)).shape) == (3, 0)


def test_capacity_and_null_outputs(hip, bunny_small, dev):
    tri, planes, kind, want, sg = _case("nasty", hip, bunny_small)
    lib = hip.lib
    pt = _gpu(planes, dev)
    total = int(want[0][-1])
    for slices in (0, 1, 5):
        for cap in (0, total - 1, total, total + 5):
            Sl, part, n_cross, offsets, ids, seg = _raw(lib, sg, pt, slices, capacity=cap)
            k = min(cap, total)
            assert np.array_equal(offsets, want[0])                     # the overflow shows in offsets[n]
            assert np.array_equal(ids[:k], want[1][:k]) and np.array_equal(_bits(seg[:k]), _bits(want[2][:k])), (slices, cap)
            assert (ids[k:] == -9).all() and (seg[k:] == 123.0).all(), (slices, cap)   # rows past the capacity and past the total
        Sl, part, n_cross, offsets, ids, seg = _raw(lib, sg, pt, slices, want_seg=False)
        assert np.array_equal(ids[:total], want[1]) and (seg == 123.0).all()
        Sl, part, n_cross, offsets, _, _ = _raw(lib, sg, pt, slices, want_offsets=False)
        assert offsets is None and np.array_equal(n_cross, np.diff(want[0])) and np.array_equal(part, PE.part_of(want[3], Sl))
    # the wrapper: a given capacity returns that many rows, the unwritten ones with tri == -1
    for cap in (0, total - 1, total + 5):
        o, t, s = _section(sg, planes, dev, capacity=cap)
        k = min(cap, total)
        assert t.shape == (cap,) and np.array_equal(o, want[0]) and np.array_equal(t[:k], want[1][:k]) and (t[k:] == -1).all()
        assert np.array_equal(_bits(s[:k]), _bits(want[2][:k])) and not s[k:].any()


@pytest.mark.parametrize("name", T.HOST_SHAPES + T.LBVH_SHAPES)
def test_every_tree_shape(hip, dev, name):
    tri, nodes, expect = T.shape(name)
    planes, kind = PS.planes_for(tri, 5, n_random=24, n_axis=3)
    want = PE.section(planes, tri)
    sg = hip.scene_create(tri, nodes)
    for slices in (None, 1, 3):
        _same(_section(sg, planes, dev, slices=slices), want, "%s slices=%r" % (name, slices))
    assert (np.diff(want[0]) > 0).sum() >= 24


def test_plane_section_at(hip, bunny_small, dev):
    tri, planes, kind, want, sg = _case("voxel_solid", hip, bunny_small)
    rng = np.random.default_rng(31)
    n, m = planes.shape[0], tri.shape[0]
    pt = _gpu(planes, dev)
    ids = rng.integers(0, m, n).astype(np.int32)
    ids[::9], ids[1::9], ids[2::9] = -1, m, 2 ** 31 - 1
    c, side, seg = query.plane_section_at(sg, pt, _gpu(ids, dev, np.int32))
    rows = rng.integers(-2, m + 2, (n, 40)).astype(np.int32)
    cr, sider, segr = query.plane_section_at(sg, pt, _gpu(rows, dev, np.int32))
    torch.cuda.synchronize()
    assert c.dtype == torch.bool and side.dtype == torch.int8 and seg.dtype == torch.float32
    assert tuple(c.shape) == (n,) and tuple(side.shape) == (n, 3) and tuple(seg.shape) == (n, 2, 3)
    assert tuple(cr.shape) == (n, 40) and tuple(sider.shape) == (n, 40, 3) and tuple(segr.shape) == (n, 40, 2, 3)
    for got, w in (((c, side, seg), PE.section_at(planes, tri, ids)), ((cr, sider, segr), PE.section_at(planes, tri, rows))):
        assert np.array_equal(got[0].cpu().numpy(), w[0]) and np.array_equal(got[1].cpu().numpy(), w[1])
        assert np.array_equal(_bits(got[2].cpu().numpy()), _bits(w[2]))
    w = PE.section_at(planes, tri, rows)
    assert w[0].sum() > 100 and (w[1] == 0).any() and (w[1] == 1).any() and (w[1] == -1).any()
    assert not w[0][rows < 0].any() and not w[1][rows >= m].any() and not w[1][kind == PS.KIND_DEAD].any()
    # crosses of all ids sums to n_cross, and its segments are the section's
    every = torch.arange(m, dtype=torch.int32, device=dev)[None, :].expand(n, m).contiguous()
    ce, _, se = query.plane_section_at(sg, pt, every)
    n_cross = query.plane_count(sg, pt)
    torch.cuda.synchronize()
    assert torch.equal(ce.sum(1).to(torch.int32), n_cross) and np.array_equal(ce.cpu().numpy(), want[3])
    assert np.array_equal(_bits(se[ce].cpu().numpy()), _bits(want[2]))
    e = query.plane_section_at(sg, torch.empty((0, 4), device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev))
    assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 4, 3) and tuple(e[2].shape) == (0, 4, 2, 3)


def test_a_flipped_winding_swaps_the_ends(hip, bunny_small, dev):
    for name in ("voxel_solid", "bunny"):
        tri, planes, kind, want, sg = _case(name, hip, bunny_small)
        nodes = PS.scene(name, bunny_small)[1]
        flipped = hip.scene_create(PE.flipped(tri), nodes)
        o, t, s = _section(flipped, planes, dev)
        assert np.array_equal(o, want[0]) and np.array_equal(t, want[1])
        assert np.array_equal(_bits(s), _bits(want[2][:, ::-1])) and not np.array_equal(_bits(s), _bits(want[2]))


def test_sections_of_the_closed_solid_chain_into_loops(hip, bunny_small, dev):
    tri, planes, kind, want, sg = _case("voxel_solid", hip, bunny_small)
    o, t, s = _section(sg, planes, dev)
    closed = 0
    for i in range(planes.shape[0]):
        q0, q1 = PE.loop_balance(s[o[i]:o[i + 1]])
        assert np.array_equal(q0, q1), i                                # every end point as often a q0 as a q1, on the bits
        closed += o[i + 1] > o[i]
    assert closed >= 70
    z = np.float32([[0, 0, 1, 1.5], [0, 0, -1, -1.5]])
    o, t, s = _section(sg, z, dev)
    assert list(o) == [0, 32, 64] and PE.signed_area(s[:32], z[0]) == 8.0 == PE.signed_area(s[32:], z[1])


def test_after_a_refit(hip, bunny_small, dev):
    v = IS.voxel_solid()
    tri, nodes = v["tri"], v["nodes"]
    planes, _ = PS.planes_for(tri, 3)
    moved = tri.copy()
    shift = np.float32([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + shift
    q = planes.copy()
    with np.errstate(all="ignore"):                                  # (the planes that are not live stay so)
        q[:, 3] = (2 * planes[:, 3].astype(np.float64) + planes[:, :3].astype(np.float64) @ shift).astype(np.float32)   # roughly the moved planes
    sg = hip.scene_create(tri, nodes)
    first = _section(sg, q, dev)
    refit.refit(sg, moved)
    want = PE.section(q, moved)
    _same(_section(sg, q, dev), want, "after the refit")
    _same(_section(sg, q, dev, slices=4), want, "after the refit, sliced")
    assert want[1].size > 1000 and not np.array_equal(first[0], want[0])


def test_stream_order(hip, bunny_small, dev):
    tri, planes, kind, want, sg = _case("nasty", hip, bunny_small)
    src = _gpu(planes, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                   # the planes are written on `side`, behind the sleep
    total = int(want[0][-1])
    a = query.plane_section(sg, p, capacity=total, stream=side)        # issued from the default stream's context, onto `side`
    b = query.plane_section(sg, p, stream=side.cuda_stream)            # a raw handle; synchronises `side` itself for the total
    c = query.plane_count(sg, p, slices=1, stream=side)
    ids = torch.zeros(planes.shape[0], dtype=torch.int32, device=dev)
    d = query.plane_section_at(sg, p, ids, stream=side)
    side.synchronize()
    for got in (a, b):
        _same(tuple(x.cpu().numpy() for x in got), want, "on a side stream")
    assert np.array_equal(c.cpu().numpy(), np.diff(want[0]))
    assert np.array_equal(d[0].cpu().numpy(), PE.section_at(planes, tri, np.zeros(planes.shape[0], np.int32))[0])


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    tri, planes, kind, want, _ = _case("bunny", hip, bunny_small)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    p = _gpu(planes, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    query.plane_count(sg, p)
    query.plane_section(sg, p, slices=1)
    query.plane_section_at(sg, p, torch.zeros(planes.shape[0], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.plane_section(sg, p, capacity=int(want[0][-1]), stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(frame.cpu().numpy()), _bits(alone.cpu().numpy()))
    _same(tuple(x.cpu().numpy() for x in got), want, "beside a render call")


def test_errors(hip, oracle, bunny_small, dev):
    tri, planes, kind, want, sg = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = planes.shape[0]
    p = _gpu(planes, dev)
    Sl = lib.ezrt_plane_slices(n, tri.shape[0], 0)
    total = int(want[0][-1])
    part = torch.zeros((n, Sl), dtype=torch.int32, device=dev)
    nc = torch.zeros(n, dtype=torch.int32, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ids = torch.zeros(total, dtype=torch.int32, device=dev)
    seg = torch.zeros((total, 6), dtype=torch.float32, device=dev)
    cr = torch.zeros(n, dtype=torch.uint8, device=dev)
    side = torch.zeros((n, 3), dtype=torch.int8, device=dev)
    seg_at = torch.zeros((n, 6), dtype=torch.float32, device=dev)
    tid = torch.zeros(n, dtype=torch.int32, device=dev)
    host_p = np.ascontiguousarray(planes)
    host_i32, host_i64, host_f, host_u8 = np.zeros(n * Sl + total, np.int32), np.zeros(n + 1, np.int64), np.zeros(total * 6 + n * 6, np.float32), np.zeros(3 * n, np.uint8)
    f, g, h = lib.ezrt_query_plane_count_device, lib.ezrt_query_plane_section_device, lib.ezrt_plane_section_at_device
    torch.cuda.synchronize()
    d = lambda t: P(t.data_ptr())
    hp = lambda a: P(a.ctypes.data)
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("planes", d(p)), kw.get("n", n), kw.get("slices", 0), kw.get("part", d(part)),
                       kw.get("n_cross", d(nc)), kw.get("offsets", d(off)), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("planes", d(p)), kw.get("n", n), kw.get("slices", 0), kw.get("part", d(part)),
                       kw.get("offsets", d(off)), kw.get("capacity", total), kw.get("tri", d(ids)), kw.get("seg", d(seg)), None]
    ha = lambda **kw: [kw.get("s", sg._h), kw.get("planes", d(p)), kw.get("tri", d(tid)), kw.get("n", n), kw.get("crosses", d(cr)),
                       kw.get("side", d(side)), kw.get("seg", d(seg_at)), None]
    assert f(*fa()) == 0 and g(*ga()) == 0 and h(*ha()) == 0
    assert f(*fa(offsets=None)) == 0 and g(*ga(seg=None)) == 0 and h(*ha(side=None, seg=None)) == 0 and g(*ga(capacity=0, tri=None, seg=None)) == 0
    for slices in (-1, -2 ** 31):
        assert f(*fa(slices=slices)) == EZRT_ERR_INVALID and b"slices" in lib.ezrt_last_error()
        assert g(*ga(slices=slices)) == EZRT_ERR_INVALID and b"slices" in lib.ezrt_last_error()
    assert g(*ga(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    # host memory is rejected, never read or written
    assert f(*fa(planes=hp(host_p))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*fa(part=hp(host_i32))) == EZRT_ERR_INVALID and f(*fa(n_cross=hp(host_i32))) == EZRT_ERR_INVALID
    assert f(*fa(offsets=hp(host_i64))) == EZRT_ERR_INVALID
    assert g(*ga(planes=hp(host_p))) == EZRT_ERR_INVALID and g(*ga(part=hp(host_i32))) == EZRT_ERR_INVALID
    assert g(*ga(offsets=hp(host_i64))) == EZRT_ERR_INVALID and g(*ga(tri=hp(host_i32))) == EZRT_ERR_INVALID
    assert g(*ga(seg=hp(host_f))) == EZRT_ERR_INVALID
    assert h(*ha(planes=hp(host_p))) == EZRT_ERR_INVALID and h(*ha(tri=hp(host_i32))) == EZRT_ERR_INVALID
    assert h(*ha(crosses=hp(host_u8))) == EZRT_ERR_INVALID and h(*ha(side=hp(host_u8))) == EZRT_ERR_INVALID
    assert h(*ha(seg=hp(host_f))) == EZRT_ERR_INVALID
    assert not host_i32.any() and not host_i64.any() and not host_f.any() and not host_u8.any()
    # NULL, n < 0, n == 0
    for k in ("s", "planes", "part", "n_cross"):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID, k
    for k in ("s", "planes", "part", "offsets", "tri"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID, k
    for k in ("s", "planes", "tri", "crosses"):
        assert h(*ha(**{k: None})) == EZRT_ERR_INVALID, k
    assert f(*fa(n=-1)) == EZRT_ERR_INVALID and g(*ga(n=-1)) == EZRT_ERR_INVALID and h(*ha(n=-1)) == EZRT_ERR_INVALID
    part.fill_(5), nc.fill_(5), off.fill_(5), ids.fill_(5), cr.fill_(5)
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0 and h(*ha(n=0)) == 0 and f(*fa(n=0, slices=4)) == 0
    torch.cuda.synchronize()
    for t in (part, nc, off, ids, cr):
        assert bool((t == 5).all())                                    # n == 0 launches nothing
    # the rejected calls left no HIP error behind: the next call works
    _same(_section(sg, planes, dev), want, "after the rejected calls")
    # the wrapper
    with pytest.raises(ValueError):
        query.plane_count(sg, p, slices=0)
    with pytest.raises(ValueError):
        query.plane_section(sg, p, capacity=-1)
    with pytest.raises(TypeError):
        query.plane_count(sg, torch.from_numpy(host_p))
    with pytest.raises(TypeError):
        query.plane_section(bunny_small.upload(oracle), p)
    with pytest.raises(TypeError):
        query.plane_section_at(bunny_small.upload(oracle), p, tid)
    with pytest.raises(ValueError):
        query.plane_count(sg, torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError):
        query.plane_section_at(sg, p, torch.zeros((n + 1,), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        query.plane_section_at(sg, p, torch.zeros((n,), dtype=torch.int64, device=dev))

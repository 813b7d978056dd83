"""Inside and signed-distance queries on device tensors (include/ezrt_inside.h, ezrt_amd/query.py: inside, signed_distance).

`crossings` and `inside` are compared on the bits with tests/inside_expected.py -- the header's rule restated in numpy over ALL
triangles, pinned to the occupancy truth by tests/test_inside_expected.py -- for all six axes:

* on the voxel solid (also against the occupancy grid directly), the Bunny scene, adversarial geometry (slivers, a coplanar grid,
  duplicates, a far cluster) and a scene that does not prune (the sweep route), with tests/closest_point_expected.py's points and a
  third more exactly on vertices, edge midpoints and box planes of the tree;
* the walk against the sweep, batches of 1, 63, 64, 65 and 4000 points, NULL outputs, a [2, 3, 5, 3] shape;
* signed_distance against closest_point on the bits, with and without d_max, the sign against inside, misses +-inf by side;
* a refit, stream order, a render call beside it, untouched counters, the error contract.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import closest_point_expected as E  # noqa: E402
import inside_expected as IE  # noqa: E402
import inside_scenes as IS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
NAMES = ("voxel_solid", "bunny", "nasty", "not_nested")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_cache = {}


def _case(name, hip, bunny_small):
    """(tri, nodes, points, (crossings [6, n], inside [6, n]) by the restatement, the device scene), computed once and shared"""
    if name not in _cache:
        if name == "voxel_solid":
            v = IS.voxel_solid()
            tri, nodes, pts = v["tri"], v["nodes"], v["points"]
        else:
            tri, nodes, _ = A.scene(name, bunny_small)
            seed = 500 + NAMES.index(name)
            base, n_finite = E.points_for(tri, nodes, seed)
            base = np.concatenate([base[:n_finite:3], base[n_finite::4]])        # every kind, the non-finite ones included
            pts = np.ascontiguousarray(np.concatenate([base, IS.surface_points(tri, nodes, seed, base.shape[0] // 2)]), np.float32)
        _cache[name] = (tri, nodes, pts, IE.all_axes(pts, tri), hip.scene_create(tri, nodes))
    return _cache[name]


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _inside(sg, pts, dev, axis, **kw):
    ins, cr = query.inside(sg, _gpu(pts, dev), axis, crossings=True, **kw)
    torch.cuda.synchronize()
    assert ins.dtype == torch.bool and cr.dtype == torch.int32 and tuple(ins.shape) == tuple(cr.shape) == tuple(pts.shape[:-1])
    return cr.cpu().numpy(), ins.cpu().numpy().astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_crossings_on_the_bits(hip, bunny_small, dev, name):
    tri, nodes, pts, want, sg = _case(name, hip, bunny_small)
    if name == "not_nested":
        assert sg.prune_info()["mode"] == -1                           # pruning is unavailable: the sweep route runs
    else:
        assert sg.prune_info()["mode"] != -1                           # the walk
    for axis in range(6):
        cr, ins = _inside(sg, pts, dev, axis)
        bad = cr != want[0][axis]
        assert not bad.any(), "%s axis %d: %d of %d crossing counts differ, first at point %s" % (
            name, axis, int(bad.sum()), bad.size, pts[np.argmax(bad)])
        assert np.array_equal(ins, want[1][axis])
    assert want[0].max() >= 2 and want[1].any() and not want[1].all()  # the comparison is not of zeros
    assert not want[0][:, ~np.isfinite(pts).all(1)].any()


def test_against_the_occupancy_truth(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    v = IS.voxel_solid()
    kept, truth = v["kept"], v["truth"]
    assert kept[v["kind"] == 0].all() and (kept & (v["kind"] > 0)).sum() >= 200 and (kept & (v["kind"] > 0) & truth).sum() >= 50
    for axis in range(6):
        ins = query.inside(sg, _gpu(pts, dev), axis)
        torch.cuda.synchronize()
        wrong = (ins.cpu().numpy() != truth)[kept]
        assert not wrong.any(), "axis %d: %d of %d points differ from the occupancy grid" % (axis, int(wrong.sum()), int(kept.sum()))


def test_routes_agree(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("bunny", hip, bunny_small)
    swept = hip.scene_create(*A.not_nested(bunny_small))               # the same triangles, created so that pruning is unavailable
    assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
    for axis in range(6):
        a, b = _inside(sg, pts, dev, axis), _inside(swept, pts, dev, axis)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), axis
    sa, sb = query.signed_distance(sg, _gpu(pts, dev), axis=3), query.signed_distance(swept, _gpu(pts, dev), axis=3)
    torch.cuda.synchronize()
    for x, y in zip(sa, sb):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(x.view(np.uint8).reshape(-1), y.view(np.uint8).reshape(-1))


@pytest.mark.parametrize("name", NAMES)
def test_signed_distance_against_closest_point(hip, bunny_small, dev, name):
    tri, nodes, pts, want, sg = _case(name, hip, bunny_small)
    rng = np.random.default_rng(17)
    size = float(np.ptp(tri[:, :9].reshape(-1, 3), axis=0).max())
    p = _gpu(pts, dev)
    for axis, d_max in ((0, None), (5, rng.uniform(0.0, 0.05 * size, pts.shape[0]).astype(np.float32)), (2, np.zeros(pts.shape[0], np.float32))):
        dm = None if d_max is None else _gpu(d_max, dev)
        sd = query.signed_distance(sg, p, dm, axis=axis)
        cp = query.closest_point(sg, p, dm)
        torch.cuda.synchronize()
        assert isinstance(sd, query.SignedDistance) and sd.inside.dtype == torch.bool
        sd, cp = [x.cpu().numpy() for x in sd], [x.cpu().numpy() for x in cp]
        assert np.array_equal(sd[0], cp[0])
        assert np.array_equal(_bits(sd[1]), _bits(cp[1])) and np.array_equal(_bits(sd[3]), _bits(cp[3]))
        assert np.array_equal(_bits(np.abs(sd[2])), _bits(cp[2]))                    # |dist| is closest_point's, on the bits
        assert np.array_equal(np.signbit(sd[2]), sd[4])                              # the sign is `inside`
        assert np.array_equal(sd[4].astype(np.uint8), want[1][axis])                 # ... the restatement's
        miss = sd[0] < 0
        assert np.all(np.isinf(sd[2][miss])) and np.array_equal(sd[2][miss] < 0, sd[4][miss])
        if d_max is not None:                                                        # (without one only a non-finite point misses)
            assert (miss & sd[4]).any() and (miss & ~sd[4]).any()                    # -inf inside, +inf outside


def test_batch_sizes_null_outputs_and_shapes(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    axis = 2
    for n in (1, 63, 64, 65, 4000):
        sel = np.arange(n) * 7 % pts.shape[0]
        cr, ins = _inside(sg, pts[sel], dev, axis)
        assert np.array_equal(cr, want[0][axis][sel]) and np.array_equal(ins, want[1][axis][sel]), n
    n = 257
    P = C.c_void_p
    p = _gpu(pts[:n], dev)
    lib = hip.lib
    # crossings NULL: not touched; inside written
    ins = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    assert lib.ezrt_query_inside_device(sg._h, P(p.data_ptr()), n, axis, P(ins.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ins.cpu().numpy(), want[1][axis][:n])
    # signed distance: every optional output NULL in turn; what is not passed is not touched
    cp = [x.cpu().numpy() for x in query.closest_point(sg, p)]
    for skip in range(5):
        ids = torch.full((n,), -7, dtype=torch.int32, device=dev)
        bufs = [torch.full((n, 3), 7.0, device=dev), torch.full((n,), 7.0, device=dev), torch.full((n, 2), 7.0, device=dev),
                torch.full((n,), 7, dtype=torch.uint8, device=dev)]
        use = [k != skip for k in range(4)]                                       # skip == 4: all passed
        args = [P(b.data_ptr()) if u else None for b, u in zip(bufs, use)]
        assert lib.ezrt_query_signed_distance_device(sg._h, P(p.data_ptr()), None, n, axis, P(ids.data_ptr()), *args, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), cp[0])
        for k, (b, u) in enumerate(zip(bufs, use)):
            if not u:
                assert bool((b == 7).all()), skip
        if use[0]:
            assert np.array_equal(_bits(bufs[0].cpu().numpy()), _bits(cp[1]))
        if use[1]:
            assert np.array_equal(_bits(np.abs(bufs[1].cpu().numpy())), _bits(cp[2]))
            assert np.array_equal(np.signbit(bufs[1].cpu().numpy()).astype(np.uint8), want[1][axis][:n])
        if use[3]:
            assert np.array_equal(bufs[3].cpu().numpy(), want[1][axis][:n])
    lead = pts[:30].reshape(2, 3, 5, 3)
    ins, cr = query.inside(sg, _gpu(lead, dev), axis, crossings=True)
    sd = query.signed_distance(sg, _gpu(lead, dev), axis=axis)
    torch.cuda.synchronize()
    assert tuple(ins.shape) == tuple(cr.shape) == (2, 3, 5) and np.array_equal(cr.cpu().numpy().reshape(-1), want[0][axis][:30])
    assert tuple(sd.tri.shape) == tuple(sd.dist.shape) == tuple(sd.inside.shape) == (2, 3, 5)
    assert tuple(sd.point.shape) == (2, 3, 5, 3) and tuple(sd.bary.shape) == (2, 3, 5, 2)
    assert np.array_equal(sd.inside.cpu().numpy().reshape(-1).astype(np.uint8), want[1][axis][:30])
    only = query.inside(sg, _gpu(lead, dev))                                      # axis 0, no crossings: one tensor
    assert isinstance(only, torch.Tensor) and only.dtype == torch.bool and tuple(only.shape) == (2, 3, 5)
    e = query.inside(sg, torch.empty((0, 3), device=dev), crossings=True)
    assert tuple(e[0].shape) == (0,) == tuple(e[1].shape)
    assert tuple(query.signed_distance(sg, torch.empty((0, 3), device=dev)).point.shape) == (0, 3)


def test_after_a_refit(hip, bunny_small, dev):
    v = IS.voxel_solid()
    tri, nodes, pts, kept, truth = v["tri"], v["nodes"], v["points"], v["kept"], v["truth"]
    moved = tri.copy()
    shift = np.float32([3, -5, 11])
    for k in range(3):                                                 # p1 p2 p3: scaled by 2, shifted by integers (normals keep)
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + shift
    q = pts * np.float32(2) + shift
    sg = hip.scene_create(tri, nodes)
    first = _inside(sg, q, dev, 1)
    refit.refit(sg, moved)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))
    assert sg.prune_info()["mode"] != -1 and fresh.prune_info()["mode"] != -1
    for axis in range(6):
        got, ref = _inside(sg, q, dev, axis), _inside(fresh, q, dev, axis)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), axis
        assert np.array_equal(got[1][kept].astype(bool), truth[kept]), axis              # the new truth: the same grid, moved
    assert not np.array_equal(first[1], _inside(sg, q, dev, 1)[1])


def test_stream_order(hip, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    src = _gpu(pts, dev)
    p = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        p.copy_(src)                                                   # the points are written on `side`, behind the sleep
    a = query.inside(sg, p, 4, crossings=True, stream=side)            # issued from the default stream's context, onto `side`
    b = query.signed_distance(sg, p, axis=4, stream=side.cuda_stream)  # a raw handle
    side.synchronize()
    assert np.array_equal(a[1].cpu().numpy(), want[0][4]) and np.array_equal(b.inside.cpu().numpy().astype(np.uint8), want[1][4])


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
    query.inside(sg, p, 0)
    query.signed_distance(sg, p)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.inside(sg, p, 1, crossings=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(frame.cpu().numpy()), _bits(alone.cpu().numpy()))
    assert np.array_equal(got[1].cpu().numpy(), want[0][1])


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, pts, want, sg = _case("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = 500
    p = _gpu(pts[:n], dev)
    ins = torch.zeros(n, dtype=torch.uint8, device=dev)
    cr = torch.zeros(n, dtype=torch.int32, device=dev)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    host_pts = np.ascontiguousarray(pts[:n])
    host_b = np.zeros(n, np.uint8)
    host_i = np.zeros(n, np.int32)
    host_f = np.zeros((n, 3), np.float32)
    P = C.c_void_p
    f, g = lib.ezrt_query_inside_device, lib.ezrt_query_signed_distance_device
    torch.cuda.synchronize()
    fa = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("n", n), kw.get("axis", 0), kw.get("inside", P(ins.data_ptr())),
                       kw.get("crossings", P(cr.data_ptr())), None]
    ga = lambda **kw: [kw.get("s", sg._h), kw.get("pts", P(p.data_ptr())), kw.get("d_max"), kw.get("n", n), kw.get("axis", 0),
                       kw.get("tri", P(ids.data_ptr())), kw.get("point"), kw.get("dist"), kw.get("bary"), kw.get("inside"), None]
    assert f(*fa()) == 0 and g(*ga()) == 0
    for axis in (6, -1, 100):
        assert f(*fa(axis=axis)) == EZRT_ERR_INVALID and b"axis" in lib.ezrt_last_error()
        assert g(*ga(axis=axis)) == EZRT_ERR_INVALID and b"axis" in lib.ezrt_last_error()
    # host memory is rejected, never read or written
    assert f(*fa(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert f(*fa(inside=P(host_b.ctypes.data))) == EZRT_ERR_INVALID and f(*fa(crossings=P(host_i.ctypes.data))) == EZRT_ERR_INVALID
    assert g(*ga(pts=P(host_pts.ctypes.data))) == EZRT_ERR_INVALID and g(*ga(tri=P(host_i.ctypes.data))) == EZRT_ERR_INVALID
    for name in ("d_max", "point", "dist", "bary"):
        assert g(*ga(**{name: P(host_f.ctypes.data)})) == EZRT_ERR_INVALID, name
    assert g(*ga(inside=P(host_b.ctypes.data))) == EZRT_ERR_INVALID
    assert not host_b.any() and not host_i.any() and not host_f.any()
    # NULL, n < 0, n == 0
    assert f(*fa(inside=None)) == EZRT_ERR_INVALID and f(*fa(s=None)) == EZRT_ERR_INVALID and f(*fa(pts=None)) == EZRT_ERR_INVALID
    assert g(*ga(tri=None)) == EZRT_ERR_INVALID and g(*ga(s=None)) == EZRT_ERR_INVALID and g(*ga(pts=None)) == EZRT_ERR_INVALID
    assert f(*fa(n=-1)) == EZRT_ERR_INVALID and g(*ga(n=-1)) == EZRT_ERR_INVALID
    assert f(*fa(n=0)) == 0 and g(*ga(n=0)) == 0
    # the rejected calls left no HIP error behind: the next call works
    got = _inside(sg, pts[:n], dev, 0)
    assert np.array_equal(got[0], want[0][0][:n])
    # the wrapper
    with pytest.raises(ValueError):
        query.inside(sg, p, 6)
    with pytest.raises(TypeError):
        query.inside(sg, torch.from_numpy(host_pts))
    with pytest.raises(TypeError):
        query.inside(bunny_small.upload(oracle), p)
    with pytest.raises(TypeError):
        query.signed_distance(bunny_small.upload(oracle), p)
    with pytest.raises(ValueError):
        query.signed_distance(sg, p, torch.zeros(10, device=dev))
    with pytest.raises(ValueError):
        query.inside(sg, torch.zeros((4, 6), device=dev))

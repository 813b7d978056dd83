"""Device refit (include/ezrt_refit.h, ezrt_amd/refit.py): a scene whose triangles were moved by ezrt_scene_refit_device answers
exactly as the CPU oracle's scene created from (tri', refit_nodes(tri', nodes)), compared on the bits (NaN equal to NaN):
frames of every integrator, path records, instrumented counters (they walk the binary records' boxes), ezrt_query_hits and the
stream-ordered queries, on Cornell and C2 under rigid, smooth, collapsing, exploding and sliver-making deformations; the pruning
scalars equal those of the HIP library's own create on the refitted arrays; stream order against render calls and queries; the
fallback routes; the 10^6-triangle scene; errors; ProgressiveRenderer.set_geometry.
"""
import ctypes as C

import numpy as np
import pytest

from ezrt_amd import query, refit, scenes, trace
from ezrt_amd import scene as S
from ezrt_amd.progressive import ProgressiveRenderer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID, EZRT_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _same(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


class _Scene:
    """a scene's arrays with the env of the C2 fixture"""

    def __init__(self, name, tri, nodes, hdr, cache):
        self.name, self.tri, self.nodes, self.hdr, self.cache = name, tri, nodes, hdr, cache

    def make(self, lib, tri=None, nodes=None):
        s = lib.scene_create(self.tri if tri is None else tri, self.nodes if nodes is None else nodes)
        s.set_env(self.hdr, self.cache)
        return s


@pytest.fixture(scope="module")
def fixtures(bunny_small):
    c = scenes.cornell_scene()
    return {"cornell": _Scene("cornell", c.tri, c.nodes, bunny_small.hdr, bunny_small.cache),
            "c2": _Scene("c2", bunny_small.tri, bunny_small.nodes, bunny_small.hdr, bunny_small.cache)}


def _rot(tri, th, shift):
    t = tri.copy()
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float64)
    P = t[:, :9].reshape(-1, 3, 3).astype(np.float64)
    t[:, :9] = (P @ R.T + np.asarray(shift)).reshape(-1, 9).astype(np.float32)
    N = t[:, 9:18].reshape(-1, 3, 3).astype(np.float64)
    t[:, 9:18] = (N @ R.T).reshape(-1, 9).astype(np.float32)
    return t


def _leaf_of(nodes, n_tri):
    leaf = np.zeros(n_tri, np.int64)
    for i in range(1, nodes.shape[0]):
        if nodes[i, 3] > 0:
            leaf[int(nodes[i, 4]):int(nodes[i, 4] + nodes[i, 3])] = i
    return leaf


def _deformations(sc):
    tri = sc.tri
    rng = np.random.default_rng(7)
    P = tri[:, :9].reshape(-1, 3, 3).astype(np.float64)
    out = {"rigid": _rot(tri, 0.6, (0.3, -0.2, 0.1))}
    t = tri.copy()                                  # smooth in the position: shared vertices stay shared
    t[:, :9] = (P + 0.08 * np.sin(2.5 * P[..., [1, 2, 0]])).reshape(-1, 9).astype(np.float32)
    out["smooth"] = t
    t = tri.copy()                                  # a subset collapsed to zero area
    Q = t[:, :9].reshape(-1, 3, 3)
    Q[::4, 1] = Q[::4, 0]
    Q[1::9, 2] = Q[1::9, 1]
    out["collapse"] = t
    t = tri.copy()                                  # leaves far apart
    leaf = _leaf_of(sc.nodes, tri.shape[0])
    off = rng.normal(size=(sc.nodes.shape[0], 3)) * 2.0
    t[:, :9] = (P + off[leaf][:, None, :]).reshape(-1, 9).astype(np.float32)
    out["explode"] = t
    t = tri.copy()                                  # slivers: not ordinary (prune_bad > 0, flags set)
    Q = t[:, :9].reshape(-1, 3, 3).astype(np.float64)
    k = np.arange(0, Q.shape[0], 3)
    Q[k, 2] = 0.5 * (Q[k, 0] + Q[k, 1]) + 1e-7 * (Q[k, 2] - Q[k, 0])
    t[:, :9] = Q.reshape(-1, 9).astype(np.float32)
    out["slivers"] = t
    return out


def _rays(tri, n, seed):
    rng = np.random.default_rng(seed)
    P = tri[:, :9].reshape(-1, 3)
    P = P[np.isfinite(P).all(1)]
    lo, hi = P.min(0), P.max(0)
    o = rng.uniform(lo - 1, hi + 1, (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = n // 4
    ax = rng.integers(0, 3, m)
    d[np.arange(m), ax] = 0.0                       # one zero component, origins on vertex planes
    v = P[rng.integers(0, P.shape[0], m)]
    o[np.arange(m), ax] = v[np.arange(m), ax]
    return np.concatenate([o, d], 1).astype(np.float32)


def _gpu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def _compare(sg, so, tri, dev, what, integrators=(3, 50, 51, 52), size=40, spp=2):
    eye, cam = S.camera(20, 10, 5)
    for integ in integrators:
        p = trace.make_params(size, size, eye, cam, integ, 4, spp=spp, frame0=1)
        assert _same(sg.render(p), so.render(p)), "%s: frame of integrator %d" % (what, integ)
    p = trace.make_params(24, 24, eye, cam, 50, 3, frame0=2)
    tg, dg, cg = sg.render_paths(p)
    to, do, co = so.render_paths(p)
    assert np.array_equal(tg, to) and _same(dg, do) and _same(cg, co), "%s: render_paths" % what
    sg.set_instrumentation(1)
    so.set_instrumentation(1)
    sg.counters_reset()
    so.counters_reset()
    p = trace.make_params(24, 24, eye, cam, 50, 4, spp=2)
    assert _same(sg.render(p), so.render(p)), what
    assert sg.counters() == so.counters(), "%s: instrumented counters" % what
    sg.set_instrumentation(0)
    so.set_instrumentation(0)
    rays = _rays(tri, 20000, 3)
    to, do = so.query_hits(rays)
    tg, dg = sg.query_hits(rays)
    assert np.array_equal(tg, to) and _same(dg, do), "%s: query_hits" % what
    tri_d, t_d = query.closest(sg, _gpu(rays, dev))
    torch.cuda.synchronize()
    assert np.array_equal(tri_d.cpu().numpy(), to) and _same(t_d.cpu().numpy(), do), "%s: closest" % what
    t_max = np.random.default_rng(5).uniform(0, 6, rays.shape[0]).astype(np.float32)
    hit = (to >= 0) & (do < t_max)
    tri_d, t_d = query.closest(sg, _gpu(rays, dev), _gpu(t_max, dev))
    occ = query.occluded(sg, _gpu(rays, dev), _gpu(t_max, dev))
    occ0 = query.occluded(sg, _gpu(rays, dev))
    torch.cuda.synchronize()
    assert np.array_equal(tri_d.cpu().numpy(), np.where(hit, to, -1)), "%s: closest t_max" % what
    assert _same(t_d.cpu().numpy(), np.where(hit, do, np.float32(114514.0))), what
    assert np.array_equal(occ.cpu().numpy(), hit) and np.array_equal(occ0.cpu().numpy(), to >= 0), "%s: occluded" % what


def test_identity_refit_changes_nothing(hip, fixtures, dev):
    sc = fixtures["c2"]
    ref, sg = sc.make(hip), sc.make(hip)
    refit.refit(sg, _gpu(sc.tri, dev))
    eye, cam = S.camera(0, 0, 4)
    for integ in (50, 51):
        p = trace.make_params(48, 48, eye, cam, integ, 4, spp=3)
        assert _same(sg.render(p), ref.render(p)), integ
    p = trace.make_params(24, 24, eye, cam, 51, 3)
    a, b = sg.render_paths(p), ref.render_paths(p)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])
    for s in (sg, ref):
        s.set_instrumentation(1)
        s.counters_reset()
        s.render(trace.make_params(24, 24, eye, cam, 50, 4, spp=2))
    assert sg.counters() == ref.counters()
    assert sg.prune_info() == ref.prune_info()


@pytest.mark.parametrize("name", ["cornell", "c2"])
def test_deformed_scenes_equal_the_oracle(hip, oracle, fixtures, dev, name):
    sc = fixtures[name]
    base = sc.make(hip)
    before = base.prune_info()
    seen_bad = False
    for what, tri2 in _deformations(sc).items():
        nodes2 = refit.refit_nodes(tri2, sc.nodes)
        sg = sc.make(hip)
        refit.refit(sg, _gpu(tri2, dev))
        so = sc.make(oracle, tri2, nodes2)
        _compare(sg, so, tri2, dev, "%s/%s" % (name, what))
        info, fresh = sg.prune_info(), sc.make(hip, tri2, nodes2).prune_info()
        for k in ("G", "Z", "M", "unprunable_triangles", "margin_a"):
            assert info[k] == fresh[k] or (np.isnan(info[k]) and np.isnan(fresh[k])), (name, what, k, info[k], fresh[k])
        for k in ("mode", "retreed", "records4"):
            assert info[k] == before[k], (name, what, k)
        seen_bad |= what == "slivers" and info["unprunable_triangles"] > 0
    assert seen_bad or name == "cornell"


def test_refit_back_restores_the_original_frames(hip, fixtures, dev):
    sc = fixtures["c2"]
    sg = sc.make(hip)
    eye, cam = S.camera(0, 0, 4)
    p = trace.make_params(40, 40, eye, cam, 51, 4, spp=2)
    f0 = sg.render(p)
    info0 = sg.prune_info()
    refit.refit(sg, _deformations(sc)["explode"])          # (a numpy array: copied to the device first)
    assert not _same(sg.render(p), f0)
    refit.refit(sg, sc.tri)
    assert _same(sg.render(p), f0)
    assert sg.prune_info() == info0


def test_stream_order_render_refit_render(hip, oracle, fixtures, dev):
    sc = fixtures["c2"]
    sg = sc.make(hip)
    sg.set_option("pipeline_calls", 1)
    tri2 = _rot(sc.tri, -0.8, (0.0, 0.2, -0.3))
    so_old, so_new = sc.make(oracle), sc.make(oracle, tri2, refit.refit_nodes(tri2, sc.nodes))
    eye, cam = S.camera(0, 0, 4)
    p = trace.make_params(64, 64, eye, cam, 50, 4, spp=8)
    fa, fb = hip.frame(64, 64), hip.frame(64, 64)
    t2 = _gpu(tri2, dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sg.render_device(p, fa.ptr, s.cuda_stream)
    refit.refit(sg, t2, stream=s)
    sg.render_device(p, fb.ptr, s.cuda_stream)
    s.synchronize()
    assert _same(fa.read(), so_old.render(p)) and _same(fb.read(), so_new.render(p))


def test_device_query_before_the_refit_answers_for_the_old_geometry(hip, oracle, fixtures, dev):
    sc = fixtures["c2"]
    sg = sc.make(hip)
    rays = _rays(sc.tri, 200000, 11)
    to, do = sc.make(oracle).query_hits(rays)
    r = _gpu(rays, dev)
    tri2 = _gpu(_rot(sc.tri, 1.1, (0.5, 0.0, 0.0)), dev)
    qs, rs = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    tri_d, t_d = query.closest(sg, r, stream=qs)
    refit.refit(sg, tri2, stream=rs)
    torch.cuda.synchronize()
    assert np.array_equal(tri_d.cpu().numpy(), to) and _same(t_d.cpu().numpy(), do)


def _not_nested(sc):
    nodes = sc.nodes.copy()
    for i in range(2, nodes.shape[0]):                      # (the root's own box is never tested)
        if nodes[i, 3] <= 0:
            c = int(nodes[i, 0])
            nodes[c, 6:9] -= 1.0                            # a child box larger than its parent's: the binary kernel's route
            break
    return nodes


@pytest.mark.parametrize("route", ["binary", "prune0", "megakernel"])
def test_fallback_routes_match_the_oracle(hip, oracle, fixtures, dev, route):
    sc = fixtures["c2"]
    nodes = _not_nested(sc) if route == "binary" else sc.nodes
    sg = sc.make(hip, nodes=nodes)
    if route == "binary":
        assert sg.prune_info()["records4"] == 0
    elif route == "prune0":
        sg.set_option("prune", 0)
    else:
        sg.set_option("megakernel", 1)
    tri2 = _deformations(sc)["smooth"]
    refit.refit(sg, _gpu(tri2, dev))
    so = sc.make(oracle, tri2, refit.refit_nodes(tri2, nodes))
    eye, cam = S.camera(0, 0, 4)
    for integ in (50, 51):
        p = trace.make_params(40, 40, eye, cam, integ, 4, spp=2)
        assert _same(sg.render(p), so.render(p)), (route, integ)
    rays = _rays(tri2, 20000, 13)
    to, do = so.query_hits(rays)
    tri_d, t_d = query.closest(sg, _gpu(rays, dev))
    torch.cuda.synchronize()
    assert np.array_equal(tri_d.cpu().numpy(), to) and _same(t_d.cpu().numpy(), do)


def test_million_triangle_scene(hip, oracle, dev):
    bs = scenes.mega_scene()
    sg = bs.upload(hip)
    tri2 = _rot(bs.tri, 0.35, (0.2, 0.1, -0.4))
    refit.refit(sg, _gpu(tri2, dev))
    nodes2 = refit.refit_nodes(tri2, bs.nodes)
    so = oracle.scene_create(tri2, nodes2)
    rng = np.random.default_rng(17)
    n = 60000
    o = rng.uniform([-7, -1.3, -6], [7, 3, 6], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    to, do = so.query_hits(rays)
    assert (to >= 0).mean() > 0.3
    tri_d, t_d = query.closest(sg, _gpu(rays, dev))
    t_max = rng.uniform(0, 12, n).astype(np.float32)
    occ = query.occluded(sg, _gpu(rays, dev), _gpu(t_max, dev))
    torch.cuda.synchronize()
    assert np.array_equal(tri_d.cpu().numpy(), to) and _same(t_d.cpu().numpy(), do)
    assert np.array_equal(occ.cpu().numpy(), (to >= 0) & (do < t_max))
    fresh = hip.scene_create(tri2, nodes2).prune_info()
    info = sg.prune_info()
    for k in ("G", "Z", "M", "unprunable_triangles", "margin_a"):
        assert info[k] == fresh[k], k


def _dag_scene():
    T = np.zeros((4, 36), np.float32)
    for k in range(4):
        T[k, :9] = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32) + np.float32(k) * np.array([0, 0, -1] * 3, np.float32)
    T[:, 9:18] = np.tile([0, 0, 1], 3)
    T[:, 18:36] = S.Material.disney().to18()
    nodes = np.zeros((6, 12), np.float32)
    nodes[1, :2] = [2, 3]
    nodes[2, :2] = [4, 5]
    nodes[3, :2] = [4, 5]                                   # nodes 4 and 5 have two parents
    nodes[4, 3:5] = [2, 0]
    nodes[5, 3:5] = [2, 2]
    return T, refit.refit_nodes(T, nodes)


def test_errors_leave_the_scene_unchanged(hip, fixtures, dev):
    sc = fixtures["c2"]
    sg = sc.make(hip)
    eye, cam = S.camera(0, 0, 4)
    p = trace.make_params(32, 32, eye, cam, 50, 3, spp=2)
    f0 = sg.render(p)
    lib = hip.lib
    t2 = _gpu(_rot(sc.tri, 0.5, (0, 0, 0)), dev)
    n = sc.tri.shape[0]
    host = np.ascontiguousarray(sc.tri, np.float32)
    assert lib.ezrt_scene_refit_device(sg._h, C.c_void_p(t2.data_ptr()), n - 1, None) == EZRT_ERR_INVALID
    assert lib.ezrt_scene_refit_device(sg._h, C.c_void_p(host.ctypes.data), n, None) == EZRT_ERR_INVALID
    assert lib.ezrt_scene_refit_device(sg._h, None, n, None) == EZRT_ERR_INVALID
    assert lib.ezrt_scene_refit_device(None, C.c_void_p(t2.data_ptr()), n, None) == EZRT_ERR_INVALID
    with pytest.raises(trace.TraceError):
        refit.refit(sg, t2[:-1])
    assert _same(sg.render(p), f0)
    T, nodes = _dag_scene()
    sd = hip.scene_create(T, nodes)
    pd = trace.make_params(16, 16, S.camera(0, 0, 4)[0], S.camera(0, 0, 4)[1], 3, 2, spp=1)
    fd = sd.render(pd)
    assert lib.ezrt_scene_refit_device(sd._h, C.c_void_p(_gpu(T, dev).data_ptr()), 4, None) == EZRT_ERR_UNSUPPORTED
    assert _same(sd.render(pd), fd)


def test_progressive_set_geometry(hip, fixtures, dev):
    sc = fixtures["c2"]
    tri2 = _deformations(sc)["smooth"]
    pr = ProgressiveRenderer(sc.make(hip), 48, 48, integrator=51, max_bounce=3)
    pr.step(2)
    pr.set_geometry(_gpu(tri2, dev))
    assert pr.frameCounter == 0
    pr.step(3)
    fresh = ProgressiveRenderer(sc.make(hip, tri2, refit.refit_nodes(tri2, sc.nodes)), 48, 48, integrator=51, max_bounce=3)
    fresh.step(3)
    assert _same(pr.accum, fresh.accum)

"""The ray queries on every tree shape a caller can pass (tests/tree_shapes.py: ray_queries, ray_expected): query.closest,
query.occluded, query.all_hits, query.surface, query.surface_at and path.radiance on a median tree with leaves of one triangle, leaves
of 128, a chain of depth 63, a root that is a leaf, a root with two leaves, triangles that no leaf holds, loose boxes, a leaf box
that misses a vertex and the device LBVH builder's trees -- every shape that walks with the re-tree off (the records are a collapse of
the caller's own inner nodes) and on.

The ray contract is hitBVH on the caller's arrays, so unlike the point queries the answers depend on the leaves: a triangle below no
leaf is never seen, and of two triangles at one distance the one whose leaf the reference reaches first wins.  Every answer is
compared on the bits (NaN equal to NaN) with the CPU oracle's ezrt_query_hits and the restated all-hits lists on the same arrays;
nothing of the product is in the expectation.  First the route (prune_info, stats), then the queries, without t_max and with the
nearest hit's own t, one ulp either side of it, the second hit's t, +inf, NaN, 0 and a negative value.  tests/test_tree_shapes.py
shows on the CPU that the rays tie across leaves, leave 48 entries pending on the chain and are decided by the missing leaves."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit, scenes, trace
from ezrt_amd import scene as S

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_shapes as T  # noqa: E402
from test_gpu_tree_shapes import _Env  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WALKS = [n for n in T.HOST_SHAPES + T.LBVH_SHAPES if n not in ("root_leaf_1", "root_leaf_8", "leaf_misses")]
CASES = [(n, r) for n in T.HOST_SHAPES + T.LBVH_SHAPES for r in ((0, 1) if n in WALKS else (None,))]
PRUNE_CASES = [(n, r) for n, r in CASES if n in WALKS or n == "leaf_misses"]
STACK_CAP_CASES = [(n, r) for n, r in CASES if n in ("chain", "median1")]
RADIANCE_CASES = [(n, r) for n, r in CASES if n in ("chain", "median1", "leaf128", "root_leaf_8", "two_leaves") and (n == "chain" or r != 0)]
REFIT_CASES = [("median1", 0), ("median1", 1), ("chain", 0)]
# (tree_shapes.CAMERAS: the camera that looks at the shape -- at least a fifth of the 40 x 24 paths hit it and some reach the last bounce)
CAMERAS, _look_at = T.CAMERAS, T._look_at
W, H, BOUNCES, FRAMES = 40, 24, 3, (0, 7)
STEP = np.float32([0.25, -0.5, 0.25])


def _ids(cases):
    return ["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _scene(hip, name, retree, arrays=None):
    """a fresh device scene of a case; EZRT_RETREE is read at scene creation"""
    tri, nodes = arrays or T.shape(name)[:2]
    if retree is None:
        return hip.scene_create(tri, nodes)
    with _Env(EZRT_RETREE=retree):
        return hip.scene_create(tri, nodes)


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.array(x, dtype, order="C")).to(dev)   # (a copy: the shared arrays are read-only)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tags():
    return [(None, "")] + [(k, "[%s]" % k) for k in T.T_MAX]


def _route(sg, name, retree):
    """The route of the scene, printed and asserted as tests/test_gpu_tree_shapes.py does; returns whether query.occluded runs the
    bounded any-hit kernel.  Nothing reports that choice: it is query_device_body's condition (ezrt_launch.hip) spelled out --
    `occluded && use_wide4(s) && prune_mode(s) == 2`, where use_wide4 is "the scene has 4-wide records" (records4 > 0; the knob wide4 and
    the instrumentation are at their defaults here) and prune_info's mode is prune_mode(s), or -1 where the scene does not prune."""
    expect = T.shape(name)[2]
    info = sg.prune_info()
    route = dict(mode=info["mode"], records4=info["records4"], retreed=info["retreed"])
    any_hit = route["records4"] > 0 and route["mode"] == 2
    print("route %s%s: %s, depth %d, occluded by the any-hit kernel: %s" % (name, "" if retree is None else " EZRT_RETREE=%d" % retree, route,
                                                                            sg.stats()["depth"], any_hit))
    if expect["walk"]:
        assert route["mode"] != -1 and route["records4"] > 0, route
    else:
        assert route["mode"] == -1 or route["records4"] == 0, route
    if "mode" in expect:
        assert route["mode"] == expect["mode"] and route["records4"] > 0, route   # (leaf_misses: records, but no pruning)
    if expect.get("records4") is not None:
        assert route["records4"] == expect["records4"], route
    want = retree if retree is not None else expect["retree"]
    if want is not None:
        assert route["retreed"] == float(want), route
    if "depth" in expect:
        assert sg.stats()["depth"] == expect["depth"]
    assert any_hit == expect["walk"], route                             # mode 2 is the default of every scene that prunes
    return any_hit


def closest_answers(sg, r, X, dev):
    """query.closest and query.occluded without t_max and with every derived t_max; occluded == (closest.tri >= 0) on the device"""
    G = {}
    for key, tag in _tags():
        tm = None if key is None else _gpu(X["_t_max." + key], dev)
        tri, t = query.closest(sg, r, tm)
        occ = query.occluded(sg, r, tm)
        assert occ.dtype == torch.bool and torch.equal(occ, tri >= 0), "occluded != (closest.tri >= 0) %s" % tag
        G["closest%s.tri" % tag], G["closest%s.t" % tag], G["occluded%s" % tag] = tri, t, occ
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in G.items()}


def _closest_names(X):
    return {k: v for k, v in X.items() if k.startswith(("closest", "occluded"))}


def _check(got, want, what):
    bad = T.differing(got, want)
    assert not bad, "%s: %s" % (what, ", ".join(bad))


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_closest_and_occluded_on_the_bits(hip, oracle, dev, name, retree):
    X = T.ray_expected(oracle, name)
    sg = _scene(hip, name, retree)
    _route(sg, name, retree)
    _check(closest_answers(sg, _gpu(T.ray_queries(name)["rays"], dev), X, dev), _closest_names(X), name)


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_all_hits_on_the_bits(hip, oracle, dev, name, retree):
    X = T.ray_expected(oracle, name)
    sg = _scene(hip, name, retree)
    r = _gpu(T.ray_queries(name)["rays"], dev)
    n = r.shape[0]
    G, P = {}, C.c_void_p
    for key, tag in _tags():
        tm = None if key is None else _gpu(X["_t_max." + key], dev)
        tri, t = query.closest(sg, r, tm)
        occ = query.occluded(sg, r, tm)
        for K in T.ALL_HITS_K:
            at, ad, ac = query.all_hits(sg, r, K, tm)
            assert torch.equal(at[:, 0], tri) and _bits_equal(ad[:, 0], t) and torch.equal(ac > 0, occ), "K=%d %s" % (K, tag)
            G["all%d%s.tri" % (K, tag)], G["all%d%s.t" % (K, tag)], G["all%d%s.count" % (K, tag)] = at, ad, ac
            only = torch.full((n, K), -7, dtype=torch.int32, device=dev)   # without t_hit and n_hits (the C entry point): the same ids
            assert hip.lib.ezrt_query_all_hits_device(sg._h, P(r.data_ptr()), None if tm is None else P(tm.data_ptr()), n, K,
                                                      P(only.data_ptr()), None, None, None) == 0
            assert torch.equal(only, at), "K=%d %s, no t_hit" % (K, tag)
    torch.cuda.synchronize()
    _check({k: v.cpu().numpy() for k, v in G.items()}, {k: v for k, v in X.items() if k.startswith("all")}, name)


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_surface_and_surface_at_on_the_bits(hip, oracle, dev, name, retree):
    tri36 = T.shape(name)[0]
    rays = T.ray_queries(name)["rays"]
    X = T.ray_expected(oracle, name)
    sg = _scene(hip, name, retree)
    r = _gpu(rays, dev)
    G = {}
    tri, t = query.closest(sg, r)
    at, ad, _ = query.all_hits(sg, r, 5)
    for form in T.SURFACE_FORMS:
        s = query.surface(sg, r, integrator=form)
        assert torch.equal(s.tri, tri) and _bits_equal(s.t, t), form
        G["surface%d.point" % form], G["surface%d.normal" % form], G["surface%d.inside" % form] = s.point, s.normal, s.inside
        p5, n5, i5 = query.surface_at(sg, r, at, ad, integrator=form)   # the all-hits rows passed straight in: slot 0 is the surface
        assert _bits_equal(p5[:, 0], s.point) and _bits_equal(n5[:, 0], s.normal) and torch.equal(i5[:, 0], s.inside), form
        p1, n1, i1 = query.surface_at(sg, r, tri, t, integrator=form)
        assert _bits_equal(p1, s.point) and _bits_equal(n1, s.normal) and torch.equal(i1, s.inside), form
    torch.cuda.synchronize()
    G = {k: v.cpu().numpy() for k, v in G.items()}
    assert np.array_equal(tri.cpu().numpy(), X["closest.tri"]) and T.RS.same_bits(t.cpu().numpy(), X["closest.t"])
    _check(G, {k: v for k, v in X.items() if k.startswith("surface")}, name)
    for key in T.T_MAX:                                                # with a t_max: {tri, t} is closest's, the attributes their restatement
        s = query.surface(sg, r, _gpu(X["_t_max." + key], dev))
        torch.cuda.synchronize()
        st, sd = s.tri.cpu().numpy(), s.t.cpu().numpy()
        assert np.array_equal(st, X["closest[%s].tri" % key]) and T.RS.same_bits(sd, X["closest[%s].t" % key]), key
        wp, wn, wi = T.RS.restate(tri36, rays, st, sd, True)
        assert T.RS.same_bits(s.point.cpu().numpy(), wp) and T.RS.same_bits(s.normal.cpu().numpy(), wn), key
        assert np.array_equal(s.inside.cpu().numpy(), wi), key


@pytest.mark.parametrize("name,retree", PRUNE_CASES, ids=_ids(PRUNE_CASES))
def test_every_pruning_mode(hip, oracle, dev, name, retree):
    """closest and occluded under every mode the scene accepts, a fresh scene each: 0 the unpruned walk in slot order, 1 pruned, 2
    nearest first (the only mode in which occluded runs the any-hit kernel).  leaf_misses does not prune whatever is asked."""
    X = T.ray_expected(oracle, name)
    r = _gpu(T.ray_queries(name)["rays"], dev)
    for mode in (0, 1, 2):
        sg = _scene(hip, name, retree)
        assert sg.prune_info()["mode"] == (-1 if name == "leaf_misses" else 2)
        sg.set_option("prune", mode)
        assert sg.prune_info()["mode"] == (-1 if name == "leaf_misses" else mode)
        _check(closest_answers(sg, r, X, dev), _closest_names(X), "%s prune=%d" % (name, mode))


@pytest.mark.parametrize("name,retree", STACK_CAP_CASES, ids=_ids(STACK_CAP_CASES))
def test_a_tiny_stack_hands_the_rays_to_the_redo_launch(hip, oracle, dev, name, retree):
    """debug_stack_cap: a ring of four stack rows and a spill area of 0 (cap 1) or 4 (cap 2) entries for the nearest-first walk of both
    kernels of the device-query route; a ray that needs more goes to the device-driven redo launch.  The answers do not change."""
    X = T.ray_expected(oracle, name)
    r = _gpu(T.ray_queries(name)["rays"], dev)
    for cap in (1, 2):
        sg = _scene(hip, name, retree)
        sg.set_option("debug_stack_cap", cap)
        assert sg.prune_info()["mode"] == 2
        _check(closest_answers(sg, r, X, dev), _closest_names(X), "%s debug_stack_cap=%d" % (name, cap))


_audits = {}


def _audit(oracle, name, env, integ, frame):
    """the oracle's path audit of one frame on the shape's arrays, computed once per shape (the re-tree settings share it)"""
    if (name, integ, frame) not in _audits:
        tri, nodes = T.shape(name)[:2]
        so = oracle.scene_create(tri, nodes)
        so.set_env(*env)
        ids, _, col = so.render_paths(trace.make_params(W, H, *_look_at(*CAMERAS[name]), integ, BOUNCES, frame0=frame))
        _audits[(name, integ, frame)] = (ids.reshape(W * H, -1), col.reshape(W * H, 3))
    return _audits[(name, integ, frame)]


@pytest.mark.parametrize("name,retree", RADIANCE_CASES, ids=_ids(RADIANCE_CASES))
def test_radiance_equals_the_path_audit(hip, oracle, dev, name, retree):
    from ezrt_amd import path
    hdr = scenes.synthetic_hdr(64, 32)
    env = (hdr, S.calculateHdrCache(hdr))
    sg = _scene(hip, name, retree)
    sg.set_env(*env)
    for integ in (50, 51):
        for frame in FRAMES:
            ids, want = _audit(oracle, name, env, integ, frame)
            assert (ids[:, 0] >= 0).mean() >= 0.2, "too few paths hit the shape"
            assert (ids[:, -1] >= -1).any(), "no path reaches the last bounce"
            p = trace.make_params(W, H, *_look_at(*CAMERAS[name]), integ, BOUNCES, frame0=frame)
            ys, xs = np.mgrid[0:H, 0:W]
            xyf = np.stack([xs.ravel(), ys.ravel(), np.full(W * H, frame)], 1).astype(np.uint32)
            dx = torch.from_numpy(xyf.view(np.int32)).to(dev).view(torch.uint32)
            got = path.radiance(sg, path.camera_rays(sg, p, dx), dx, integrator=integ, max_bounce=BOUNCES)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(1)
            assert not bad.any(), "integrator %d, frame %d: %d of %d pixels differ; first %d: %r != %r" % (
                integ, frame, int(bad.sum()), bad.size, int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])
            assert float(np.nanmax(want)) > 0.1 and np.isnan(want).any(1).mean() < 0.01


def _refit_answers(sg, r, dev):
    G = {}
    G["closest.tri"], G["closest.t"] = query.closest(sg, r)
    G["occluded"] = query.occluded(sg, r)
    G["all5.tri"], G["all5.t"], G["all5.count"] = query.all_hits(sg, r, 5)
    s = query.surface(sg, r)
    G["surface50.point"], G["surface50.normal"], G["surface50.inside"] = s.point, s.normal, s.inside
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in G.items()}


@pytest.mark.parametrize("name,retree", REFIT_CASES, ids=_ids(REFIT_CASES))
def test_a_refit_by_an_exact_step(hip, oracle, dev, name, retree):
    """Every triangle moves by (0.25, -0.5, 0.25) -- exact on the base set's multiples of 1/4 -- and so do the rays: the ids are the
    unmoved scene's, the distances the oracle's on the moved arrays with refit_nodes; refitted back, the first call's bits again."""
    tri, nodes = T.shape(name)[:2]
    rays = T.ray_queries(name)["rays"]
    X = T.ray_expected(oracle, name)
    moved, rays2 = np.array(tri), np.array(rays)
    for v in range(3):
        moved[:, 3 * v:3 * v + 3] += STEP
    with np.errstate(invalid="ignore"):
        rays2[:, :3] += STEP
    assert np.array_equal(moved[:, :9] - np.tile(STEP, 3), tri[:, :9])
    nodes2 = refit.refit_nodes(moved, nodes)
    to, do = oracle.scene_create(moved, nodes2).query_hits(rays2)
    lists = T.AE.expected_all_hits(oracle, moved, nodes2, rays2, None)
    M = {"closest.tri": to, "closest.t": do, "occluded": to >= 0}
    M["all5.tri"], M["all5.t"], M["all5.count"] = T.AE.rows(lists, 5)
    M["surface50.point"], M["surface50.normal"], M["surface50.inside"] = T.RS.restate(moved, rays2, to, do, True)
    assert np.array_equal(to, X["closest.tri"]) and np.array_equal(M["all5.tri"], X["all5.tri"])   # the ids of the unmoved scene
    assert not T.RS.same_bits(do, X["closest.t"])                      # (the distances are not: other roundings)
    sg = _scene(hip, name, retree)
    route = sg.prune_info()
    r, r2 = _gpu(rays, dev), _gpu(rays2, dev)
    first = _refit_answers(sg, r, dev)
    _check(first, {k: X[k] for k in first}, name)
    refit.refit(sg, moved)
    assert sg.prune_info()["mode"] == route["mode"] and sg.prune_info()["records4"] == route["records4"]
    _check(_refit_answers(sg, r2, dev), M, "%s, moved" % name)
    refit.refit(sg, np.array(tri))
    _check(_refit_answers(sg, r, dev), first, "%s, moved back" % name)

"""Stream-ordered surface queries (include/ezrt_surface.h, ezrt_amd/query.py: surface): the closest hit of every ray with its hit
point, shading normal and side, compared on the bits (NaN equal to NaN):

* against the executed chapter-5 shader's own hitBVH records (tests/golden/fsh_golden.npz: C2, exact ties, C3, C5), no oracle in
  between; 51 and 52 give the same bits as 50;
* {tri, t} against query.closest on broad and adversarial ray mixes, for every kind of t_max;
* the attributes against the numpy restatement of tests/test_surface_restatement.py (itself pinned to the goldens and, where
  oracle/_ref was built, to the executed chapter-3/4 shaders) for the three forms, and directly against the chapter-3/4 shaders;
* every traversal route giving the same outputs; refit; the eight combinations of optional outputs; streams, scene state, errors;
  2^22 rays on the 10^6-triangle scene.
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
import test_surface_restatement as RS  # noqa: E402  (restate, the golden scenes)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
MISS_T = np.float32(114514.0)
_same = RS.same_bits


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _gpu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def _surface(sg, rays, dev, t_max=None, integrator=50):
    r = query.surface(sg, _gpu(rays, dev), None if t_max is None else _gpu(t_max, dev), integrator)
    torch.cuda.synchronize()
    assert r.tri.dtype == torch.int32 and r.t.dtype == torch.float32 and r.inside.dtype == torch.bool
    assert r.point.dtype == torch.float32 and r.normal.dtype == torch.float32
    return tuple(x.cpu().numpy() for x in r)


def _closest(sg, rays, dev, t_max=None):
    tri, t = query.closest(sg, _gpu(rays, dev), None if t_max is None else _gpu(t_max, dev))
    torch.cuda.synchronize()
    return tri.cpu().numpy(), t.cpu().numpy()


def _same_out(a, b):
    return all(np.array_equal(x, y) if x.dtype != np.float32 else _same(x, y) for x, y in zip(a, b))


def _check_restated(tri36, rays, out, p5, what=""):
    """the attributes of `out` = restate(its own {tri, t}); misses are zeros"""
    tri, t, point, normal, inside = out
    wp, wn, wi = RS.restate(tri36, rays, tri, t, p5)
    assert _same(point, wp), what
    assert _same(normal, wn), what
    assert np.array_equal(inside, wi), what
    miss = tri < 0
    assert not point[miss].any() and not normal[miss].any() and not inside[miss].any()


# ---- the executed reference shader's records: the core test

@pytest.mark.parametrize("key", RS.HITBVH_SETS)
def test_surface_equals_the_executed_shaders_hit_records(hip, dev, key):
    tri36, nodes = RS.golden_scene(key)
    rays, want = RS.GOLD[key + "_rays"], RS.GOLD[key]
    sg = hip.scene_create(tri36, nodes)
    out = _surface(sg, rays, dev, integrator=50)
    tri, t, point, normal, inside = out
    hit = want[:, 0] > 0
    assert np.array_equal(tri >= 0, hit)
    assert _same(t[hit], want[hit, 2])
    assert np.array_equal(inside[hit], want[hit, 1] > 0)
    assert _same(point[hit], want[hit, 3:6])
    assert _same(normal[hit], want[hit, 6:9])
    assert _same(tri36[tri[hit], 21:24], want[hit, 9:12])
    assert not point[~hit].any() and not normal[~hit].any() and not inside[~hit].any()
    assert np.array_equal(tri[~hit], np.full((~hit).sum(), -1)) and (t[~hit] == MISS_T).all()
    for integ in (51, 52):
        assert _same_out(_surface(sg, rays, dev, integrator=integ), out), integ


# ---- {tri, t} = query.closest, every t_max rule

def _camera_rays(n, rng, eye=(0.0, 0.0, 4.0)):
    o = np.tile(np.asarray(eye, np.float32), (n, 1))
    d = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), -1.5 * np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def _broad_rays(tri, rng, n=200000):
    """random, camera, axis-parallel / one-zero-component (origins on box planes), unnormalised, and not-tame rays"""
    P = tri[:, :9].reshape(-1, 3, 3)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    parts = []
    k = n // 4
    o = rng.uniform(lo - 1, hi + 1, (k, 3))
    d = rng.uniform(lo, hi, (k, 3)) - o
    parts.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    parts.append(_camera_rays(k, rng))
    m = n // 4
    o = rng.uniform(lo - 1, hi + 1, (m, 3))
    d = rng.uniform(lo, hi, (m, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = rng.integers(0, 3, m)
    d[np.arange(m), ax] = rng.choice([0.0, -0.0], m)
    two = rng.random(m) < 0.3
    d[two, (ax[two] + 1) % 3] = 0.0
    onp = rng.random(m) < 0.3
    v = P[rng.integers(0, P.shape[0], m), rng.integers(0, 3, m)]
    o[onp, ax[onp]] = v[onp, ax[onp]]
    parts.append(np.concatenate([o, d], 1))
    u = n // 8
    o = rng.uniform(lo - 1, hi + 1, (u, 3))
    d = (rng.uniform(lo, hi, (u, 3)) - o) * 10.0 ** rng.uniform(-3, 3, (u, 1))
    parts.append(np.concatenate([o, d], 1))
    w = n - 2 * k - m - u
    o = rng.uniform(lo - 1, hi + 1, (w, 3))
    d = rng.normal(size=(w, 3))
    sel = rng.integers(0, 4, w)
    j = rng.integers(0, 3, w)
    r = np.arange(w)
    d[r[sel == 0], j[sel == 0]] = np.inf
    d[r[sel == 1], j[sel == 1]] = -np.inf
    o[r[sel == 2], j[sel == 2]] = rng.choice([-np.inf, np.inf], int((sel == 2).sum()))
    o[r[sel == 3], j[sel == 3]] = rng.choice([-3.2e38, 3.3e38], int((sel == 3).sum()))
    parts.append(np.concatenate([o, d], 1))
    rays = np.concatenate(parts).astype(np.float32)
    return rays[rng.permutation(rays.shape[0])]


def _nasty_scene(rng):
    """slivers, near-degenerate and grazing geometry, a tiled plane, far flat triangles, duplicates"""
    parts = []
    c = rng.uniform(-2, 2, (1500, 1, 3))
    parts.append(c + rng.uniform(-0.15, 0.15, (1500, 3, 3)))
    p1 = rng.uniform(-2, 2, (600, 3))
    e = rng.normal(size=(600, 3)); e /= np.linalg.norm(e, axis=1, keepdims=True)
    o = np.cross(e, rng.normal(size=(600, 3))); o /= np.linalg.norm(o, axis=1, keepdims=True)
    w = 10.0 ** rng.uniform(-5, -2, (600, 1))
    parts.append(np.stack([p1, p1 + 2.0 * e, p1 + rng.uniform(0.2, 1.8, (600, 1)) * e + w * o], 1))
    g = np.linspace(-2, 2, 17)
    for i in range(16):
        for j in range(16):
            a, b = np.array([g[i], g[j], 0.25]), np.array([g[i + 1], g[j + 1], 0.25])
            parts.append(np.array([[[a[0], a[1], .25], [b[0], a[1], .25], [b[0], b[1], .25]],
                                   [[a[0], a[1], .25], [b[0], b[1], .25], [a[0], b[1], .25]]]))
    parts.append(rng.uniform(-1, 1, (100, 1, 3)) + np.array([40.0, -35.0, 30.0]) +
                 rng.uniform(-0.5, 0.5, (100, 3, 3)) * np.array([1.0, 1e-3, 1.0]))
    P = np.concatenate(parts).astype(np.float32)
    P = np.concatenate([P, P[:100]])
    n = P.shape[0]
    T = np.zeros((n, 36), np.float32)
    T[:, :9] = P.reshape(n, 9)
    # vertex normals that vary across each triangle (the interpolation matters), and a spread of base colours
    T[:, 9:18] = rng.normal(size=(n, 9)).astype(np.float32)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    T[:, 21:24] = rng.uniform(0, 1, (n, 3))
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(T))
    hs.buildBVHwithSAH(4)
    tri, nodes = hs.encode()
    rays = []
    o = rng.uniform(-3, 3, (20000, 3)); d = rng.uniform(-2, 2, (20000, 3)) - o
    rays.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    k = rng.integers(0, n, 20000)
    bc = rng.dirichlet([1, 1, 1], 20000)
    pt = (P[k] * bc[:, :, None]).sum(1)
    d = rng.normal(size=(20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays.append(np.concatenate([pt - d * rng.uniform(0.5, 4.0, (20000, 1)), d], 1))
    o = rng.uniform(-1, 1, (20000, 3)) * 300.0
    d = (rng.uniform(-2, 2, (20000, 3)) - o) * rng.uniform(0.01, 5.0, (20000, 1))
    rays.append(np.concatenate([o, d], 1))
    return tri, nodes, np.concatenate(rays).astype(np.float32)


def _t_max_cases(t, rng):
    n = t.shape[0]
    with np.errstate(invalid="ignore"):
        return {
            "None": None,
            "own t": t.copy(),
            "t + ulp": np.nextafter(t, np.float32(np.inf)),
            "t - ulp": np.nextafter(t, np.float32(-np.inf)),
            "uniform": rng.uniform(0.0, 6.0, n).astype(np.float32),
            "+inf": np.full(n, np.inf, np.float32),
            "nan": np.full(n, np.nan, np.float32),
            "zero": np.zeros(n, np.float32),
            "negative": -rng.uniform(0.0, 3.0, n).astype(np.float32),
            "mixed": np.where(rng.random(n) < 0.5, np.nextafter(t, np.float32(np.inf)),
                              rng.choice(np.float32([np.nan, 0.0, 0.0005, 0.00050001, -1.0, np.inf]), n)).astype(np.float32),
        }


def _check_closest(sg, tri36, rays, dev, t_max, what):
    out = _surface(sg, rays, dev, t_max)
    tc, dc = _closest(sg, rays, dev, t_max)
    assert np.array_equal(out[0], tc), "%s: %d triangle ids differ" % (what, int((out[0] != tc).sum()))
    assert _same(out[1], dc), what
    _check_restated(tri36, rays, out, True, what)
    return out


def test_tri_and_t_equal_closest_for_every_t_max(hip, oracle, bunny_small, dev):
    rng = np.random.default_rng(71)
    rays = _broad_rays(bunny_small.tri, rng, 100000)
    sg = bunny_small.upload(hip)
    to, do = bunny_small.upload(oracle).query_hits(rays)
    assert 0.05 < (to >= 0).mean() < 0.95
    for name, t_max in _t_max_cases(do, rng).items():
        out = _check_closest(sg, bunny_small.tri, rays, dev, t_max, name)
    out = _surface(sg, rays, dev)
    assert np.array_equal(out[0], to) and _same(out[1], do)
    # NaN / <= 0.0005 t_max: dead rays, all zeros
    out = _surface(sg, rays, dev, _t_max_cases(do, rng)["nan"])
    assert (out[0] == -1).all() and not out[2].any() and not out[3].any() and not out[4].any()
    # leading dimensions are kept
    r = query.surface(sg, _gpu(rays[:6000], dev).reshape(20, 300, 6))
    assert tuple(r.tri.shape) == (20, 300) and tuple(r.point.shape) == (20, 300, 3) and tuple(r.inside.shape) == (20, 300)


def test_tri_and_t_equal_closest_on_adversarial_geometry(hip, oracle, dev):
    rng = np.random.default_rng(2024)
    tri36, nodes, rays = _nasty_scene(rng)
    sg = hip.scene_create(tri36, nodes)
    to, do = oracle.scene_create(tri36, nodes).query_hits(rays)
    assert 0.2 < (to >= 0).mean() < 0.99
    for name, t_max in _t_max_cases(do, rng).items():
        _check_closest(sg, tri36, rays, dev, t_max, name)


def test_nothing_at_or_beyond_the_reference_infinity_is_a_hit(hip, oracle, dev):
    rng = np.random.default_rng(99)
    near = rng.uniform(-2, 2, (300, 1, 3)) + rng.uniform(-0.3, 0.3, (300, 3, 3))
    far = np.array([[[-1e6, -1e6, -2e5], [1e6, -1e6, -2e5], [0.0, 1e6, -2e5]]])
    P = np.concatenate([near, far]).astype(np.float32)
    T = np.zeros((P.shape[0], 36), np.float32)
    T[:, :9] = P.reshape(-1, 9)
    T[:, 9:18] = np.tile([0, 0, 1], 3)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    hs = S.HostScene()
    hs.addTriangles(T)
    hs.buildBVHwithSAH(4)
    tri36, nodes = hs.encode()
    sg = hip.scene_create(tri36, nodes)
    n = 20000
    o = rng.uniform(-3, 3, (n, 3))
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 1.0
    rays = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    to, _ = oracle.scene_create(tri36, nodes).query_hits(rays)
    assert 0.01 < (to >= 0).mean() < 0.5
    for t_max in (None, np.full(n, np.inf, np.float32), np.full(n, 3e5, np.float32), np.full(n, 114514.0, np.float32)):
        out = _check_closest(sg, tri36, rays, dev, t_max, "far wall")
        assert np.array_equal(out[0], to)


# ---- the attributes against the restatement, all three forms; the executed chapter-3/4 shaders

@pytest.mark.parametrize("which", ["bunny_small", "c2"])
def test_attributes_equal_the_restatement(hip, bunny_small, dev, which):
    tri36, nodes = (bunny_small.tri, bunny_small.nodes) if which == "bunny_small" else RS.golden_scene("hitbvh_c2")
    rng = np.random.default_rng(5)
    rays = np.concatenate([_broad_rays(tri36, rng, 60000), RS._bunny_rays(bunny_small, rng)])
    sg = hip.scene_create(tri36, nodes)
    tc, dc = _closest(sg, rays, dev)
    assert (tc >= 0).mean() > 0.1
    outs = {}
    for integ in (3, 4, 50):
        out = outs[integ] = _surface(sg, rays, dev, integrator=integ)
        assert np.array_equal(out[0], tc) and _same(out[1], dc)
        _check_restated(tri36, rays, out, integ >= 50, "integrator %d" % integ)
        assert out[4].any()
    assert _same_out(outs[3], outs[4]) and not _same(outs[3][3], outs[50][3])


@pytest.mark.parametrize("chapter", [3, 4])
def test_chapter_3_4_forms_equal_the_executed_shaders(hip, bunny_small, dev, chapter):
    if not RS.R.fsh_available(chapter):
        pytest.skip("oracle/_ref/libezrt_ref_fsh_p%d.so not built (python oracle/ref_recipe/build_ref.py)" % chapter)
    f = RS.R.Fsh(chapter)
    f.set_scene(bunny_small.tri, bunny_small.nodes)
    rays = RS._bunny_rays(bunny_small, np.random.default_rng(30 + chapter))
    want = f.fn(8, rays)
    tri, t, point, normal, inside = _surface(bunny_small.upload(hip), rays, dev, integrator=chapter)
    hit = want[:, 0] > 0
    assert np.array_equal(tri >= 0, hit) and _same(t[hit], want[hit, 2])
    assert _same(point[hit], want[hit, 3:6]) and _same(normal[hit], want[hit, 6:9])
    assert np.array_equal(inside[hit], want[hit, 1] > 0)


# ---- every traversal route: the attribute pass does not depend on it

def test_every_route_gives_the_same_outputs(hip, oracle, bunny_small, dev):
    rng = np.random.default_rng(77)
    rays = _broad_rays(bunny_small.tri, rng, 60000)
    base = bunny_small.upload(hip)
    assert base.prune_info()["mode"] == 2 and base.prune_info()["records4"] > 0
    tc, dc = _closest(base, rays, dev)
    t_max = _t_max_cases(dc, rng)["mixed"]
    want = {tm: _surface(base, rays, dev, t_max if tm else None) for tm in (0, 1)}
    _check_restated(bunny_small.tri, rays, want[0], True, "4-wide")
    nodes = bunny_small.nodes.copy()                          # a leaf with two parents: no 4-wide records, the binary kernel
    is_leaf = nodes[:, 3] > 0
    cand = [i for i in range(2, nodes.shape[0]) if not is_leaf[i] and is_leaf[int(nodes[i, 0])]]
    q = cand[len(cand) // 3]
    nodes[q, 0] = np.float32([i for i in range(int(nodes[q, 0]) + 50, nodes.shape[0]) if is_leaf[i]][0])
    sg = hip.scene_create(bunny_small.tri, nodes)
    assert sg.prune_info()["records4"] == 0
    to, do = oracle.scene_create(bunny_small.tri, nodes).query_hits(rays)   # (another tree: the oracle's answers on it)
    for tm in (None, t_max):
        out = _surface(sg, rays, dev, tm)
        wt, wd = _closest(sg, rays, dev, tm)
        assert np.array_equal(out[0], wt) and _same(out[1], wd)
        _check_restated(bunny_small.tri, rays, out, True, "binary")
    assert np.array_equal(out[0], np.where((to >= 0) & (do < t_max), to, -1))
    for opts in ({"prune": 0}, {"prune": 1}, {"wide4": 0}, {"wide4": 0, "steal": 0}, {"instr": 1}):
        sg = bunny_small.upload(hip)
        for k, v in opts.items():
            if k == "instr":
                sg.set_instrumentation(v)
            else:
                sg.set_option(k, v)
        for tm in (0, 1):
            assert _same_out(_surface(sg, rays, dev, t_max if tm else None), want[tm]), (opts, tm)


# ---- refit

def _rotated(tri, angle):
    c, s = np.cos(angle), np.sin(angle)
    R3 = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = tri.copy()
    for k in range(6):
        t[:, 3 * k:3 * k + 3] = (tri[:, 3 * k:3 * k + 3].astype(np.float64) @ R3.T + (0.3 if k < 3 else 0.0)).astype(np.float32)
    return t


def test_refit_equals_a_fresh_scene_and_waits_for_earlier_queries(hip, bunny_small, dev):
    tri, nodes = RS.golden_scene("hitbvh_c2")
    rng = np.random.default_rng(3)
    rays = _broad_rays(tri, rng, 1 << 20)
    tri2 = _rotated(tri, 0.7)
    old = _surface(hip.scene_create(tri, nodes), rays, dev)
    fresh = _surface(hip.scene_create(tri2, refit.refit_nodes(tri2, nodes)), rays, dev)
    assert (old[0] >= 0).mean() > 0.05 and not np.array_equal(old[0], fresh[0])
    sg = hip.scene_create(tri, nodes)
    r, t2 = _gpu(rays, dev), _gpu(tri2, dev)
    qs, rs = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    before = query.surface(sg, r, stream=qs)                  # a large query issued before the refit, on another stream
    refit.refit(sg, t2, stream=rs)
    torch.cuda.synchronize()
    assert _same_out(tuple(x.cpu().numpy() for x in before), old)
    assert _same_out(_surface(sg, rays, dev), fresh)


# ---- optional outputs

def test_optional_outputs_in_every_combination(hip, bunny_small, dev):
    sg = bunny_small.upload(hip)
    rng = np.random.default_rng(6)
    rays_np = _broad_rays(bunny_small.tri, rng, 50000)
    n = rays_np.shape[0]
    rays = _gpu(rays_np, dev)
    t_max = _gpu(rng.uniform(0, 5, n).astype(np.float32), dev)
    want = query.surface(sg, rays, t_max)
    torch.cuda.synchronize()
    want = [x.cpu().numpy() for x in want]
    assert (want[0] >= 0).any() and (want[0] < 0).any()
    P = C.c_void_p
    sentinel = np.float32(-7.25)
    for mask in range(8):
        tri = torch.full((n,), 12345, dtype=torch.int32, device=dev)
        t = torch.full((n,), sentinel, device=dev)
        pt = torch.full((n, 3), sentinel, device=dev)
        nm = torch.full((n, 3), sentinel, device=dev)
        ins = torch.full((n,), 77, dtype=torch.uint8, device=dev)
        rc = hip.lib.ezrt_query_surface_device(sg._h, P(rays.data_ptr()), P(t_max.data_ptr()), n, 50, P(tri.data_ptr()),
                                               P(t.data_ptr()), P(pt.data_ptr()) if mask & 1 else None,
                                               P(nm.data_ptr()) if mask & 2 else None, P(ins.data_ptr()) if mask & 4 else None,
                                               None)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(tri.cpu().numpy(), want[0]) and _same(t.cpu().numpy(), want[1])
        for bit, buf, w, fill in ((1, pt, want[2], sentinel), (2, nm, want[3], sentinel), (4, ins, want[4], 77)):
            got = buf.cpu().numpy()
            if mask & bit:
                assert (np.array_equal(got, w.astype(np.uint8)) if bit == 4 else _same(got, w)), (mask, bit)
            else:
                assert (got == fill).all(), (mask, bit)
    miss = want[0] < 0
    assert (want[1][miss] == MISS_T).all() and not want[2][miss].any() and not want[3][miss].any() and not want[4][miss].any()


# ---- streams and scene state

def test_surface_queries_are_ordered_on_their_stream(hip, bunny_small, dev):
    rng = np.random.default_rng(8)
    n = 1 << 18
    host = _broad_rays(bunny_small.tri, rng, n)
    sg = bunny_small.upload(hip)
    want = _surface(sg, host, dev)
    src = _gpu(host, dev)
    rays = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)
        rays.copy_(src)                                        # filled after the sleep, on the same stream
        r1 = query.surface(sg, rays)                           # the current stream, `side`
        r2 = query.surface(sg, rays, stream=side)
    torch.cuda.synchronize()
    for r in (r1, r2):
        assert _same_out(tuple(x.cpu().numpy() for x in r), want)
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)
        r3 = query.surface(sg, rays)
        busy = side.query()
    assert not busy                                            # returned without waiting
    side.synchronize()
    assert _same_out(tuple(x.cpu().numpy() for x in r3), want)


def test_surface_query_beside_a_render_call(hip, bunny_small, dev):
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    p = trace.make_params(256, 256, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=4, tile=(16, 16))
    host = _broad_rays(bunny_small.tri, np.random.default_rng(21), 1 << 17)
    sg = bunny_small.upload(hip)
    rays = _gpu(host, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    sg.render_device(p, alone.data_ptr(), a.cuda_stream)
    want = query.surface(sg, rays, stream=b)
    torch.cuda.synchronize()
    alone, want = alone.cpu().numpy(), tuple(x.cpu().numpy() for x in want)
    _check_restated(bunny_small.tri, host, want, True)
    frame = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(p, frame.data_ptr(), a.cuda_stream)
    got = query.surface(sg, rays, stream=b)
    torch.cuda.synchronize()
    assert _same(frame.cpu().numpy(), alone)
    assert _same_out(tuple(x.cpu().numpy() for x in got), want)


def test_surface_queries_leave_counters_and_timings_alone(hip, bunny_small, dev):
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    sg.render(trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2))
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    rays = _gpu(_broad_rays(bunny_small.tri, np.random.default_rng(4), 50000), dev)
    for integ in (3, 50):
        query.surface(sg, rays, integrator=integ)
        query.surface(sg, rays, torch.full((50000,), 2.0, device=dev), integrator=integ)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before


# ---- errors

def test_errors(hip, oracle, bunny_small, dev):
    sg = bunny_small.upload(hip)
    lib = hip.lib
    n = 1000
    rays_np = _broad_rays(bunny_small.tri, np.random.default_rng(2), n)
    rays = _gpu(rays_np, dev)
    P = C.c_void_p
    dtri = torch.full((n,), 5, dtype=torch.int32, device=dev)
    dt = torch.full((n,), 3.0, device=dev)
    dpt = torch.full((n, 3), 3.0, device=dev)
    dnm = torch.full((n, 3), 3.0, device=dev)
    dins = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    htri, ht = np.full(n, 5, np.int32), np.full(n, 3.0, np.float32)
    hpt, hnm, hins = np.full((n, 3), 3.0, np.float32), np.full((n, 3), 3.0, np.float32), np.full(n, 9, np.uint8)
    host_rays = np.ascontiguousarray(rays_np)
    torch.cuda.synchronize()

    def call(s=sg._h, r=P(rays.data_ptr()), tm=None, cnt=n, integ=50, tri=P(dtri.data_ptr()), t=P(dt.data_ptr()),
             pt=P(dpt.data_ptr()), nm=P(dnm.data_ptr()), ins=P(dins.data_ptr())):
        return lib.ezrt_query_surface_device(s, r, tm, cnt, integ, tri, t, pt, nm, ins, None)

    # host memory in any position is rejected, never read or written
    for kw in ({"r": P(host_rays.ctypes.data)}, {"tm": P(ht.ctypes.data)}, {"tri": P(htri.ctypes.data)}, {"t": P(ht.ctypes.data)},
               {"pt": P(hpt.ctypes.data)}, {"nm": P(hnm.ctypes.data)}, {"ins": P(hins.ctypes.data)}):
        assert call(**kw) == EZRT_ERR_INVALID, kw
        assert b"device memory" in lib.ezrt_last_error()
    assert (htri == 5).all() and (ht == 3.0).all() and (hpt == 3.0).all() and (hnm == 3.0).all() and (hins == 9).all()
    # integrators outside {3, 4, 50, 51, 52}, n < 0, NULL arguments
    for integ in (0, 1, 2, 5, 49, 53, -1, 1000):
        assert call(integ=integ) == EZRT_ERR_INVALID, integ
    assert call(cnt=-1) == EZRT_ERR_INVALID
    assert call(s=None) == EZRT_ERR_INVALID
    assert call(r=None) == EZRT_ERR_INVALID
    assert call(tri=None) == EZRT_ERR_INVALID
    assert call(t=None) == EZRT_ERR_INVALID
    assert call(cnt=0) == 0
    torch.cuda.synchronize()
    assert (dtri.cpu().numpy() == 5).all() and (dt.cpu().numpy() == 3.0).all() and (dpt.cpu().numpy() == 3.0).all()
    assert (dnm.cpu().numpy() == 3.0).all() and (dins.cpu().numpy() == 9).all()
    # the rejected calls left no HIP error behind: the next call works
    out = _surface(sg, rays_np, dev)
    th, dh = sg.query_hits(rays_np)
    assert np.array_equal(out[0], th) and _same(out[1], dh)
    # the wrapper
    with pytest.raises(TypeError):
        query.surface(sg, torch.from_numpy(rays_np))
    with pytest.raises(TypeError):
        query.surface(sg, rays.double())
    with pytest.raises(TypeError):
        query.surface(bunny_small.upload(oracle), rays)
    with pytest.raises(ValueError):
        query.surface(sg, rays, integrator=5)
    with pytest.raises(ValueError):
        query.surface(sg, rays, torch.ones(n + 1, dtype=torch.float32, device=dev))
    e = query.surface(sg, torch.empty((0, 6), device=dev))
    assert e.tri.shape == (0,) and e.point.shape == (0, 3) and e.inside.shape == (0,)


# ---- a large batch on the 10^6-triangle scene

def test_a_large_batch_on_the_million_triangle_scene(hip, dev):
    bs = scenes.mega_scene()
    sg = bs.upload(hip)
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    o = torch.rand((n, 3), device=dev, generator=g) * torch.tensor([14.0, 4.3, 12.0], device=dev) - torch.tensor([7.0, 1.3, 6.0], device=dev)
    d = torch.randn((n, 3), device=dev, generator=g)
    rays = torch.cat([o, d / d.norm(dim=1, keepdim=True)], 1).contiguous()
    r = query.surface(sg, rays)
    tri, t = query.closest(sg, rays)
    torch.cuda.synchronize()
    out = tuple(x.cpu().numpy() for x in r)
    assert (out[0] >= 0).mean() > 0.3
    assert np.array_equal(out[0], tri.cpu().numpy()) and _same(out[1], t.cpu().numpy())
    _check_restated(bs.tri, rays.cpu().numpy(), out, True, "C5")

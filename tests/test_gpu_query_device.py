"""Stream-ordered device queries (include/ezrt_query.h, ezrt_amd/query.py): closest hits and bounded occlusion on device tensors,
compared on the bits with the CPU oracle's ezrt_query_hits (NaN equal to NaN):

* closest with t_max = None is ezrt_query_hits: broad ray mixes (random, camera, axis-parallel and one-zero-component rays with
  origins on box planes, unnormalised directions, rays that are not tame), k-way ties, the 10^6-triangle scene, 2^22 rays;
* occluded == (tri >= 0) & (t < t_max) on adversarial geometry (slivers, grazing rays, duplicates) with t_max at the oracle's own t,
  one ulp either side of it, random, +inf, NaN, 0, negative and None; closest with t_max is the oracle's hit filtered by t < t_max;
* the routes without the any-hit kernel: the binary kernel (boxes not nested) and scenes with pruning off;
* stream order, concurrency with a render call on another stream, untouched scene state, and the errors of the contract.
"""
import ctypes as C

import numpy as np
import pytest

from ezrt_amd import query
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
MISS_T = np.float32(114514.0)      # t of a miss in ezrt_query_hits (the reference's INF, EZ_INF)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _same(a, b):
    """equal on the bits, NaN equal to NaN"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _gpu(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def _closest(sg, rays, dev, t_max=None):
    tri, t = query.closest(sg, _gpu(rays, dev), None if t_max is None else _gpu(t_max, dev))
    torch.cuda.synchronize()
    return tri.cpu().numpy(), t.cpu().numpy()


def _occluded(sg, rays, dev, t_max=None):
    o = query.occluded(sg, _gpu(rays, dev), None if t_max is None else _gpu(t_max, dev))
    torch.cuda.synchronize()
    assert o.dtype == torch.bool
    return o.cpu().numpy()


def _filtered(to, do, t_max):
    """the contract's answers from the oracle's hits: closest (tri, t) and occluded"""
    if t_max is None:
        hit = to >= 0
    else:
        with np.errstate(invalid="ignore"):
            hit = (to >= 0) & (do < t_max)
    return np.where(hit, to, -1).astype(np.int32), np.where(hit, do, MISS_T).astype(np.float32), hit


def _check(sg, so_hits, rays, dev, t_max=None, what=""):
    to, do = so_hits
    wt, wd, wo = _filtered(to, do, t_max)
    tg, dg = _closest(sg, rays, dev, t_max)
    assert np.array_equal(tg, wt), "%s closest: %d triangle ids differ" % (what, int((tg != wt).sum()))
    assert _same(dg, wd), what
    og = _occluded(sg, rays, dev, t_max)
    assert np.array_equal(og, wo), "%s occluded: %d rays differ" % (what, int((og != wo).sum()))


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
    # zero direction components: one (semi) or two (axis-parallel), origins on vertex coordinates of the zero axis for a third
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
    # unnormalised directions
    u = n // 8
    o = rng.uniform(lo - 1, hi + 1, (u, 3))
    d = (rng.uniform(lo, hi, (u, 3)) - o) * 10.0 ** rng.uniform(-3, 3, (u, 1))
    parts.append(np.concatenate([o, d], 1))
    # not tame: +-inf components, |o| >= 3e38
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


# ---- closest hits with t_max = None: ezrt_query_hits on the bits

def test_closest_equals_the_reference_on_broad_rays(hip, oracle, bunny_small, dev):
    rng = np.random.default_rng(71)
    rays = _broad_rays(bunny_small.tri, rng)
    sg, so = bunny_small.upload(hip), bunny_small.upload(oracle)
    to, do = so.query_hits(rays)
    assert 0.05 < (to >= 0).mean() < 0.95
    tg, dg = _closest(sg, rays, dev)
    assert np.array_equal(tg, to), "%d triangle ids differ" % int((tg != to).sum())
    assert _same(dg, do)
    th, dh = sg.query_hits(rays)                               # the host route of the same library
    assert np.array_equal(tg, th) and _same(dg, dh)
    # leading dimensions are kept
    tri, t = query.closest(sg, _gpu(rays[:6000], dev).reshape(20, 300, 6))
    assert tuple(tri.shape) == (20, 300) and tuple(t.shape) == (20, 300) and tri.dtype == torch.int32
    assert np.array_equal(tri.cpu().numpy().ravel(), to[:6000])


def _copies(bunny_small, k, seed):
    """every 7th triangle of the Bunny scene, k identical copies each (different colours), shuffled: every hit is a k-way tie"""
    base = bunny_small.tri[:5300:7]
    parts = []
    for c in range(k):
        t = base.copy()
        t[:, 21:24] = (0.9 - 0.3 * c, 0.1 + 0.3 * c, 0.1)
        parts.append(t)
    tri = np.concatenate(parts)
    tri = tri[np.random.default_rng(seed).permutation(tri.shape[0])]
    hs = S.HostScene()
    hs.addTriangles(tri)
    hs.buildBVHwithSAH(8)
    return hs.encode()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_closest_keeps_the_reference_winner_of_k_way_ties(hip, oracle, bunny_small, dev, k):
    tri, nodes = _copies(bunny_small, k, 40 + k)
    rng = np.random.default_rng(50 + k)
    rays = np.concatenate([_camera_rays(40000, rng), _broad_rays(tri, rng, 40000)])
    sg, so = hip.scene_create(tri, nodes), oracle.scene_create(tri, nodes)
    to, do = so.query_hits(rays)
    assert (to >= 0).mean() > 0.05
    tg, dg = _closest(sg, rays, dev)
    assert np.array_equal(tg, to), (k, int((tg != to).sum()))
    assert _same(dg, do)
    t_max = rng.uniform(0.0, 8.0, rays.shape[0]).astype(np.float32)
    _check(sg, (to, do), rays, dev, t_max, "ties k=%d" % k)


def test_closest_on_the_deep_tree_of_the_million_triangle_scene(hip, oracle, dev):
    bs = scenes.mega_scene()
    sg, so = bs.upload(hip), bs.upload(oracle)
    rng = np.random.default_rng(5)
    n = 100000
    o = rng.uniform([-7, -1.3, -6], [7, 3, 6], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    rays[: n // 4] = _camera_rays(n // 4, rng, eye=(0.0, 2.0, 10.0))
    to, do = so.query_hits(rays)
    assert (to >= 0).mean() > 0.3
    t_max = np.where(rng.random(n) < 0.5, rng.uniform(0, 12, n), np.inf).astype(np.float32)
    _check(sg, (to, do), rays, dev, None, "mega")
    _check(sg, (to, do), rays, dev, t_max, "mega t_max")


# ---- occlusion and t_max

def _nasty_triangles(rng):
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
            parts.append(np.array([[[a[0], a[1], .25], [b[0], a[1], .25], [b[0], b[1], .25]], [[a[0], a[1], .25], [b[0], b[1], .25], [a[0], b[1], .25]]]))
    far = rng.uniform(-1, 1, (100, 1, 3)) + np.array([40.0, -35.0, 30.0]) + rng.uniform(-0.5, 0.5, (100, 3, 3)) * np.array([1.0, 1e-3, 1.0])
    parts.append(far)
    P = np.concatenate(parts).astype(np.float32)
    P = np.concatenate([P, P[:100]])
    return P


def _nasty_rays(P, rng, n_each=20000):
    rays = []
    n = P.shape[0]
    o = rng.uniform(-3, 3, (n_each, 3)); t = rng.uniform(-2, 2, (n_each, 3)); d = t - o
    rays.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    k = rng.integers(0, n, n_each)
    bc = rng.dirichlet([1, 1, 1], n_each)
    pt = (P[k] * bc[:, :, None]).sum(1)
    e1 = P[k, 1] - P[k, 0]; e2 = P[k, 2] - P[k, 0]
    N = np.cross(e1, e2); N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-30)
    u = e1 / np.maximum(np.linalg.norm(e1, axis=1, keepdims=True), 1e-30)
    v = np.cross(N, u)
    ang = rng.uniform(0, 2 * np.pi, (n_each, 1))
    inplane = np.cos(ang) * u + np.sin(ang) * v
    tilt = 10.0 ** rng.uniform(-6, -2, (n_each, 1)) * rng.choice([-1, 1], (n_each, 1))
    d = inplane + tilt * N; d /= np.linalg.norm(d, axis=1, keepdims=True)
    L = rng.uniform(0.5, 4.0, (n_each, 1))
    rays.append(np.concatenate([pt - d * L, d], 1))
    k = rng.integers(0, n, n_each)
    o = rng.uniform(-3, 3, (n_each, 3)).astype(np.float32).astype(np.float64)
    tgt = P[k, rng.integers(0, 3, n_each)].astype(np.float64)
    d = tgt - o
    rays.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    o = rng.uniform(-2, 2, (n_each, 3)); d = np.zeros((n_each, 3)); ax = rng.integers(0, 3, n_each)
    d[np.arange(n_each), ax] = rng.choice([-1.0, 1.0], n_each)
    d += rng.choice([0.0, 1e-30, 1e-12, 1e-7, 1e-4], (n_each, 1)) * rng.normal(size=(n_each, 3))
    rays.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    o = rng.uniform(-1, 1, (n_each, 3)) * 300.0
    d = (rng.uniform(-2, 2, (n_each, 3)) - o) * rng.uniform(0.01, 5.0, (n_each, 1))
    rays.append(np.concatenate([o, d], 1))
    return np.concatenate(rays).astype(np.float32)


def _tri_array(P):
    n = P.shape[0]
    T = np.zeros((n, 36), np.float32)
    T[:, :9] = P.reshape(n, 9)
    T[:, 9:18] = np.tile([0, 0, 1], 3)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    return T


@pytest.fixture(scope="module")
def nasty():
    rng = np.random.default_rng(2024)
    P = _nasty_triangles(rng)
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(_tri_array(P), np.float32))
    hs.buildBVHwithSAH(4)
    tri, nodes = hs.encode()
    return tri, nodes, _nasty_rays(P, rng)


def _t_max_cases(to, do, rng):
    n = to.shape[0]
    with np.errstate(invalid="ignore"):
        return {
            "own t": do.copy(),                                                    # t < t is false: 0 everywhere
            "t + ulp": np.nextafter(do, np.float32(np.inf)),                       # every hit counts
            "t - ulp": np.nextafter(do, np.float32(-np.inf)),
            "uniform": rng.uniform(0.0, 6.0, n).astype(np.float32),
            "+inf": np.full(n, np.inf, np.float32),
            "nan": np.full(n, np.nan, np.float32),
            "zero": np.zeros(n, np.float32),
            "negative": -rng.uniform(0.0, 3.0, n).astype(np.float32),
            "mixed": np.where(rng.random(n) < 0.5, np.nextafter(do, np.float32(np.inf)),
                              rng.choice(np.float32([np.nan, 0.0, 0.0005, 0.00050001, -1.0, np.inf]), n)).astype(np.float32),
        }


def test_occluded_on_adversarial_geometry(hip, oracle, nasty, dev):
    tri, nodes, rays = nasty
    so, sg = oracle.scene_create(tri, nodes), hip.scene_create(tri, nodes)
    assert sg.prune_info()["mode"] == 2                            # the any-hit kernel's route
    to, do = so.query_hits(rays)
    assert 0.2 < (to >= 0).mean() < 0.99
    rng = np.random.default_rng(9)
    cases = _t_max_cases(to, do, rng)
    for name, t_max in cases.items():
        _check(sg, (to, do), rays, dev, t_max, name)
    assert not _occluded(sg, rays, dev, cases["own t"]).any()
    assert np.array_equal(_occluded(sg, rays, dev, cases["t + ulp"]), to >= 0)
    assert not _occluded(sg, rays, dev, cases["nan"]).any() and not _occluded(sg, rays, dev, cases["zero"]).any()
    _check(sg, (to, do), rays, dev, None, "None")
    # the schedule's knobs do not change the answers
    for opts in ({"steal": 0}, {"handover": 0}, {"steal_bound": 0}, {"leaf_threshold": 1}, {"debug_stack_cap": 2}):
        s2 = hip.scene_create(tri, nodes)
        for k, v in opts.items():
            s2.set_option(k, v)
        _check(s2, (to, do), rays, dev, cases["mixed"], str(opts))


def test_occluded_on_broad_rays_and_segments(hip, oracle, bunny_small, dev):
    rng = np.random.default_rng(12)
    rays = _broad_rays(bunny_small.tri, rng, 100000)
    sg, so = bunny_small.upload(hip), bunny_small.upload(oracle)
    to, do = so.query_hits(rays)
    for name, t_max in _t_max_cases(to, do, rng).items():
        _check(sg, (to, do), rays, dev, t_max, name)
    # segments between two points: direction = b - a, t_max = 1 (unnormalised directions)
    a = rng.uniform(-2, 2, (50000, 3))
    b = rng.uniform(-2, 2, (50000, 3))
    seg = np.concatenate([a, b - a], 1).astype(np.float32)
    ts, ds = so.query_hits(seg)
    _check(sg, (ts, ds), seg, dev, np.ones(50000, np.float32), "segments")


def test_nothing_at_or_beyond_the_reference_infinity_is_a_hit(hip, oracle, dev):
    """The reference's traversal starts at best_t = INF (114514): a triangle farther away is a miss, whatever t_max says."""
    rng = np.random.default_rng(99)
    near = rng.uniform(-2, 2, (300, 1, 3)) + rng.uniform(-0.3, 0.3, (300, 3, 3))
    far = np.array([[[-1e6, -1e6, -2e5], [1e6, -1e6, -2e5], [0.0, 1e6, -2e5]]])   # a wall 2e5 away along -z
    P = np.concatenate([near, far]).astype(np.float32)
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(_tri_array(P), np.float32))
    hs.buildBVHwithSAH(4)
    tri, nodes = hs.encode()
    sg, so = hip.scene_create(tri, nodes), oracle.scene_create(tri, nodes)
    n = 20000
    o = rng.uniform(-3, 3, (n, 3))
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 1.0
    rays = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    to, do = so.query_hits(rays)
    assert 0.01 < (to >= 0).mean() < 0.5                      # the wall is never hit: only the near triangles
    for t_max in (None, np.full(n, np.inf, np.float32), np.full(n, 3e5, np.float32), np.full(n, 114514.0, np.float32)):
        _check(sg, (to, do), rays, dev, t_max, "far wall")


def test_routes_without_the_any_hit_kernel(hip, oracle, bunny_small, dev):
    """Boxes that are not nested (the binary kernel traces the scene) and scenes with pruning off: closest + compare, exact."""
    rng = np.random.default_rng(77)
    rays = _broad_rays(bunny_small.tri, rng, 60000)
    # a leaf with two parents: no 4-wide records
    nodes = bunny_small.nodes.copy()
    is_leaf = nodes[:, 3] > 0
    cand_q = [i for i in range(2, nodes.shape[0]) if not is_leaf[i] and is_leaf[int(nodes[i, 0])]]
    q = cand_q[len(cand_q) // 3]
    nodes[q, 0] = np.float32([i for i in range(int(nodes[q, 0]) + 50, nodes.shape[0]) if is_leaf[i]][0])
    # shrunk leaf boxes: the pruning bound does not hold, pruning switches itself off
    nodes2 = bunny_small.nodes.copy()
    leaves = np.nonzero(nodes2[:, 3] > 0)[0]
    pick = np.random.default_rng(3).choice(leaves, 40, replace=False)
    c = (nodes2[pick, 6:9] + nodes2[pick, 9:12]) * np.float32(0.5)
    nodes2[pick, 6:9] = c + (nodes2[pick, 6:9] - c) * np.float32(0.5)
    nodes2[pick, 9:12] = c + (nodes2[pick, 9:12] - c) * np.float32(0.5)
    for nd, want in ((nodes, "records4"), (nodes2, "mode")):
        sg, so = hip.scene_create(bunny_small.tri, nd), oracle.scene_create(bunny_small.tri, nd)
        info = sg.prune_info()
        assert (info["records4"] == 0) if want == "records4" else (info["mode"] == -1)
        to, do = so.query_hits(rays)
        assert (to >= 0).mean() > 0.05
        for name, t_max in _t_max_cases(to, do, rng).items():
            _check(sg, (to, do), rays, dev, t_max, "%s %s" % (want, name))
        _check(sg, (to, do), rays, dev, None, want)
    # knobs that take the same routes on an ordinary scene
    so = bunny_small.upload(oracle)
    to, do = so.query_hits(rays)
    t_max = _t_max_cases(to, do, rng)["mixed"]
    for opts in ({"prune": 0}, {"prune": 1}, {"wide4": 0}, {"wide4": 0, "steal": 0}):
        sg = bunny_small.upload(hip)
        for k, v in opts.items():
            sg.set_option(k, v)
        _check(sg, (to, do), rays, dev, t_max, str(opts))
        _check(sg, (to, do), rays, dev, None, str(opts))
    sg = bunny_small.upload(hip)
    sg.set_instrumentation(1)                                      # instrumented scenes trace with the binary kernel
    _check(sg, (to, do), rays, dev, t_max, "instr")


def test_a_large_batch(hip, oracle, bunny_small, dev):
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    o = torch.rand((n, 3), device=dev, generator=g) * 6 - 3
    d = torch.randn((n, 3), device=dev, generator=g)
    rays = torch.cat([o, d / d.norm(dim=1, keepdim=True)], 1).contiguous()
    sg = bunny_small.upload(hip)
    tri, t = query.closest(sg, rays)
    occ = query.occluded(sg, rays)
    torch.cuda.synchronize()
    r = rays.cpu().numpy()
    th, dh = sg.query_hits(r)
    assert (th >= 0).mean() > 0.05
    assert np.array_equal(tri.cpu().numpy(), th) and _same(t.cpu().numpy(), dh)
    assert np.array_equal(occ.cpu().numpy(), th >= 0)
    sub = np.random.default_rng(1).choice(n, 1 << 16, replace=False)
    to, do = bunny_small.upload(oracle).query_hits(r[sub])
    assert np.array_equal(th[sub], to) and _same(dh[sub], do)


# ---- streams and scene state

def test_queries_are_ordered_on_their_stream(hip, oracle, bunny_small, dev):
    rng = np.random.default_rng(8)
    n = 1 << 18
    host = _broad_rays(bunny_small.tri, rng, n)
    to, do = bunny_small.upload(oracle).query_hits(host)
    sg = bunny_small.upload(hip)
    src = _gpu(host, dev)
    t_max = _gpu(np.full(n, 3.0, np.float32), dev)
    rays = torch.zeros_like(src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)
        rays.copy_(src)                                        # filled after the sleep, on the same stream
        tri, t = query.closest(sg, rays)                       # default stream of the call: the current one, `side`
        occ = query.occluded(sg, rays, t_max, stream=side)
    torch.cuda.synchronize()
    assert np.array_equal(tri.cpu().numpy(), to) and _same(t.cpu().numpy(), do)
    assert np.array_equal(occ.cpu().numpy(), _filtered(to, do, np.full(n, 3.0, np.float32))[2])
    # warmed up at this n: the call returns while its stream is still busy
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)
        tri2, t2 = query.closest(sg, rays)
        occ2 = query.occluded(sg, rays, t_max)
        busy = side.query()
    assert not busy
    side.synchronize()
    assert np.array_equal(tri2.cpu().numpy(), to) and _same(t2.cpu().numpy(), do)
    assert np.array_equal(occ2.cpu().numpy(), occ.cpu().numpy())


def test_queries_run_beside_a_render_call_on_another_stream(hip, oracle, bunny_small, dev):
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    p = trace.make_params(256, 256, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=4, tile=(16, 16))
    rng = np.random.default_rng(21)
    host = _broad_rays(bunny_small.tri, rng, 1 << 17)
    to, do = bunny_small.upload(oracle).query_hits(host)
    sg = bunny_small.upload(hip)
    rays = _gpu(host, dev)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    sg.render_device(p, alone.data_ptr(), a.cuda_stream)
    tri0, t0 = query.closest(sg, rays, stream=b)               # (scratch of both in place)
    torch.cuda.synchronize()
    alone = alone.cpu().numpy()
    frame = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(p, frame.data_ptr(), a.cuda_stream)
    tri, t = query.closest(sg, rays, stream=b)
    occ = query.occluded(sg, rays, stream=b)
    torch.cuda.synchronize()
    assert _same(frame.cpu().numpy(), alone)
    assert np.array_equal(tri.cpu().numpy(), to) and _same(t.cpu().numpy(), do)
    assert np.array_equal(occ.cpu().numpy(), to >= 0)


def test_queries_leave_counters_and_timings_alone(hip, bunny_small, dev):
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    p = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2)
    sg.render(p)
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    rays = _gpu(_broad_rays(bunny_small.tri, np.random.default_rng(4), 50000), dev)
    for _ in range(2):
        query.closest(sg, rays)
        query.occluded(sg, rays, torch.full((50000,), 2.0, device=dev))
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    sg.set_instrumentation(1)                                  # (instrumented: the binary kernel, which counts everything)
    sg.counters_reset()
    query.closest(sg, rays)
    torch.cuda.synchronize()
    assert all(v == 0 for v in sg.counters().values())


# ---- errors

def test_errors(hip, oracle, bunny_small, dev):
    sg = bunny_small.upload(hip)
    lib = hip.lib
    n = 1000
    rays_np = _broad_rays(bunny_small.tri, np.random.default_rng(2), n)
    rays = _gpu(rays_np, dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    t = torch.empty(n, dtype=torch.float32, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    P = C.c_void_p
    host_rays = np.ascontiguousarray(rays_np)
    host_tri = np.zeros(n, np.int32)
    torch.cuda.synchronize()
    # host (numpy) memory is rejected, never read or written
    assert lib.ezrt_query_closest_device(sg._h, P(host_rays.ctypes.data), None, n, P(tri.data_ptr()), P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_closest_device(sg._h, P(rays.data_ptr()), None, n, P(host_tri.ctypes.data), P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_occluded_device(sg._h, P(rays.data_ptr()), P(host_rays.ctypes.data), n, P(occ.data_ptr()), None) == EZRT_ERR_INVALID
    assert b"device memory" in lib.ezrt_last_error()
    assert not host_tri.any()
    # NULL arguments, n_rays < 0, n_rays == 0
    assert lib.ezrt_query_closest_device(None, P(rays.data_ptr()), None, n, P(tri.data_ptr()), P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_closest_device(sg._h, None, None, n, P(tri.data_ptr()), P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_closest_device(sg._h, P(rays.data_ptr()), None, n, None, P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_occluded_device(sg._h, None, None, n, P(occ.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_occluded_device(sg._h, P(rays.data_ptr()), None, n, None, None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_closest_device(sg._h, P(rays.data_ptr()), None, -1, P(tri.data_ptr()), P(t.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_occluded_device(sg._h, P(rays.data_ptr()), None, -5, P(occ.data_ptr()), None) == EZRT_ERR_INVALID
    assert lib.ezrt_query_closest_device(sg._h, P(rays.data_ptr()), None, 0, P(tri.data_ptr()), P(t.data_ptr()), None) == 0
    assert lib.ezrt_query_occluded_device(sg._h, P(rays.data_ptr()), None, 0, P(occ.data_ptr()), None) == 0
    # the rejected calls left no HIP error behind: the next call works
    tg, dg = _closest(sg, rays_np, dev)
    th, dh = sg.query_hits(rays_np)
    assert np.array_equal(tg, th) and _same(dg, dh)
    # the wrapper
    with pytest.raises(TypeError):
        query.closest(sg, torch.from_numpy(rays_np))                       # CPU tensor
    with pytest.raises(TypeError):
        query.occluded(sg, rays.double())                                  # dtype
    with pytest.raises(TypeError):
        query.occluded(sg, rays, torch.ones(n, dtype=torch.float32))       # CPU t_max
    with pytest.raises(TypeError):
        query.closest(bunny_small.upload(oracle), rays)                    # a scene of the oracle library
    with pytest.raises(ValueError):
        query.closest(sg, rays.reshape(-1)[: 5 * n].reshape(n, 5).contiguous())
    with pytest.raises(ValueError):
        query.occluded(sg, rays, torch.ones(n + 1, dtype=torch.float32, device=dev))
    e0, e1 = query.closest(sg, torch.empty((0, 6), device=dev))
    assert e0.shape == (0,) and e1.shape == (0,)

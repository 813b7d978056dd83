"""Scenes and rays of the all-hits tests (tests/test_allhits_expected.py on the CPU, tests/test_gpu_allhits.py on the device): the
generators of tests/test_gpu_query_device.py restated at the smallest sizes that still reach every case (a helper, no test)."""
import numpy as np

from ezrt_amd import scene as S

N_RAYS = 4000


def camera_rays(n, rng, eye=(0.0, 0.0, 4.0), spread=0.6):
    o = np.tile(np.asarray(eye, np.float32), (n, 1))
    d = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), -1.5 * np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def broad_rays(tri, rng, n):
    """random; axis-parallel and one-zero-component rays (a third with origins on box planes); unnormalised; not tame"""
    P = tri[:, :9].reshape(-1, 3, 3)
    lo, hi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)       # the bulk of the mesh: a few far vertices (a floor) do not thin the mix
    parts = []
    k = n // 4
    o = rng.uniform(lo - 1, hi + 1, (k, 3))
    d = rng.uniform(lo, hi, (k, 3)) - o
    parts.append(np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], 1))
    m = 3 * n // 8
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
    u = n // 4
    o = rng.uniform(lo - 1, hi + 1, (u, 3))
    d = (rng.uniform(lo, hi, (u, 3)) - o) * 10.0 ** rng.uniform(-3, 3, (u, 1))
    parts.append(np.concatenate([o, d], 1))
    w = n - k - m - u
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


def rays_for(tri, seed, n=N_RAYS, eye=(0.0, 0.0, 4.0), spread=0.6):
    """half camera-style rays (directions within +-spread / 1.5 of the axis), half the broad mix, shuffled"""
    rng = np.random.default_rng(seed)
    rays = np.concatenate([camera_rays(n // 2, rng, eye, spread), broad_rays(tri, rng, n - n // 2)])
    return np.ascontiguousarray(rays[rng.permutation(n)], np.float32)


def copies(bunny_small, k, seed):
    """every 7th triangle of the Bunny scene, k identical copies each (different colours), shuffled: every crossing is a k-way tie"""
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


def _nasty_triangles(rng):
    """blobs, slivers, a coplanar grid, a far cluster, duplicates"""
    parts = []
    c = rng.uniform(-2, 2, (1500, 1, 3))
    parts.append(c + rng.uniform(-0.15, 0.15, (1500, 3, 3)))
    p1 = rng.uniform(-2, 2, (600, 3))
    e = rng.normal(size=(600, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    o = np.cross(e, rng.normal(size=(600, 3)))
    o /= np.linalg.norm(o, axis=1, keepdims=True)
    w = 10.0 ** rng.uniform(-5, -2, (600, 1))
    parts.append(np.stack([p1, p1 + 2.0 * e, p1 + rng.uniform(0.2, 1.8, (600, 1)) * e + w * o], 1))
    g = np.linspace(-2, 2, 17)
    for i in range(16):
        for j in range(16):
            a, b = (g[i], g[j]), (g[i + 1], g[j + 1])
            parts.append(np.array([[[a[0], a[1], .25], [b[0], a[1], .25], [b[0], b[1], .25]],
                                   [[a[0], a[1], .25], [b[0], b[1], .25], [a[0], b[1], .25]]]))
    far = rng.uniform(-1, 1, (100, 1, 3)) + np.array([40.0, -35.0, 30.0]) + rng.uniform(-0.5, 0.5, (100, 3, 3)) * np.array([1.0, 1e-3, 1.0])
    parts.append(far)
    P = np.concatenate(parts).astype(np.float32)
    return np.concatenate([P, P[:100]])


def nasty():
    P = _nasty_triangles(np.random.default_rng(2024))
    n = P.shape[0]
    T = np.zeros((n, 36), np.float32)
    T[:, :9] = P.reshape(n, 9)
    T[:, 9:18] = np.tile([0, 0, 1], 3)
    T[:, 18:36] = S.Material.disney(baseColor=(0.8, 0.6, 0.4)).to18()
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(T, np.float32))
    hs.buildBVHwithSAH(4)
    return hs.encode()


def not_nested(bunny_small):
    """The Bunny scene with a leaf that has two parents: its boxes are not nested, so the scene has no 4-wide records and the
    render calls and the closest-hit queries trace it with the binary kernel."""
    nodes = bunny_small.nodes.copy()
    is_leaf = nodes[:, 3] > 0
    cand = [i for i in range(2, nodes.shape[0]) if not is_leaf[i] and is_leaf[int(nodes[i, 0])]]
    q = cand[len(cand) // 3]
    nodes[q, 0] = np.float32([i for i in range(int(nodes[q, 0]) + 50, nodes.shape[0]) if is_leaf[i]][0])
    return bunny_small.tri, nodes


def scene(name, bunny_small):
    """(tri, nodes, rays) of the named test scene"""
    if name == "bunny":
        tri, nodes = bunny_small.tri, bunny_small.nodes
        return tri, nodes, rays_for(tri, 101)
    if name == "ties":
        tri, nodes = copies(bunny_small, 3, 43)
        return tri, nodes, rays_for(tri, 102, eye=(0.3, -0.6, 4.0), spread=0.25)   # (a thinned mesh: a narrow cone at its middle)
    if name == "nasty":
        tri, nodes = nasty()
        return tri, nodes, rays_for(tri, 103)
    assert name == "not_nested"
    tri, nodes = not_nested(bunny_small)
    return tri, nodes, rays_for(tri, 104, 2000)


SCENES = ("bunny", "ties", "nasty", "not_nested")

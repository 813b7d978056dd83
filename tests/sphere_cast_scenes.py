"""Scenes and queries of the sphere-cast tests (tests/test_sphere_cast_expected.py on the CPU, tests/test_gpu_sphere_cast.py on the
device, tools/sphere_cast_host_check.py; a helper, no test).

queries_for: about 2 000 (ray, radius) per scene with a fixed seed.  Origins on a shell around the scene and inside its bounding box;
directions at the scene (at faces, at edge midpoints and at vertices, from the outside along the summed normals of the faces that meet there, so that every kind
of feature supplies winners), past it and away from it, of lengths 0.25 .. 4 (t is in units of d); radii from 0 to a quarter of the
extent, r = 0 included; starts that touch; direction components that are exactly 0 or -0; a few queries that are not live.  On a
scene whose coordinates are multiples of 1/4 (the voxel solid), axis rays with origins and radii on multiples of 1/8: t is then the
inflated box plane exactly, coplanar neighbours and shared edges tie, and the index rule decides.

constructed: pairs with known answers on an integer grid, exact in fp32 -- one scene that holds them all, 64 apart along x."""
import numpy as np

import allhits_scenes as A
import inside_scenes as IS

F = np.float32
NAMES = ("voxel_solid", "bunny", "nasty")
SEED = 2000                                                        # + the scene's index
N_DEAD = 12


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)


def dead_queries(lo, hi, rng):
    """(rays float32 [12, 6], radius [12]): each clause of the liveness rule once"""
    o = rng.uniform(lo, hi, (N_DEAD, 3))
    d = _unit(rng.normal(size=(N_DEAD, 3)))
    rays = np.concatenate([o, d], 1).astype(F)
    r = np.full(N_DEAD, 0.05 * float(np.max(hi - lo)), F)
    rays[0, 0] = np.nan                                            # o
    rays[1, 1] = np.inf
    rays[2, 4] = np.nan                                            # d
    rays[3, 5] = -np.inf
    r[4] = np.nan                                                  # r
    r[5] = np.inf
    r[6] = -1.0
    rays[7, 3:] = 0.0                                              # dot(d, d) = 0
    rays[8, 3:] = (0.0, -0.0, 0.0)
    rays[9, 3:] = (3e19, 3e19, 0.0)                                # dot(d, d) overflows
    rays[10, 3] = 1e-39                                            # a component whose reciprocal overflows
    rays[11, 3:] = (0.0, 1e-42, -1e-41)
    return rays, r


def queries_for(tri, seed, n=2000):
    """(rays float32 [n', 6], radius float32 [n']) for the scene's triangle array [m, 36]"""
    rng = np.random.default_rng(seed)
    T = np.ascontiguousarray(tri, F).reshape(-1, 36)
    ok = np.isfinite(T[:, :9]).all(1)
    P = T[ok, :9].reshape(-1, 3, 3).astype(np.float64)
    N = T[ok, 9:18].reshape(-1, 3, 3).astype(np.float64)
    lo, hi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(hi - lo))
    centre = 0.5 * (lo + hi)
    m = P.shape[0]
    face_n = _unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    face_n = face_n * np.where((face_n * _unit(N[:, 0])).sum(1) < 0, -1.0, 1.0)[:, None]      # on the side of the shading normal
    _, corner = np.unique(P.reshape(-1, 3), axis=0, return_inverse=True)                    # the outward direction at a corner: the
    summed = np.zeros((int(corner.max()) + 1, 3))                                            # faces that meet there, summed
    np.add.at(summed, corner.reshape(-1), np.repeat(face_n, 3, 0))
    out_n = _unit(summed[corner.reshape(-1)]).reshape(-1, 3, 3)
    count = np.bincount(corner.reshape(-1))
    blunt = (np.linalg.norm(summed, axis=1) / count)[corner.reshape(-1)].reshape(-1, 3)     # 1 on a flat patch, less at a corner
    reach = np.full(summed.shape[0], -np.inf)                                                # how far a face at the corner rises along
    for j in range(3):                                                                       # that direction: <= 0 at a convex corner
        np.maximum.at(reach, corner.reshape(-1), ((P[:, j][:, None, :] - P) * out_n).sum(-1).reshape(-1))
    sharp = np.argwhere((blunt < 0.9) & (reach[corner.reshape(-1)].reshape(-1, 3) <= 1e-9 * size))   # (triangle, vertex) of the convex corners
    O, D, R = [], [], []

    def add(o, d, r):
        O.append(o), D.append(d * rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], (o.shape[0], 1))), R.append(np.broadcast_to(r, o.shape[:1]))

    def radii(k, top=0.25):
        r = size * np.where(rng.random(k) < 0.5, rng.uniform(0, top, k), 10.0 ** rng.uniform(-4, -1, k))
        r[::11] = 0.0
        return r

    def target(k, kind):
        """(point on the mesh, outward direction there): face points, edge midpoints, vertices"""
        t, e = rng.integers(0, m, k), rng.integers(0, 3, k)
        if kind == 0:
            w = rng.dirichlet((1, 1, 1), k)
            return (P[t] * w[:, :, None]).sum(1), face_n[t]
        if kind == 1:
            return 0.5 * (P[t, e] + P[t, (e + 1) % 3]), _unit(out_n[t, e] + out_n[t, (e + 1) % 3])
        if sharp.shape[0] >= 16:                                       # a vertex in a flat patch is never the first contact
            t, e = sharp[rng.integers(0, sharp.shape[0], k)].T
        return P[t, e], out_n[t, e]

    k = n // 12
    shell = lambda k: centre + _unit(rng.normal(size=(k, 3))) * size * rng.uniform(0.7, 1.3, (k, 1))  # noqa: E731
    for kind in (0, 1, 2, 2):                                          # from the shell at a feature, and from just outside it along its normal
        p, out = target(k, kind)
        o = shell(k)
        add(o, _unit(p - o), radii(k))
        p, out = target(k, kind)
        r = radii(k, 0.08)
        o = p + out * (r + size * rng.uniform(0.01, 0.3, k))[:, None] + rng.normal(size=(k, 3)) * size * 0.003
        add(o, _unit(p - o), r)
    o = shell(k)                                                       # past the scene: at a point off it
    add(o, _unit(centre + _unit(rng.normal(size=(k, 3))) * size * rng.uniform(0.5, 1.0, (k, 1)) - o), radii(k))
    o = shell(k)                                                       # away from it
    add(o, _unit(o - centre + rng.normal(size=(k, 3)) * 0.3 * size), radii(k))
    o = rng.uniform(lo, hi, (k, 3))                                    # inside the bounding box, anywhere
    add(o, _unit(rng.normal(size=(k, 3))), radii(k, 0.1))
    p, out = target(k, 0)                                              # starts that touch: nearer to the surface than r
    r = size * rng.uniform(0.01, 0.2, k)
    add(p + out * (r * rng.uniform(0, 0.98, k))[:, None], _unit(rng.normal(size=(k, 3))), r)
    rays = np.concatenate([np.concatenate(O), np.concatenate(D)], 1).astype(F)
    radius = np.concatenate(R).astype(F)
    z = rng.permutation(rays.shape[0])[:rays.shape[0] // 8]            # direction components that are exactly 0 or -0
    rays[z, 3 + rng.integers(0, 3, z.size)] = np.where(rng.random(z.size) < 0.5, F(0.0), F(-0.0))
    z2 = z[:z.size // 3]
    rays[z2, 3 + rng.integers(0, 3, z2.size)] = F(0.0)
    grid = np.all(T[ok, :9] * 4 == np.round(T[ok, :9] * 4))            # the voxel solid: axis rays on the 1/8 grid
    if grid:
        g = n // 8
        glo, ghi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
        o = np.round(rng.uniform(glo - 1.0, ghi + 1.0, (g, 3)) * 8) / 8
        axis, sign = rng.integers(0, 3, g), rng.choice([-1.0, 1.0], g)
        o[np.arange(g), axis] = np.where(sign > 0, glo[axis] - 1.5, ghi[axis] + 1.5)
        d = np.zeros((g, 3))
        d[np.arange(g), axis] = sign * rng.choice([0.5, 1.0, 2.0], g)
        d[::2][d[::2] == 0] = -0.0
        rays = np.concatenate([rays, np.concatenate([o, d], 1).astype(F)])
        radius = np.concatenate([radius, (rng.integers(0, 9, g) / 8).astype(F)])
    dr, dd = dead_queries(lo, hi, rng)
    rays, radius = np.concatenate([rays, dr]), np.concatenate([radius, dd])
    order = rng.permutation(rays.shape[0])
    return np.ascontiguousarray(rays[order], F), np.ascontiguousarray(radius[order], F)


def host_case(name, bunny_small, leaf=None):
    """(tri, nodes, rays, radius) of the named scene; `leaf` rebuilds the tree with buildBVHwithSAH(leaf), which reorders the
    triangles (the queries stay those of the scene as it comes)"""
    if name == "voxel_solid":
        v = IS.voxel_solid()
        tri, nodes = v["tri"], v["nodes"]
    else:
        tri, nodes, _ = A.scene(name, bunny_small)
    rays, radius = queries_for(tri, SEED + NAMES.index(name))
    if leaf is not None:
        tri, nodes = IS.build(tri, leaf)
    return tri, nodes, rays, radius


def caps(want):
    """the shares the tests require of a bit-for-bit batch, from the restatement's answer (tri, t, point, touching, sub)"""
    tri, t, _, touching, sub = want
    swept = (tri >= 0) & (touching == 0)
    won = max(1, int(swept.sum()))
    return dict(swept=float((swept & (t > 0)).mean()), touching=float((touching == 1).mean()), miss=float((tri < 0).mean()),
                face=float((sub[swept] == 0).sum()) / won, edge=float(((sub[swept] >= 1) & (sub[swept] <= 3)).sum()) / won,
                vertex=float((sub[swept] >= 4).sum()) / won)


def caps_met(want):
    c = caps(want)
    return c["swept"] >= 0.10 and c["touching"] >= 0.10 and c["miss"] >= 0.10 and min(c["face"], c["edge"], c["vertex"]) >= 0.05


# ---- constructed pairs on the triangle (0,0,0) (8,0,0) (0,8,0): (name, o, d, r, tri hit?, t, point, touching, sub); integers and
# powers of two, so every number below is exact in fp32.  t None: the answer is the restatement's, only its kind is known.
ONE_UP = float(np.nextafter(F(1), F(2)))
CASES = (
    ("face contact", [2, 2, 5], [0, 0, -1], 1, True, 4, [2, 2, 0], 0, 0),
    ("face contact, d of length 2", [2, 2, 5], [0, 0, -2], 1, True, 2, [2, 2, 0], 0, 0),
    ("face contact from below", [2, 2, -5], [0, 0, 1], 1, True, 4, [2, 2, 0], 0, 0),
    ("a ray (r = 0) onto the face", [2, 2, 5], [0, 0, -1], 0, True, 5, [2, 2, 0], 0, 0),
    ("edge contact in the plane", [4, -5, 0], [0, 1, 0], 1, True, 4, [4, 0, 0], 0, 1),
    ("vertex contact in the plane", [-6, -8, 0], [3, 4, 0], 5, True, 1, [0, 0, 0], 0, 4),
    ("grazing an edge from above", [4, -5, 1], [0, 1, 0], 1, True, 5, [4, 0, 0], 0, 1),
    ("passing over the edge", [4, -5, 2], [0, 1, 0], 1, False, np.inf, [0, 0, 0], 0, -1),
    ("moving away", [2, 2, 5], [0, 0, 1], 1, False, np.inf, [0, 0, 0], 0, -1),
    ("a start that touches", [2, 2, 0.5], [0, 0, -1], 1, True, 0, [2, 2, 0], 1, -1),
    ("a start that touches exactly", [2, 2, 1], [0, 0, 1], 1, True, 0, [2, 2, 0], 1, -1),
    ("one ulp clear, moving inward", [2, 2, ONE_UP], [0, 0, -1], 1, True, None, [2, 2, 0], 0, 0),
)
SPACING = 64


def constructed(leaf=4):
    """(tri [m, 36], nodes, rays float32 [n, 6], radius [n], index of each case's triangle [n])"""
    base = F([[0, 0, 0], [8, 0, 0], [0, 8, 0]])
    P, rays, radius = [], [], []
    for k, c in enumerate(CASES):
        shift = F([SPACING * k, 0, 0])
        P.append(base + shift)
        rays.append(np.concatenate([F(c[1]) + shift, F(c[2])]))
        radius.append(c[3])
    filler = [F([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) + F([SPACING * k, 40 + 3 * j, 0]) for k in range(len(CASES)) for j in range(3)]
    tri, nodes = IS.build(IS.tri36(np.stack(P + filler)), leaf)
    V = np.ascontiguousarray(tri, F)[:, :9].reshape(-1, 3, 3)
    where = np.array([int(np.nonzero((V == p).all((1, 2)))[0][0]) for p in P])
    return tri, nodes, np.ascontiguousarray(np.stack(rays), F), F(radius), where


# ---- the tree shapes of tests/tree_shapes.py

def shape_queries(tri, expect, seed, n=192):
    """(rays float32 [n', 6], radius [n']): about 260 queries for a shape of tests/tree_shapes.py -- queries_for's, then 32 aimed at
    the triangles that no leaf holds and 32 at the duplicated ones (where the shape has such), with small radii"""
    import tree_shapes as T
    rays, radius = queries_for(tri, seed, 2 * n)
    rays, radius = rays[:n], radius[:n]
    V = T.vertices(tri)
    rng = np.random.default_rng(seed + 7)
    size = float(np.max(np.ptp(V.reshape(-1, 3), axis=0)))
    extra = [np.asarray(expect.get("uncovered", []), int), T.copied(tri) if V.shape[0] > 8 else np.zeros(0, int)]
    for ids in extra:
        if ids.size:
            a = T.aimed_rays(V, np.resize(ids, 32), rng)
            rays = np.concatenate([rays, a])
            radius = np.concatenate([radius, (size * rng.choice([0.0, 0.001, 0.01], 32)).astype(F)])
    return np.ascontiguousarray(rays, F), np.ascontiguousarray(radius, F)

"""A numpy float32 restatement of the surface attributes of a hit (include/ezrt_surface.h: hit point, shading normal, side), pinned
here against the reference's own executed hitBVH records so that the GPU tests (tests/test_gpu_surface_query.py) can use it as a
yardstick on scenes and forms that have no goldens.

`restate` follows shade_point / surface_point (ezrt_amd/csrc/hip/ezrt_device.h) operation by operation, in its evaluation order:
left-to-right sums, no fused multiply-add, correctly rounded division and square root (normalize = v * (1 / sqrt(dot(v, v)))).  The
geometric normal is the scene record's (ezi::tri_normal: normalize(cross(p2 - p1, p3 - p1)) in the same style), the two denominator
pairs are shade_denominators'.  Fed the oracle's {tri, t} (ezrt_query_hits), it must reproduce isInside (field 1), hitPoint (3:6)
and the normal (6:9) of every hit of the four hitBVH record sets of tests/golden/fsh_golden.npz -- 16 384 rays of the executed
chapter-5 shader on C2, the scene of exact ties, C3 and C5 -- on the bits.  Where oracle/_ref was built, the chapter-3/4 form is
checked against those chapters' executed hitBVH as well."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import make_fsh_golden as G  # noqa: E402  (the scenes of the goldens; reading them needs no oracle/_ref)
from oracle import ref as R  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fsh_golden.npz"))
HITBVH_SETS = ("hitbvh_c2", "hitbvh_ties", "hitbvh_c3", "hitbvh_c5")

F = np.float32


def _normalize(x, y, z):
    inv = F(1.0) / np.sqrt((x * x + y * y) + z * z)
    return x * inv, y * inv, z * inv


def restate(tri36, rays, tri_id, t, p5):
    """(point [n, 3], normal [n, 3], inside [n] bool) of the rays with tri_id >= 0 at distance t; zeros elsewhere.  p5: the
    P5/fsh:206-207 form of the smooth normal (+1e-7), else P3/fsh:273-274 = P4/fsh:196-197 (+-0.00005)."""
    tri36 = np.ascontiguousarray(tri36, F).reshape(-1, 36)
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    tri_id = np.asarray(tri_id).ravel()
    t = np.ascontiguousarray(t, F).ravel()
    n = rays.shape[0]
    point = np.zeros((n, 3), F)
    normal = np.zeros((n, 3), F)
    inside = np.zeros(n, bool)
    hit = tri_id >= 0
    T = tri36[tri_id[hit]]
    Sx, Sy, Sz = (rays[hit, k] for k in range(3))
    dx, dy, dz = (rays[hit, k] for k in range(3, 6))
    tt = t[hit]
    p1x, p1y, p1z, p2x, p2y, p2z, p3x, p3y, p3z = (T[:, k] for k in range(9))
    n1 = (T[:, 9], T[:, 10], T[:, 11])
    n2 = (T[:, 12], T[:, 13], T[:, 14])
    n3 = (T[:, 15], T[:, 16], T[:, 17])
    with np.errstate(all="ignore"):
        # the geometric normal of the scene record (ezi::tri_normal, P5/fsh:172)
        e1x, e1y, e1z = p2x - p1x, p2y - p1y, p2z - p1z
        e2x, e2y, e2z = p3x - p1x, p3y - p1y, p3z - p1z
        cx, cy, cz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
        inv = F(1.0) / np.sqrt((cx * cx + cy * cy) + cz * cz)
        Nx, Ny, Nz = cx * inv, cy * inv, cz * inv
        ins = ((Nx * dx + Ny * dy) + Nz * dz) > F(0.0)
        Px, Py, Pz = Sx + dx * tt, Sy + dy * tt, Sz + dz * tt
        # shade_denominators
        if p5:
            da = (-(p1x - p2x)) * (p3y - p2y) + (p1y - p2y) * (p3x - p2x) + F(1e-7)
            db = (-(p2x - p3x)) * (p1y - p3y) + (p2y - p3y) * (p1x - p3x) + F(1e-7)
        else:
            e = F(0.00005)
            da = (-(p1x - p2x - e)) * (p3y - p2y + e) + (p1y - p2y + e) * (p3x - p2x + e)
            db = (-(p2x - p3x - e)) * (p1y - p3y + e) + (p2y - p3y + e) * (p1x - p3x + e)
        alpha = ((-(Px - p2x)) * (p3y - p2y) + (Py - p2y) * (p3x - p2x)) / da
        beta = ((-(Px - p3x)) * (p1y - p3y) + (Py - p3y) * (p1x - p3x)) / db
        gama = (F(1.0) - alpha) - beta
        sx, sy, sz = _normalize((n1[0] * alpha + n2[0] * beta) + n3[0] * gama, (n1[1] * alpha + n2[1] * beta) + n3[1] * gama,
                                (n1[2] * alpha + n2[2] * beta) + n3[2] * gama)
    point[hit] = np.stack([Px, Py, Pz], 1)
    normal[hit] = np.stack([np.where(ins, -sx, sx), np.where(ins, -sy, sy), np.where(ins, -sz, sz)], 1)
    inside[hit] = ins
    return point, normal, inside


def same_bits(a, b):
    """equal on the bits, NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


_SCENES = {}


def golden_scene(key):
    """(tri36, nodes) of the scene a hitBVH record set was taken on"""
    if key not in _SCENES:
        if key == "hitbvh_ties":
            _SCENES[key] = G.tie_scene()
        else:
            bs = G.big_scene(G.BIG_TREES[key][0] if key in G.BIG_TREES else "c2")
            _SCENES[key] = (bs.tri, bs.nodes)
    return _SCENES[key]


@pytest.mark.parametrize("key", HITBVH_SETS)
def test_restatement_reproduces_the_executed_shaders_hit_records(oracle, key):
    tri, nodes = golden_scene(key)
    rays, want = GOLD[key + "_rays"], GOLD[key]
    to, do = oracle.scene_create(tri, nodes).query_hits(rays)
    hit = want[:, 0] > 0
    assert np.array_equal(to >= 0, hit)
    assert 0.2 < hit.mean() < 0.95
    point, normal, inside = restate(tri, rays, to, do, p5=True)
    assert same_bits(point[hit], want[hit, 3:6])
    assert same_bits(normal[hit], want[hit, 6:9])
    assert np.array_equal(inside[hit], want[hit, 1] > 0)
    # the goldens exercise both sides, and the other form of the normal is not the same arithmetic
    assert inside[hit].any() and not inside[hit].all()
    assert not same_bits(restate(tri, rays, to, do, p5=False)[1][hit], want[hit, 6:9])
    # misses: zeros
    assert not point[~hit].any() and not normal[~hit].any() and not inside[~hit].any()


def _bunny_rays(bunny_small, rng, n=6000):
    """camera rays, rays leaving surface points in random directions, axis-parallel rays"""
    from ezrt_amd import scene as S
    eye, cam = S.camera(10, 5, 3)
    m = np.asarray(cam, np.float64).reshape(4, 4).T
    px, py = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    d = px[:, None] * m[:3, 0] + py[:, None] * m[:3, 1] - 1.5 * m[:3, 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cam_rays = np.concatenate([np.broadcast_to(np.asarray(eye, np.float64), d.shape), d], 1)
    P = bunny_small.tri[:, :9].reshape(-1, 3, 3).astype(np.float64)
    k = rng.integers(0, P.shape[0], n)
    bc = rng.dirichlet([1, 1, 1], n)
    o = (P[k] * bc[:, :, None]).sum(1)
    u = rng.normal(size=(n, 3))
    surf = np.concatenate([o, u / np.linalg.norm(u, axis=1, keepdims=True)], 1)
    axis = np.concatenate([rng.uniform(-1, 1, (600, 3)), np.tile(np.eye(3), (200, 1)) * rng.choice([-1, 1], (600, 1))], 1)
    return np.concatenate([cam_rays, surf, axis]).astype(np.float32)


@pytest.mark.parametrize("chapter", [3, 4])
def test_restatement_of_the_chapter_3_4_form_against_the_executed_shaders(oracle, bunny_small, chapter):
    if not R.fsh_available(chapter):
        pytest.skip("oracle/_ref/libezrt_ref_fsh_p%d.so not built (python oracle/ref_recipe/build_ref.py)" % chapter)
    f = R.Fsh(chapter)
    f.set_scene(bunny_small.tri, bunny_small.nodes)
    rays = _bunny_rays(bunny_small, np.random.default_rng(30 + chapter))
    want = f.fn(8, rays)
    to, do = oracle.scene_create(bunny_small.tri, bunny_small.nodes).query_hits(rays)
    hit = want[:, 0] > 0
    assert np.array_equal(to >= 0, hit) and 0.3 < hit.mean() < 0.99
    point, normal, inside = restate(bunny_small.tri, rays, to, do, p5=False)
    assert same_bits(point[hit], want[hit, 3:6])
    assert same_bits(normal[hit], want[hit, 6:9])
    assert np.array_equal(inside[hit], want[hit, 1] > 0) and inside[hit].any()

"""tests/sphere_cast_expected.py -- the numpy restatement of include/ezrt_sphere_cast.h that the device tests compare with on the
bits -- pinned to true geometry, on the CPU.

The truth is written independently of the restatement, in float64 and in another form: the direction normalised, the point-triangle
distance by barycentric projection and segment clamps, the cylinder in its scalar coefficients, the larger-magnitude root formula,
no gate, no clamp to tnear, no "already inside" rule.  It is itself cross-checked by marching closest_point_expected (fp32, the
existing restatement of ezrt_closest_point.h) along a subset of the rays.

Measured on the inputs of tests/sphere_cast_scenes.py (the three scenes, about 2 000 queries each, and the constructed pairs): the
largest residual |dist(o + d*t, mesh) - r| of a swept answer, relative to the scene's extent, is
8.16e-8 on the voxel solid, 1.59e-7 on the Bunny scene and 1.03e-6 on the adversarial scene (RESIDUAL_MEASURED); the tests assert TOL = twice the largest, rounded up to a power of two: 2^-18."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_point_expected as E  # noqa: E402
import sphere_cast_expected as SE  # noqa: E402
import sphere_cast_scenes as SS  # noqa: E402
import tree_shapes as T  # noqa: E402

F = np.float32
RESIDUAL_MEASURED = {"voxel_solid": 8.16e-8, "bunny": 1.59e-7, "nasty": 1.03e-6}  # test_residual_and_no_tunnelling prints them
TOL = 2.0 ** -18                                                    # 3.81e-6 >= 2 * 1.03e-6 > 2 ** -19
CHUNK = 1 << 17


# ---- the float64 truth

def extent(tri):
    P = SE.vertices(tri)
    P = P[np.isfinite(P).all((1, 2))].astype(np.float64).reshape(-1, 3)
    lo, hi = np.percentile(P, [2, 98], axis=0)
    return float(np.max(hi - lo))


def _d(u, w):
    return (u * w).sum(-1)


def tri_dist(p, a, b, c):
    """float64 distance of points p to triangles (a, b, c), row by row"""
    def seg(u, v):
        e = v - u
        ee = _d(e, e)
        s = np.clip(_d(p - u, e) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        g = p - (u + e * s[:, None])
        return _d(g, g)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d00, d01, d11, d20, d21 = _d(ab, ab), _d(ab, ac), _d(ac, ac), _d(ap, ab), _d(ap, ac)
        den = d00 * d11 - d01 * d01
        v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        n = np.cross(ab, ac)
        plane = _d(ap, n) ** 2 / _d(n, n)
        inside = (den > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
        best = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
        return np.sqrt(np.where(inside, np.minimum(plane, best), best))


def cast_pairs(o, dh, r, a, b, c):
    """float64 arc length s >= 0 at which the sphere (o + dh s, r), |dh| = 1, first touches the triangle, row by row; inf for none;
    0 where it touches at the start"""
    inf = np.inf
    with np.errstate(all="ignore"):
        out = np.full(o.shape[0], inf)
        ab, ac = b - a, c - a
        n = np.cross(ab, ac)
        ln = np.sqrt(_d(n, n))
        nh = n / ln[:, None]
        h = _d(o - a, nh)
        nh = np.where((h < 0)[:, None], -nh, nh)
        h = np.abs(h)
        vel = _d(dh, nh)
        s = (h - r) / -vel
        foot = o + dh * s[:, None] - nh * r[:, None]
        ap = foot - a
        d00, d01, d11, d20, d21 = _d(ab, ab), _d(ab, ac), _d(ac, ac), _d(ap, ab), _d(ap, ac)
        den = d00 * d11 - d01 * d01
        v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        ok = (ln > 0) & (vel < 0) & (s >= 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
        out = np.where(ok, np.minimum(out, s), out)
        for u, v_ in ((a, b), (b, c), (c, a)):
            e = v_ - u
            le = np.sqrt(_d(e, e))
            eh = e / le[:, None]
            m = o - u
            de, me = _d(dh, eh), _d(m, eh)
            A, B, C = 1.0 - de * de, _d(m, dh) - me * de, _d(m, m) - me * me - r * r
            disc = B * B - A * C
            s = (-B - np.sqrt(disc)) / A
            along = me + s * de
            ok = (le > 0) & (A > 0) & (disc >= 0) & (s >= 0) & (along >= 0) & (along <= le)
            out = np.where(ok, np.minimum(out, s), out)
        for p in (a, b, c):
            m = o - p
            B, C = _d(m, dh), _d(m, m) - r * r
            disc = B * B - C
            s = -B - np.sqrt(disc)
            ok = (disc >= 0) & (s >= 0)
            out = np.where(ok, np.minimum(out, s), out)
        return np.where(tri_dist(o, a, b, c) <= r, 0.0, out)


class Truth:
    """the pairs (query, triangle) whose triangle comes within r + slack of the ray at all -- by its bounding sphere, in float64 --
    and the float64 answers over them"""

    def __init__(self, rays, radius, tri, slack):
        o, d, r = SE.split(rays, radius)
        self.alive = SE.live(rays, radius)
        self.o, self.r = o.astype(np.float64), r.astype(np.float64)
        self.len = np.sqrt(_d(d.astype(np.float64), d.astype(np.float64)))
        with np.errstate(all="ignore"):
            self.dh = d.astype(np.float64) / self.len[:, None]
        V = SE.vertices(tri)
        self.V = V[np.isfinite(V).all((1, 2))].astype(np.float64)
        cen = self.V.mean(1)
        rad = np.sqrt(((self.V - cen[:, None]) ** 2).sum(-1)).max(1)
        I, K = [], []
        n, m = o.shape[0], self.V.shape[0]
        bc = max(1, CHUNK // max(1, m))
        for i0 in range(0, n, bc):
            s = slice(i0, min(n, i0 + bc))
            with np.errstate(all="ignore"):
                mc = cen[None] - self.o[s, None]
                along = np.maximum(_d(mc, self.dh[s, None]), 0.0)                   # the nearest point of the half-line
                g = mc - self.dh[s, None] * along[..., None]
                near = np.sqrt(_d(g, g)) <= (self.r[s, None] + slack) + rad[None]
            i, k = np.nonzero(near & self.alive[s, None])
            I.append(i + i0), K.append(k)
        self.i, self.k, self.n = np.concatenate(I), np.concatenate(K), n
        self._cast = {}

    def _reduce(self, f):
        out = np.full(self.n, np.inf)
        for p0 in range(0, self.i.size, CHUNK):
            i, k = self.i[p0:p0 + CHUNK], self.k[p0:p0 + CHUNK]
            np.minimum.at(out, i, f(i, self.V[k, 0], self.V[k, 1], self.V[k, 2]))
        return out

    def cast(self, dr=0.0):
        """float64 t [n] (units of d; inf for none) of the sphere of radius max(r + dr, 0)"""
        if dr not in self._cast:
            s = self._reduce(lambda i, a, b, c: cast_pairs(self.o[i], self.dh[i], np.maximum(self.r[i] + dr, 0.0), a, b, c))
            with np.errstate(all="ignore"):
                self._cast[dr] = np.where(self.alive, s / self.len, np.inf)
        return self._cast[dr]

    def dist(self, t):
        """float64 distance of the mesh (of the kept triangles: exact below r + slack) from o + d t"""
        with np.errstate(all="ignore"):
            p = self.o + self.dh * (np.where(np.isfinite(t), t, 0.0) * self.len)[:, None]
        return self._reduce(lambda i, a, b, c: tri_dist(p[i], a, b, c))


_cache = {}


def case(name, bunny_small):
    if name not in _cache:
        tri, nodes, rays, radius = SS.host_case(name, bunny_small)
        size = extent(tri)
        touch = SE.touch(rays, radius, tri)
        pruned = SE.touch(rays, radius, tri, prune=True)               # what the device tests ask: the same answers
        assert np.array_equal(touch[0], pruned[0]) and np.array_equal(touch[1].view(np.uint32), pruned[1].view(np.uint32))
        want = SE.query(rays, radius, tri, touching=touch)
        with np.errstate(all="ignore"):
            _cache[name] = (tri, nodes, rays, radius, want, size, Truth(rays, radius, tri, 4 * TOL * size))
    return _cache[name]


# ---- the tests

@pytest.mark.parametrize("name", SS.NAMES)
def test_caps(bunny_small, name):
    tri, nodes, rays, radius, want, size, truth = case(name, bunny_small)
    c = SS.caps(want)
    print(name, rays.shape[0], c)
    assert 1900 <= rays.shape[0] <= 2500
    assert c["swept"] >= 0.10 and c["touching"] >= 0.10 and c["miss"] >= 0.10, c
    assert c["face"] >= 0.05 and c["edge"] >= 0.05 and c["vertex"] >= 0.05, c
    o, d, r = SE.split(rays, radius)
    assert (r == 0).sum() >= 50 and (r > 0.2 * size).sum() >= 50
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any()
    dead = ~SE.live(rays, radius)
    assert dead.sum() == SS.N_DEAD and (want[0][dead] == -1).all() and np.isposinf(want[1][dead]).all()


@pytest.mark.parametrize("name", SS.NAMES)
@np.errstate(all="ignore")
def test_truth_against_marching(bunny_small, name):
    """the float64 truth against closest_point_expected marched along the ray: contact at its t, none at 16 earlier times, and none
    along a missing ray"""
    tri, nodes, rays, radius, want, size, truth = case(name, bunny_small)
    t64 = truth.cast()
    o, d, r = SE.split(rays, radius)
    rng = np.random.default_rng(3)
    hit = rng.permutation(np.nonzero(np.isfinite(t64) & (t64 > 0))[0])[:12]
    miss = rng.permutation(np.nonzero(truth.alive & np.isinf(t64))[0])[:6]
    u = (np.arange(16) + rng.random(16)) / 16
    tt = np.concatenate([(t64[hit, None] * u[None]).ravel(), t64[hit], (4 * size / truth.len[miss, None] * u[None]).ravel()])
    q = np.concatenate([np.repeat(hit, 16), hit, np.repeat(miss, 16)])
    p = (o[q].astype(np.float64) + d[q].astype(np.float64) * tt[:, None]).astype(F)
    dist = E.closest_point(p, tri)[2].astype(np.float64)
    tol = 1e-5 * size + 1e-6 * np.abs(p).max(1)
    k = hit.size * 16
    assert (dist[:k] >= r[q[:k]] - tol[:k]).all()
    assert (np.abs(dist[k:k + hit.size] - r[hit]) <= tol[k:k + hit.size]).all()
    assert (dist[k + hit.size:] > r[q[k + hit.size:]] - tol[k + hit.size:]).all()
    assert hit.size == 12 and miss.size == 6


@pytest.mark.parametrize("name", SS.NAMES)
@np.errstate(all="ignore")
def test_residual_and_no_tunnelling(bunny_small, name):
    """where the restatement reports a swept contact the sphere touches the mesh there, to TOL of the extent; no earlier sampled
    position is deeper than that; and its t lies between the truth's for the radii r - TOL and r + TOL of the extent"""
    tri, nodes, rays, radius, want, size, truth = case(name, bunny_small)
    win, t, point, touching, sub = want
    swept = (win >= 0) & (touching == 0)
    t32 = t.astype(np.float64)
    res = np.abs(truth.dist(t32) - truth.r) / size
    print("%s: largest residual of %d swept answers %.3e of the extent %.4g (TOL %.3e)" % (name, swept.sum(), res[swept].max(), size, TOL))
    assert res[swept].max() <= TOL
    rng = np.random.default_rng(4)
    u = rng.random(len(t32))                                             # no tunnelling, sampled: one earlier time per query
    deep = (truth.r - truth.dist(t32 * u)) / size
    assert deep[swept].max() <= TOL, deep[swept].max()
    late, early = truth.cast(-TOL * size), truth.cast(TOL * size)
    with np.errstate(all="ignore"):
        big = truth.alive & (truth.r >= TOL * size)                    # (a sphere thinner than TOL may pass a crack a ray passes)
        assert (t32[big] <= late[big] * (1 + 1e-6)).all()               # never later than the smaller sphere: nothing was passed
        assert (early[truth.alive] <= t32[truth.alive] * (1 + 1e-6)).all()     # never earlier than the larger one
    # the contact point lies on the winner, at r from the centre
    V = SE.vertices(tri)[np.maximum(win, 0)].astype(np.float64)
    on = tri_dist(point.astype(np.float64), V[:, 0], V[:, 1], V[:, 2]) / size
    c = truth.o + truth.dh * (t32 * truth.len)[:, None]
    off = np.abs(np.sqrt(((c - point) ** 2).sum(1)) - truth.r) / size
    assert on[swept].max() <= TOL and off[swept].max() <= 2 * TOL, (on[swept].max(), off[swept].max())


@pytest.mark.parametrize("name", SS.NAMES)
@np.errstate(all="ignore")
def test_touching_is_closest_point(bunny_small, name):
    tri, nodes, rays, radius, want, size, truth = case(name, bunny_small)
    win, t, point, touching, sub = want
    o, d, r = SE.split(rays, radius)
    m = touching == 1
    alive = SE.live(rays, radius)
    some = np.nonzero(alive)[0][:300]                                   # closest_point as the caller would ask it
    cp = E.closest_point(o[some], tri, r[some])
    ms = m[some]
    assert m.sum() > 100 and ms.sum() > 20 and np.array_equal(ms, cp[0] >= 0)
    assert np.array_equal(win[some][ms], cp[0][ms]) and np.array_equal(point[some][ms].view(np.uint32), cp[1][ms].view(np.uint32))
    assert not t[m].any() and (sub[m] == -1).all() and not m[~alive].any()
    t64 = truth.cast()                                                  # ... and the truth agrees, away from dist = r
    far = alive & (np.abs(truth.dist(np.zeros(len(t))) - truth.r) > TOL * size)
    assert np.array_equal(m[far], (t64 == 0)[far])


def test_constructed_pairs():
    for leaf in (4, 8):
        tri, nodes, rays, radius, where = SS.constructed(leaf)
        win, t, point, touching, sub = SE.query(rays, radius, tri)
        for i, (name, o, d, r, hit, tt, x, touch, s) in enumerate(SS.CASES):
            assert (win[i] == where[i]) == hit and (win[i] >= 0) == hit, name
            assert touching[i] == touch and sub[i] == s, name
            assert np.array_equal(point[i], F(x) + F([SS.SPACING * i, 0, 0]) if hit else F([0, 0, 0])), name
            if tt is not None:
                assert t[i] == F(tt), name
        i = [c[0] for c in SS.CASES].index("one ulp clear, moving inward")
        assert 0 <= t[i] <= 2.0 ** -22 and touching[i] == 0


def test_t_max_and_at(bunny_small):
    tri, nodes, rays, radius, want, size, truth = case("voxel_solid", bunny_small)
    n = rays.shape[0]
    table, touch = SE.swept_all(rays, radius, tri), SE.touch(rays, radius, tri)
    own = want[1]
    k = np.arange(n) % 5
    t_max = np.select([k == 0, k == 1, k == 2, k == 3], [own, np.nextafter(own, F(-np.inf)), np.nextafter(own, F(np.inf)), np.full(n, np.nan, F)],
                      np.full(n, -1.0, F)).astype(F)
    got = SE.query(rays, radius, tri, t_max, table=table, touching=touch)
    swept = (want[0] >= 0) & (want[3] == 0)
    assert np.array_equal(got[0][want[3] == 1], want[0][want[3] == 1])           # touching does not look at t_max
    assert np.array_equal(got[0][swept & (k == 0)], want[0][swept & (k == 0)]) and np.array_equal(got[0][swept & (k == 2)], want[0][swept & (k == 2)])
    below = swept & (k == 1) & (own > 0)
    assert below.sum() > 50 and (got[1][below] > own[below]).all()
    assert (got[0][swept & (k >= 3)] == -1).all()
    a = SE.at(rays, radius, tri, want[0])                                # the pair rule on the winners reproduces them
    assert np.array_equal(a[0].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(a[2], want[3])


def _below(nodes):
    """the triangles below every node of a caller's tree, as index arrays"""
    out = [np.zeros(0, int)] * nodes.shape[0]
    for i in range(nodes.shape[0] - 1, 0, -1):
        n, index = int(nodes[i, 3]), int(nodes[i, 4])
        out[i] = np.arange(index, index + n) if n > 0 else np.concatenate([out[int(nodes[i, 0])], out[int(nodes[i, 1])]])
    return out


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_box_bound_below_every_pair(name):
    """on the bits: tnear of every node box above a triangle <= the pair's t, and the box passes the gate whenever the pair does --
    what lets the walk prune with no margin"""
    tri, nodes, expect = T.shape(name)
    facts = T.check_valid(tri, nodes)
    rays, radius = SS.shape_queries(tri, expect, T.SEEDS[name])
    cand, t, sub, gate, tnear = SE.swept_all(rays, radius, tri)
    assert cand.sum() > 100 or tri.shape[0] <= 8
    assert (tnear[cand] <= t[cand]).all()
    if not (facts["nested"] and facts["holds"]):
        assert not expect["walk"]
        return
    o, d, r = SE.split(rays, radius)
    below = _below(nodes)
    checked = 0

    def check(k, lo, hi, what):
        ok, tn = SE.slab(o, d, r, lo[None], hi[None])
        lb = np.where(ok, tn, F(np.inf))
        assert (lb[:, None] <= t[:, k])[cand[:, k]].all(), what
        assert ok[gate[:, k].any(1)].all() and (tn[:, None] <= tnear[:, k])[gate[:, k]].all(), what
        return int(cand[:, k].sum())

    for i in range(1, nodes.shape[0]):                                  # the root's box included
        k = below[i]
        if not k.size:
            continue
        checked += check(k, nodes[i, 6:9], nodes[i, 9:12], i)
        if nodes[i, 3] == 0:                                            # ... and boxes that are no node's: the union of the two children's
            l, rgt = int(nodes[i, 0]), int(nodes[i, 1])                 # (a 4-wide record's slot is a node box or such a union of boxes below it)
            check(k, np.minimum(nodes[l, 6:9], nodes[rgt, 6:9]), np.maximum(nodes[l, 9:12], nodes[rgt, 9:12]), ("union", i))
            for c in (l, rgt):                                          # the union of a child's box with a grandchild's of the other side
                if nodes[c, 3] == 0:
                    g = int(nodes[c, 0])
                    other = rgt if c == l else l
                    kk = np.concatenate([below[g], below[other]])
                    check(kk, np.minimum(nodes[g, 6:9], nodes[other, 6:9]), np.maximum(nodes[g, 9:12], nodes[other, 9:12]), ("slot", i))
    assert checked > 0 or nodes.shape[0] <= 2

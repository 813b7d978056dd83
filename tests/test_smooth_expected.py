"""tests/smooth_expected.py, the numpy restatement of include/ezrt_smooth.h (rules U1 to U9), held to the properties the header states.
Needs no GPU and no library: numpy, tests/topology_expected.py and tests/weld_expected.py for the arrays the call reads.

* the octahedron under the plain umbrella operator halves its radius every step, exactly;
* the flat power-of-two lattice with a pinned border is a fixed point on the bits for any steps and weights; without the pin the
  straight borders stay and the corners of the lattice and of its holes move;
* shape, summary, materials, face normals; reversed windings give the same points; steps compose;
* kept vertices, dead rows and corrupted arrays: nothing raises, untouched corners keep their bits;
* six Taubin steps on marching tetrahedra's spheres keep every vertex distinct and lengthen the shortest edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_expected as SM  # noqa: E402
import smooth_scenes as MS  # noqa: E402
import topology_expected as TE  # noqa: E402
import weld_expected as WE  # noqa: E402

F = np.float32
_cache = {}


def _arrays(name):
    if name not in _cache:
        R = MS.rows(name)
        _cache[name] = (TE.topology(R), WE.weld(R))
    return _cache[name]


def _run(name, **kw):
    return SM.smooth_of(MS.rows(name), *_arrays(name), **kw)


def _pos(out):
    return out[:, :9].reshape(-1, 3)


@pytest.mark.parametrize("name", MS.NAMES)
def test_shape_summary_materials_normals(name):
    R = MS.rows(name)
    n = R.shape[0]
    for kw in (dict(steps=1), dict(steps=4, lam=0.5, mu=-0.53), dict(steps=3, flags=SM.PIN_BORDER)):
        out, sm, rule, X = _run(name, **kw)
        assert out.shape == (n, 36) and out.dtype == F and X.shape == (3 * n, 3)
        assert sm[0] == n and sm[1] + sm[2] + sm[3] == 3 * n and sm[5] == kw["steps"] and sm[6] == kw.get("flags", 0) and sm[7] == 0
        assert sm[1] == (rule == SM.SMOOTH).sum() and sm[2] == (rule == SM.BORDER).sum() and 0 <= sm[4] <= 3 * n
        assert np.array_equal(SM.bits(out[:, 18:]), SM.bits(R[:, 18:]))       # U1: the material on the bits
        assert SM.same_rows(out[:, 9:18], np.tile(WE.face_normals(out), (1, 3)))
        kept = rule == SM.KEPT
        assert np.array_equal(SM.bits(_pos(out)[kept]), SM.bits(_pos(R)[kept]))   # U8: their own bits
        if kw.get("flags"):
            assert sm[2] == 0
    topo, weld = _arrays(name)
    assert _run(name)[1][4] <= int(weld.summary[1])


def test_the_octahedron_halves_exactly():
    R = MS.rows("octa")
    for j in range(1, 9):
        out, sm, rule, X = _run("octa", steps=j, lam=0.5)
        assert sm.tolist() == [8, 24, 0, 0, 6, j, 0, 0]
        P, Q = _pos(R), _pos(out)
        assert np.array_equal(SM.bits(Q), SM.bits(P * F(2.0 ** -j)))         # +-2 on an axis becomes +-2^(1 - j), every 0 stays +0
        assert set(np.abs(Q).max(axis=1).tolist()) == {2.0 ** (1 - j)}


@pytest.mark.parametrize("kw", (dict(steps=1), dict(steps=2, lam=0.5, mu=-0.53), dict(steps=9, lam=0.25, mu=0.75), dict(steps=64, lam=1.0, mu=-1.0)))
def test_the_pinned_flat_lattice_is_a_fixed_point(kw):
    R = MS.rows("grid_pow2")
    out, sm, rule, X = _run("grid_pow2", flags=SM.PIN_BORDER, **kw)
    assert sm[1] > 100 and sm[2] == 0 and sm[3] > 50
    assert np.array_equal(SM.bits(out[:, :9]), SM.bits(R[:, :9])) and np.array_equal(SM.bits(out[:, 18:]), SM.bits(R[:, 18:]))
    topo, weld = _arrays("grid_pow2")
    assert set(int(weld.star_offsets[v + 1] - weld.star_offsets[v]) for v in np.unique(weld.vertex[rule == SM.SMOOTH])) == {6}


def test_the_free_flat_lattice_moves_its_corners_only():
    R = MS.rows("grid_pow2")
    n = R.shape[0]
    topo, weld = _arrays("grid_pow2")
    out, sm, rule, X = _run("grid_pow2", steps=1, lam=0.5)
    assert sm[3] == 0 and sm[2] > 50 and sm[1] > 100
    P, Q = _pos(R), _pos(out)
    moved = (SM.bits(P) != SM.bits(Q)).any(axis=1)
    assert not moved[rule == SM.SMOOTH].any() and moved[rule == SM.BORDER].any()
    on_side = ((P[:, 0] == 0) | (P[:, 0] == 2)) ^ ((P[:, 1] == 0) | (P[:, 1] == 4))   # on one side of the lattice, not at its corners
    assert on_side.sum() > 40 and not moved[on_side].any()
    # the four corners of the lattice, four of the single missing cell and four of the pair of missing cells
    assert len(set(np.asarray(weld.vertex).reshape(-1)[moved].tolist())) == 12
    assert (Q[:, 2] == 0).all()


@pytest.mark.parametrize("name", ("tetra", "cube_pow2", "disc300", "moebius", "grid_pow2", "bunny"))
def test_reversed_windings_give_the_same_points(name):
    R = MS.rows(name)
    Rv = MS.reverse_rows(R)
    for kw in (dict(steps=1), dict(steps=5, lam=0.5, mu=-0.53)):
        out, sm = _run(name, **kw)[:2]
        rev, smv = SM.smooth_of(Rv, TE.topology(Rv), WE.weld(Rv), **kw)[:2]
        assert np.array_equal(sm, smv)
        a, b = out[:, :9].reshape(-1, 3, 3), rev[:, :9].reshape(-1, 3, 3)
        assert SM.same_rows(b[:, [0, 2, 1]], a), (name, kw)


@pytest.mark.parametrize("name", ("cube_pow2", "disc300", "grid_pow2", "bunny", "pinched"))
def test_steps_compose_after_an_even_count(name):
    topo, weld = _arrays(name)
    lam, mu = SM.TAUBIN
    for a, b in ((2, 1), (2, 3), (4, 2)):
        whole = _run(name, steps=a + b, lam=lam, mu=mu)
        first = _run(name, steps=a, lam=lam, mu=mu)
        then = SM.smooth_of(first[0], topo, weld, steps=b, lam=lam, mu=mu)   # the arrays still describe the rows, by value
        assert SM.same_rows(then[0], whole[0]) and np.array_equal(then[1][:5], whole[1][:5])
    odd = SM.smooth_of(_run(name, steps=1, lam=lam, mu=mu)[0], topo, weld, steps=1, lam=lam, mu=mu)
    assert not SM.same_rows(odd[0], _run(name, steps=2, lam=lam, mu=mu)[0])  # (an odd count leaves the next call the wrong weight)


def test_kept_vertices_do_not_move():
    for name, at in (("book5", ((0, 0, 0), (0, 0, 1))), ("pinched", ((0, 0, 0),))):
        R = MS.rows(name)
        out, sm, rule, X = _run(name, steps=3, lam=0.5, mu=-0.53)
        P = _pos(R)
        kept = np.zeros(P.shape[0], bool)
        for p in at:
            kept |= (P == F(p)).all(axis=1)
        assert kept.sum() >= 4 and (rule[kept] == SM.KEPT).all() and (rule[~kept] != SM.KEPT).all() and sm[3] == kept.sum()
        assert np.array_equal(SM.bits(_pos(out)[kept]), SM.bits(P[kept])) and sm[4] * 3 > sm[1] + sm[2] > 0


def test_dead_rows_propagate():
    R = MS.rows("dead")
    topo, weld = _arrays("dead")
    out, sm, rule, X = _run("dead", steps=2)
    dead = np.repeat(~topo.live, 3)
    assert (rule[dead] == SM.KEPT).all() and SM.same_rows(_pos(out)[dead], _pos(R)[dead]) and np.isnan(out[:, 9:18]).any()


def test_corrupted_arrays_fall_back():
    R = MS.rows("bunny")
    n = R.shape[0]
    H = 3 * n
    topo, weld = _arrays("bunny")
    P = _pos(R)
    good = SM.smooth_of(R, topo, weld, steps=3, lam=0.5, mu=-0.53)
    rng = np.random.default_rng(MS.SEED + 41)
    bad_values = np.array([-1, -2, H, H + 1, 2 ** 31 - 1, -2 ** 31])

    def run(**kw):
        a = dict(edge_class=topo.edge_class, vertex=np.asarray(weld.vertex).reshape(-1), star_offsets=weld.star_offsets, star=weld.star,
                 vert_flags=weld.vert_flags)
        a.update(kw)
        return SM.smooth(R, steps=3, lam=0.5, mu=-0.53, **a)

    hit = rng.permutation(H)[:H // 4]
    # vertex: -1 and out of range -- the corner keeps its bits and is read by its neighbours at its stored position
    vertex = np.asarray(weld.vertex).reshape(-1).copy()
    vertex[hit] = rng.choice(bad_values, hit.size)
    out, sm, rule, X = run(vertex=vertex)
    assert (rule[hit] == SM.KEPT).all() and np.array_equal(SM.bits(_pos(out)[hit]), SM.bits(P[hit])) and sm[3] >= hit.size
    # offsets: an empty, a reversed, a negative and an overlong range each keep every corner of that vertex
    for lo_hi in ((5, 5), (9, 3), (-1, 4), (0, H + 1)):
        off = weld.star_offsets.copy()
        v = 17
        off[v], off[v + 1] = lo_hi
        out, sm, rule, X = run(star_offsets=off)
        mine = np.asarray(weld.vertex).reshape(-1) == v
        assert mine.any() and (rule[mine] == SM.KEPT).all() and np.array_equal(SM.bits(_pos(out)[mine]), SM.bits(P[mine]))
    # star: one entry out of range keeps its vertex
    star = weld.star.copy()
    at = rng.permutation(star.size)[:60]
    star[at] = rng.choice(bad_values, at.size)
    out, sm, rule, X = run(star=star)
    owners = np.searchsorted(weld.star_offsets[:int(weld.summary[1]) + 1], at, side="right") - 1
    mine = np.isin(np.asarray(weld.vertex).reshape(-1), owners)
    assert mine.any() and (rule[mine] == SM.KEPT).all() and np.array_equal(SM.bits(_pos(out)[mine]), SM.bits(P[mine]))
    assert sm[4] == good[1][4] - np.unique(owners).size
    # noise everywhere: nothing raises and the sums hold
    for seed in range(3):
        r = np.random.default_rng(MS.SEED + 50 + seed)
        out, sm, rule, X = run(vertex=r.integers(-5, H + 5, H), star_offsets=r.integers(-5, H + 5, H + 1), star=r.integers(-5, H + 5, H),
                               vert_flags=r.integers(0, 4, H), edge_class=r.integers(0, 5, H))
        assert sm[1] + sm[2] + sm[3] == H and np.array_equal(SM.bits(_pos(out)[rule == SM.KEPT]), SM.bits(P[rule == SM.KEPT]))
    # vert_flags and edge_class: a border flag on an interior vertex finds no BOUNDARY half-edge and keeps it
    vf = weld.vert_flags.copy()
    inner = np.unique(np.asarray(weld.vertex).reshape(-1)[good[2] == SM.SMOOTH])[:10]
    vf[inner] = 1
    out, sm, rule, X = run(vert_flags=vf)
    assert inner.size == 10 and sm[3] > good[1][3] and sm[1] < good[1][1] and sm[2] == good[1][2] and sm[4] == good[1][4]


@pytest.mark.parametrize("n", (9, 13))
def test_taubin_on_marching_tetrahedra(n):
    R = MS.iso_sphere(n)[2]
    topo, weld = TE.topology(R), WE.weld(R)
    assert TE.closed(topo) and TE.oriented(topo) and R.shape[0] > 500
    lam, mu = SM.TAUBIN
    out, sm, rule, X = SM.smooth_of(R, topo, weld, steps=6, lam=lam, mu=mu)
    assert sm[1] == 3 * R.shape[0] and sm[4] == int(weld.summary[1])
    assert SM.distinct_vertices(out) == SM.distinct_vertices(R) == int(weld.summary[1])
    assert SM.shortest_edge(out) > SM.shortest_edge(R)
    t2 = TE.topology(out)
    assert TE.closed(t2) and TE.oriented(t2) and np.isfinite(out).all()

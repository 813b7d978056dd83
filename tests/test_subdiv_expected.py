"""tests/subdiv_expected.py, the numpy restatement of include/ezrt_subdivide.h (rules S1 to S9), held to the properties the header
states.  Needs no GPU and no library: numpy, tests/topology_expected.py and tests/weld_expected.py for the arrays Loop mode reads, and
ezrt_amd/scenes.py: subdivide for what midpoint mode has to be on the bits.

* midpoint mode is scenes.subdivide on the bits (the Bunny), keeps normals at the corners and averages them along the edges;
* on the flat power-of-two lattice every smooth vertex and every straight border vertex stays where it is and every edge point is the
  midpoint, exactly;
* rotating rows rotates their output and changes no point; reversing every winding gives the same triangles reversed;
* on the closed scenes the output has 4 F triangles, 2 E + 3 F edges, V + E vertices, the same Euler characteristic and edge classes
  (and the restatement keeps the new points distinct there, which is the stated limit);
* Loop positions against an independently written float64 Loop on the indexed mesh, within one rounding per operation;
* the kept rules: book5's spine and the pinched apex do not move; garbage arrays fall back as S3, S4 and S7 say."""
import os
import sys

import numpy as np
import pytest

from ezrt_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_scenes as CS  # noqa: E402
import subdiv_expected as SE  # noqa: E402
import subdiv_scenes as SS  # noqa: E402
import topology_expected as TE  # noqa: E402
import weld_expected as WE  # noqa: E402

F = np.float32
_cache = {}


def _arrays(name):
    if name not in _cache:
        R = SS.rows(name)
        _cache[name] = (TE.topology(R), WE.weld(R))
    return _cache[name]


def _loop(name):
    key = ("loop", name)
    if key not in _cache:
        _cache[key] = SE.loop(SS.rows(name), *_arrays(name))
    return _cache[key]


def _points(out, n):
    """(P float32 [n, 3, 3], E float32 [n, 3, 3]) read back from the output rows by S1"""
    O = out[:, :9].reshape(n, 4, 3, 3)
    return np.stack([O[:, 0, 0], O[:, 1, 1], O[:, 2, 2]], 1), np.stack([O[:, 3, 0], O[:, 3, 1], O[:, 3, 2]], 1)


def _canon(tris):
    """every triangle [m, 3, 3] as the bytes of its three vertices, rotated to start at the least"""
    out = []
    for t in np.ascontiguousarray(tris, F):
        k = [p.tobytes() for p in t]
        i = k.index(min(k))
        out.append(tuple(k[i:] + k[:i]))
    return out


@pytest.mark.parametrize("name", SS.NAMES)
def test_shape_summary_materials(name):
    R = SS.rows(name)
    n = R.shape[0]
    for mode in (SE.MIDPOINT, SE.LOOP):
        out, sm, rule, interior = SE.subdivide(R, mode) if mode == SE.MIDPOINT else _loop(name)
        assert out.shape == (4 * n, 36) and out.dtype == F
        assert sm[0] == 4 * n and sm[1] + sm[2] + sm[3] == sm[4] + sm[5] == 3 * n and sm[6] == mode and sm[7] == 0
        assert np.array_equal(SE.bits(out[:, 18:].reshape(n, 4, 18)), SE.bits(np.repeat(R[:, None, 18:], 4, 1)))
        P, E = _points(out, n)
        O = out[:, :9].reshape(n, 4, 3, 3)
        for j, piece in enumerate(SE.PIECES):                                  # S1: the pieces share their points on the bits
            for m, pt in enumerate(piece):
                want = P[:, pt] if pt < 3 else E[:, pt - 3]
                assert SE.same_rows(O[:, j, m], want)
        if mode == SE.MIDPOINT:
            assert sm[3] == sm[5] == 3 * n and SE.same_rows(P, R[:, :9].reshape(n, 3, 3))
            Nn = R[:, 9:18].reshape(n, 3, 3)
            On = out[:, 9:18].reshape(n, 4, 3, 3)
            assert SE.same_rows(np.stack([On[:, 0, 0], On[:, 1, 1], On[:, 2, 2]], 1), Nn)
            with np.errstate(all="ignore"):
                assert SE.same_rows(On[:, 3], (Nn + Nn[:, [1, 2, 0]]) * F(0.5))
        else:
            assert SE.same_rows(out[:, 9:18], np.tile(WE.face_normals(out), (1, 3)))


def test_midpoint_is_scenes_subdivide_on_the_bits():
    v, f = scenes.mesh("bunny")
    R = CS.decorate(v[f], 1)
    nf = f.shape[0]
    out, sm, _, _ = SE.subdivide(R, SE.MIDPOINT)
    v1, f1 = scenes.subdivide(v, f, 1)
    want = v1[f1].reshape(4, nf, 9)                                            # face j * F + t
    assert np.array_equal(SE.bits(out[:, :9].reshape(nf, 4, 9)), SE.bits(np.ascontiguousarray(want.transpose(1, 0, 2))))


def test_the_flat_lattice_is_a_fixed_point():
    R = SS.rows("grid_pow2")
    n = R.shape[0]
    topo, weld = _arrays("grid_pow2")
    out, sm, rule, interior = _loop("grid_pow2")
    P, E = _points(out, n)
    V = R[:, :9].reshape(n, 3, 3)
    assert np.array_equal(SE.bits(E), SE.bits((V + V[:, [1, 2, 0]]) * F(0.5))) and sm[4] > 0 and sm[5] > 0
    smooth = (rule == SE.SMOOTH).reshape(n, 3)
    assert smooth.sum() > 100 and np.array_equal(P[smooth], V[smooth])
    assert set(int(weld.star_offsets[v + 1] - weld.star_offsets[v]) for v in np.unique(weld.vertex[rule == SE.SMOOTH])) == {6}
    # a border vertex whose two border neighbours are symmetric about it is on a straight border: it stays; the corners of the
    # holes and of the lattice move
    border = (rule == SE.BORDER).reshape(n, 3)
    moved = (SE.bits(P) != SE.bits(V)).any(axis=2)
    assert border.sum() > 50 and not moved[smooth].any() and moved[border].any() and not moved[border].all()
    assert not (rule == SE.KEEP).any()
    xy = V[border]
    on_side = ((xy[:, 0] == 0) | (xy[:, 0] == 2)) ^ ((xy[:, 1] == 0) | (xy[:, 1] == 4))   # on one side of the lattice, not at its corners
    assert on_side.sum() > 40 and not moved[border][on_side].any()


@pytest.mark.parametrize("name", ("tetra", "cube_pow2", "disc300", "moebius", "grid_pow2", "dead"))
def test_rotation_and_reversal(name):
    R = SS.rows(name)
    n = R.shape[0]
    k = np.arange(n) % 3
    Rr = CS.rotate_rows(R, k)
    Rv = SS.reverse_rows(R)
    for mode in (SE.MIDPOINT, SE.LOOP):
        run = (lambda T: SE.subdivide(T, mode)) if mode == SE.MIDPOINT else (lambda T: SE.loop(T, TE.topology(T), WE.weld(T)))
        out, sm = run(R)[:2]
        got, smr = run(Rr)[:2]
        assert np.array_equal(sm, smr)
        a, b = out[:, :9].reshape(n, 4, 3, 3), got[:, :9].reshape(n, 4, 3, 3)
        for t in range(n):
            for j in range(3):                                                 # vertex j of the rotated row was vertex j + k
                assert SE.same_rows(b[t, j], np.roll(a[t, (j + k[t]) % 3], -k[t], axis=0)), (name, mode, t, j)
            assert SE.same_rows(b[t, 3], np.roll(a[t, 3], -k[t], axis=0)), (name, mode, t)
        rev, smv = run(Rv)[:2]
        assert np.array_equal(sm, smv)
        c = rev[:, :9].reshape(n, 4, 3, 3)
        fin = np.isfinite(a).all(axis=(1, 2, 3))                               # (NaN rows: a NaN is not told from a NaN by its bytes)
        for t in np.nonzero(fin)[0]:
            assert sorted(_canon(c[t][:, [0, 2, 1]])) == sorted(_canon(a[t])), (name, mode, t)


@pytest.mark.parametrize("mode", (SE.MIDPOINT, SE.LOOP))
@pytest.mark.parametrize("name", SS.CLOSED)
def test_counts_on_closed_scenes(name, mode):
    R = SS.rows(name)
    topo, weld = _arrays(name)
    Fc, Ec, Vc = int(topo.summary[0]), int(topo.summary[1]), int(weld.summary[1])
    assert TE.closed(topo) and TE.oriented(topo) and Fc == R.shape[0] and 2 * Ec == 3 * Fc
    out = SE.subdivide(R, mode)[0] if mode == SE.MIDPOINT else _loop(name)[0]
    P, E = _points(out, Fc)
    pts = np.concatenate([P.reshape(-1, 3), E.reshape(-1, 3)])
    assert len({p.tobytes() for p in (pts + F(0.0))}) == Vc + Ec               # the stated limit: no two new points coincide (-0 as +0)
    t2, w2 = TE.topology(out), WE.weld(out)
    assert t2.summary[0] == 4 * Fc and t2.summary[1] == 2 * Ec + 3 * Fc and w2.summary[1] == Vc + Ec
    assert w2.summary[1] - t2.summary[1] + t2.summary[0] == Vc - Ec + Fc
    assert TE.closed(t2) and TE.oriented(t2) and t2.summary[6] == topo.summary[6] and not w2.vert_flags.any()


def test_the_moebius_band_keeps_its_flipped_edges():
    topo, weld = _arrays("moebius")
    out = _loop("moebius")[0]
    t2 = TE.topology(out)
    assert topo.summary[4] > 0 and t2.summary[4] == 2 * topo.summary[4] and t2.summary[2] == 2 * topo.summary[2] and t2.summary[5] == 0


def _loop64(V):
    """Loop's scheme with Warren's weights in float64 on the indexed mesh of triangles V [n, 3, 3]: (new vertex positions by index,
    index of every corner, neighbour sets, edge -> opposite vertices)"""
    ids, pos = {}, []
    faces = []
    for tri in V:
        f = []
        for p in tri:
            key = tuple(float(x) + 0.0 for x in p)
            if key not in ids:
                ids[key] = len(pos)
                pos.append(np.asarray(key, np.float64))
            f.append(ids[key])
        faces.append(f)
    nb, opp = {}, {}
    for a, b, c in faces:
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            nb.setdefault(x, set()).update((y, z))
            opp.setdefault(frozenset((x, y)), []).append(z)
    new = {}
    for v, ring in nb.items():
        k = len(ring)
        beta = 3.0 / 16.0 if k == 3 else 3.0 / (8.0 * k)
        new[v] = (1.0 - k * beta) * pos[v] + beta * sum(pos[w] for w in ring)
    return np.asarray(pos), np.asarray(faces), nb, opp, new


@pytest.mark.parametrize("name", ("tetra", "octa", "cube_pow2", "torus32", "disc300", "bunny"))
def test_loop_against_float64(name):
    R = SS.rows(name)
    n = R.shape[0]
    V = R[:, :9].reshape(n, 3, 3)
    out, sm, rule, interior = _loop(name)
    P, E = _points(out, n)
    pos, faces, nb, opp, new = _loop64(V)
    eps = 2.0 ** -23
    checked = 0
    for t in range(n):
        for k in range(3):
            v = faces[t, k]
            if rule[3 * t + k] == SE.SMOOTH:
                val = len(nb[v])
                M = max(np.abs(pos[v]).max(), max(np.abs(pos[w]).max() for w in nb[v]))
                assert np.abs(P[t, k].astype(np.float64) - new[v]).max() <= (2 * val + 4) * eps * M, (name, t, k, val)
                checked += 1
            a, b, c = faces[t, k], faces[t, (k + 1) % 3], faces[t, (k + 2) % 3]
            if interior[3 * t + k]:
                (d,) = [z for z in opp[frozenset((a, b))] if z != c] or [c]
                want = 0.375 * (pos[a] + pos[b]) + 0.125 * (pos[c] + pos[d])
                M = max(np.abs(pos[x]).max() for x in (a, b, c, d))
                assert np.abs(E[t, k].astype(np.float64) - want).max() <= 4 * eps * M, (name, t, k)
            else:
                assert np.array_equal(E[t, k], ((V[t, k] + V[t, (k + 1) % 3]) * F(0.5)))
    assert checked == sm[1] and (checked == 3 * n or name in ("disc300", "bunny"))
    if name == "disc300":
        assert sm[1] == 300 and sm[2] == 600 and sm[3] == 0 and max(len(r) for r in nb.values()) == 300


def test_kept_vertices_do_not_move():
    for name, at in (("book5", ((0, 0, 0), (0, 0, 1))), ("pinched", ((0, 0, 0),))):
        R = SS.rows(name)
        n = R.shape[0]
        V = R[:, :9].reshape(n, 3, 3)
        out, sm, rule, interior = _loop(name)
        P, E = _points(out, n)
        kept = np.zeros((n, 3), bool)
        for p in at:
            kept |= (V == F(p)).all(axis=2)
        assert kept.sum() >= 2 * len(at) * 2 and (rule.reshape(n, 3)[kept] == SE.KEEP).all()
        assert np.array_equal(SE.bits(P[kept]), SE.bits(V[kept]))
        assert (rule.reshape(n, 3)[~kept] != SE.KEEP).all() and sm[3] == kept.sum()
    # book5's spine is NONMANIFOLD: its edge points are midpoints
    R = SS.rows("book5")
    out, sm, rule, interior = _loop("book5")
    assert sm[4] == 0 and sm[5] == 15


def test_dead_rows_propagate():
    R = SS.rows("dead")
    n = R.shape[0]
    topo, weld = _arrays("dead")
    out, sm, rule, interior = _loop("dead")
    assert (rule.reshape(n, 3)[~topo.live] == SE.KEEP).all() and not interior.reshape(n, 3)[~topo.live].any()
    P, E = _points(out, n)
    V = R[:, :9].reshape(n, 3, 3)
    assert SE.same_rows(P[~topo.live], V[~topo.live]) and np.isnan(out[:, :9]).any()


def test_garbage_arrays_fall_back():
    R = SS.rows("torus32")[:600]
    n = R.shape[0]
    H = 3 * n
    V = R[:, :9].reshape(n, 3, 3)
    topo, weld = TE.topology(R), WE.weld(R)
    good = SE.loop(R, topo, weld)
    Pg, Eg = _points(good[0], n)
    mid = (V + V[:, [1, 2, 0]]) * F(0.5)
    rng = np.random.default_rng(SS.SEED + 41)
    bad_values = np.array([-1, -2, H, H + 1, 2 ** 31 - 1, -2 ** 31])

    def run(**kw):
        a = dict(twin=topo.twin, edge_class=topo.edge_class, vertex=weld.vertex, star_offsets=weld.star_offsets, star=weld.star,
                 vert_flags=weld.vert_flags)
        a.update(kw)
        out, sm, rule, interior = SE.subdivide(R, SE.LOOP, **a)
        return _points(out, n) + (sm, rule, interior)

    # twin: out of range, its own triangle, a half-edge of another edge
    twin = topo.twin.copy()
    hit = rng.permutation(H)[:H // 4]
    twin[hit[:100]] = rng.choice(bad_values, 100)
    twin[hit[100:200]] = hit[100:200] // 3 * 3 + (hit[100:200] + 1) % 3
    twin[hit[200:]] = (topo.twin[hit[200:]] + 3 * 7) % H
    P, E, sm, rule, interior = run(twin=twin)
    was = good[3][hit]
    assert was.sum() > 50 and not interior[hit][was].any() and np.array_equal(SE.bits(E.reshape(H, 3)[hit]), SE.bits(mid.reshape(H, 3)[hit]))
    rest = np.ones(H, bool)
    rest[hit] = False
    assert np.array_equal(SE.bits(E.reshape(H, 3)[rest]), SE.bits(Eg.reshape(H, 3)[rest])) and np.array_equal(SE.bits(P), SE.bits(Pg))
    # vertex: -1 and out of range
    vertex = weld.vertex.copy()
    vertex[hit] = rng.choice(bad_values, hit.size)
    P, E, sm, rule, interior = run(vertex=vertex)
    assert (rule[hit] == SE.KEEP).all() and np.array_equal(SE.bits(P.reshape(H, 3)[hit]), SE.bits(V.reshape(H, 3)[hit]))
    assert np.array_equal(SE.bits(P.reshape(H, 3)[rest]), SE.bits(Pg.reshape(H, 3)[rest])) and sm[3] == good[1][3] + (good[2][hit] != SE.KEEP).sum()
    # offsets: an empty, a reversed, a negative and an overlong range each keep every corner of that vertex
    Vn = int(weld.summary[1])
    for lo_hi in ((5, 5), (9, 3), (-1, 4), (0, H + 1)):
        off = weld.star_offsets.copy()
        v = 17
        off[v], off[v + 1] = lo_hi
        P, E, sm, rule, interior = run(star_offsets=off)
        mine = weld.vertex == v
        assert mine.any() and (rule[mine] == SE.KEEP).all() and np.array_equal(SE.bits(P.reshape(H, 3)[mine]), SE.bits(V.reshape(H, 3)[mine]))
    assert Vn > 18
    # star: one entry out of range keeps its vertex
    star = weld.star.copy()
    at = rng.permutation(star.size)[:60]
    star[at] = rng.choice(bad_values, at.size)
    P, E, sm, rule, interior = run(star=star)
    owners = np.searchsorted(weld.star_offsets, at, side="right") - 1
    mine = np.isin(weld.vertex, owners)
    assert (rule[mine] == SE.KEEP).all() and np.array_equal(SE.bits(P.reshape(H, 3)[mine]), SE.bits(V.reshape(H, 3)[mine]))
    assert np.array_equal(SE.bits(P.reshape(H, 3)[~mine]), SE.bits(Pg.reshape(H, 3)[~mine]))

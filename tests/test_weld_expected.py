"""tests/weld_expected.py, the restatement of include/ezrt_vertices.h, held to what the header states -- no GPU.

* W2, W3: vert_corner is ascending with vertex[vert_corner[v]] == v, the stars partition the live corners, each ascending;
* W4: m(v, w) from the stars equals the multiplicity that tests/topology_expected.py gives the edge, on every scene;
* W5 to W7: the fans and flags the hand-built scenes are built for, V - E + F;
* reversing windings and permuting ids behave as the header says;
* N1 to N3: the PIN against the host's readObj(..., smoothNormal=True): on the bunny, the sphere and the subdivided sphere, with the
  transforms ezrt_amd/scenes.py uses and the triangles in the OBJ's order, the restatement's normals equal floats 9-17 of the
  encoded rows on the bits at every corner; on the cube stored with 24 vertex lines they differ, as documented;
* N4: weld arrays that are not usable give the face normal."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topology_expected as TE  # noqa: E402
import topology_scenes as TS  # noqa: E402
import weld_expected as WE  # noqa: E402
import weld_scenes as WS  # noqa: E402

_weld = {}


def _w(name, bunny_small=None):
    if name not in _weld:
        _weld[name] = WE.weld(WS.triangles(name, bunny_small))
    return _weld[name]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", WS.CPU_NAMES)
def test_vertices_and_stars(bunny_small, name):
    V = WS.triangles(name, bunny_small)
    w = _w(name, bunny_small)
    n = V.shape[0]
    nv = w.vert_corner.size
    L = int(w.live.sum()) * 3
    assert list(w.summary[:2]) == [L, nv] and w.summary[6] == 0 and w.summary[7] == 0
    # W1: -1 exactly on the corners of the triangles that take no part
    assert np.array_equal(w.vertex < 0, np.repeat(~w.live, 3)) and (w.vertex[w.vertex < 0] == -1).all() and w.vertex.max(initial=-1) == nv - 1
    # W2
    assert (np.diff(w.vert_corner) > 0).all() and np.array_equal(w.vertex[w.vert_corner], np.arange(nv))
    first = {}
    for c in np.nonzero(w.vertex >= 0)[0]:
        first.setdefault(int(w.vertex[c]), int(c))
    assert [first[v] for v in range(nv)] == list(w.vert_corner)
    # W3: a partition of the live corners, every star ascending and of one vertex
    assert w.star_offsets[0] == 0 and w.star_offsets[-1] == L == w.star.size and (np.diff(w.star_offsets) >= 1).all()
    assert np.array_equal(np.sort(w.star), np.nonzero(w.vertex >= 0)[0])
    assert np.array_equal(w.vertex[w.star], np.repeat(np.arange(nv), np.diff(w.star_offsets)))
    inner = np.ones(L, bool)
    inner[w.star_offsets[:-1]] = False
    assert (np.diff(w.star)[inner[1:]] > 0).all()
    assert w.summary[2] == (np.diff(w.star_offsets).max() if nv else 0)
    # equal ids exactly where the keys are equal
    K, _ = TE.keys(V)
    ids = {}
    for c in np.nonzero(w.vertex >= 0)[0]:
        assert ids.setdefault(K[c // 3][c % 3], int(w.vertex[c])) == w.vertex[c]
    assert len(ids) == nv and len(set(ids.values())) == nv
    assert n == w.live.size


@pytest.mark.parametrize("name", TS.CPU_NAMES + WS.HAND)
def test_m_is_the_topology_multiplicity(bunny_small, name):
    V = WS.triangles(name, bunny_small)
    w, t = _w(name, bunny_small), TE.topology(V, components=False)
    m = WE.edge_mult(w)
    want = {}
    for h in np.nonzero(t.mult > 0)[0]:
        a, b = int(w.vertex[h]), int(w.vertex[h // 3 * 3 + (h % 3 + 1) % 3])
        want[(a, b)] = want[(b, a)] = int(t.mult[h])
    assert dict(m) == want
    # W6 from W4, and the topology's view of the same facts: a vertex is on the border exactly when a BOUNDARY edge ends there
    border = np.zeros(w.vert_corner.size, bool)
    multi = np.zeros(w.vert_corner.size, bool)
    for (a, _), k in want.items():
        border[a] |= k == 1
        multi[a] |= k >= 3
    assert np.array_equal(w.vert_flags & 1 != 0, border) and np.array_equal(w.vert_flags & 2 != 0, multi)
    assert np.array_equal(w.vert_flags & 4 != 0, w.fans > 1) and (w.fans >= 1).all()
    assert list(w.summary[3:6]) == [border.sum(), multi.sum(), (w.fans > 1).sum()]


def _euler(name):
    w, t = _w(name), TE.topology(WS.triangles(name), components=False)
    return int(w.summary[1] - t.summary[1] + t.summary[0])


def test_the_hand_built_scenes_have_their_fans_and_flags():
    w = _w("bowtie_vertex")
    assert list(w.summary) == [24, 7, 6, 0, 0, 1, 0, 0] and list(w.fans) == [2, 1, 1, 1, 1, 1, 1] and list(w.vert_flags) == [4, 0, 0, 0, 0, 0, 0]
    assert TE.closed(TE.topology(WS.triangles("bowtie_vertex")))               # ... which the topology alone calls two clean closed parts
    w = _w("bowtie_edge")
    assert w.summary[1] == 6 and w.summary[4] == 2 and (w.vert_flags & 2 != 0).sum() == 2 and w.summary[3] == 0
    assert list(w.fans[w.vert_flags & 2 != 0]) == [1, 1]                       # the two cones are linked through the shared edge
    w = _w("tetra")
    assert list(w.summary) == [12, 4, 3, 0, 0, 0, 0, 0] and not w.vert_flags.any() and (w.fans == 1).all() and _euler("tetra") == 2
    w = _w("torus")
    assert _euler("torus") == 0 and w.summary[1] == 4096 and w.summary[2] == 6 and not w.vert_flags.any()
    assert _euler("bowtie_vertex") == 3                                         # two spheres less the vertex they share
    w = _w("moebius")
    assert (w.vert_flags == 1).all() and (w.fans == 1).all() and _euler("moebius") == 0
    w = _w("signed_zero")
    assert w.summary[1] == 4 and w.vertex[0] == w.vertex[4] and w.vertex[1] == w.vertex[3]   # +0 welds with -0
    w = _w("dead")
    assert np.array_equal(np.nonzero(w.vertex.reshape(-1, 3)[:, 0] < 0)[0], TS.DEAD_IDS) and w.vertex[3 * TS.SLIVER_ID] >= 0
    w = _w("disc300")
    assert list(w.summary) == [900, 301, 300, 300, 0, 0, 0, 0] and sorted(np.diff(w.star_offsets))[-2:] == [2, 300]
    w = _w("two_discs")
    assert list(w.summary) == [1800, 601, 600, 600, 0, 1, 0, 0] and w.fans.max() == 2 and np.diff(w.star_offsets)[w.fans == 2] == [600]
    w = _w("dup200")
    assert list(w.summary) == [600, 3, 200, 0, 3, 0, 0, 0] and list(w.fans) == [1, 1, 1]


@pytest.mark.parametrize("name", ("tetra_flip", "bowtie_vertex", "book5", "dead", "moebius", "open_solid", "disc300"))
def test_reversing_windings_changes_nothing(bunny_small, name):
    V = WS.triangles(name, bunny_small)
    w = _w(name, bunny_small)
    R = np.ascontiguousarray(V[:, [0, 2, 1]])                                  # corner 0 stays, corners 1 and 2 swap: a and b swap
    r = WE.weld(R)
    swap = np.arange(3 * V.shape[0]).reshape(-1, 3)[:, [0, 2, 1]].ravel()
    # the same vertices under the corner renaming; numbers follow the lowest corner, so compare as partitions and per key
    assert list(r.summary) == list(w.summary)
    part = lambda x, ren: sorted(sorted(int(ren[c]) for c in x.star[x.star_offsets[v]:x.star_offsets[v + 1]]) for v in range(x.vert_corner.size))
    assert part(r, swap) == part(w, np.arange(swap.size))
    per_key = lambda x, ren: sorted((min(int(ren[c]) for c in x.star[x.star_offsets[v]:x.star_offsets[v + 1]]), int(x.fans[v]), int(x.vert_flags[v]))
                                    for v in range(x.vert_corner.size))
    assert per_key(r, swap) == per_key(w, np.arange(swap.size))
    # reversing by (p3, p2, p1) as well
    assert list(WE.weld(np.ascontiguousarray(V[:, ::-1])).summary) == list(w.summary)


@pytest.mark.parametrize("name", ("bowtie_edge", "dead", "nasty", "two_discs"))
def test_a_permutation_of_the_ids_keeps_every_key(bunny_small, name):
    V = WS.triangles(name, bunny_small)
    w = _w(name, bunny_small)
    perm = np.random.default_rng(WS.SEED + 5).permutation(V.shape[0])
    p = WE.weld(np.ascontiguousarray(V[perm]))
    assert list(p.summary) == list(w.summary)
    K, _ = TE.keys(V)
    Kp, _ = TE.keys(V[perm])
    by_key = lambda x, keys: sorted((keys[x.vert_corner[v] // 3][x.vert_corner[v] % 3], int(x.star_offsets[v + 1] - x.star_offsets[v]),
                                     int(x.fans[v]), int(x.vert_flags[v])) for v in range(x.vert_corner.size))
    assert by_key(p, Kp) == by_key(w, K)


def test_the_rule_for_pairs():
    V = WS.triangles("dead")
    w = _w("dead")
    H = 3 * V.shape[0]
    a, b = np.meshgrid(np.arange(-1, H + 1), np.arange(-1, H + 1), indexing="ij")
    same = WE.at(V, a.ravel(), b.ravel()).reshape(a.shape)
    va = np.concatenate([[-1], w.vertex, [-1]])
    want = np.where((va[:, None] < 0) | (va[None, :] < 0), -1, (va[:, None] == va[None, :]).astype(np.int8))
    assert np.array_equal(same, want)


# ---- the normals

@pytest.mark.parametrize("name", WS.OBJ)
def test_the_normals_are_readobj_s_on_the_bits(name):
    """THE PIN: the host's readObj with smoothNormal=True, every corner, no tolerance"""
    T, lines, distinct = WS.read_obj(name)
    assert lines == distinct                                                   # the OBJ's vertex lines are distinct by value
    w = _w(name)
    assert w.live.all() and w.vert_corner.size <= lines
    got = WE.normals(T, w.vertex, w.star_offsets, w.star)
    assert got.dtype == np.float32 and got.shape == (T.shape[0], 9)
    same = (bits(got) == bits(T[:, 9:18])).reshape(-1, 3).all(1)
    assert same.all(), "%s: %d of %d corners equal on the bits" % (name, int(same.sum()), same.size)
    assert same.size == {"obj_bunny": 14904, "obj_sphere": 960, "obj_sphere2": 61440}[name]


def test_the_cube_with_duplicated_vertex_lines_differs_as_documented():
    T, lines, distinct = WS.read_obj("quad_cube")
    assert (lines, distinct) == (24, 8)
    w = _w("quad_cube")
    assert w.vert_corner.size == 8 and list(w.summary[:2]) == [36, 8] and not w.vert_flags.any()
    got = WE.normals(T, w.vertex, w.star_offsets, w.star)
    # readObj keeps 24 vertices: every corner has the normal of its own face; here a corner of the cube is ONE vertex of three faces
    fn = np.repeat(WE.face_normals(T), 3, axis=0)
    assert np.array_equal(T[:, 9:18].reshape(-1, 3), fn)                       # (by value: the sum from +0 turns a -0 into +0)
    assert (np.abs(got.reshape(-1, 3) - fn).max(1) > 0.1).all()


def test_not_usable_weld_arrays_give_the_face_normal():
    """N4"""
    T = np.array(WS.rows("obj_sphere")[:64])
    n, H = 64, 192
    w = WE.weld(T)
    fn = np.repeat(WE.face_normals(T), 3, axis=0).reshape(n, 9)
    good = WE.normals(T, w.vertex, w.star_offsets, w.star)
    assert (bits(good) != bits(fn)).any()
    full = lambda x, size: np.concatenate([x, np.zeros(size - x.size, np.int32)])
    vertex, off, star = w.vertex.copy(), full(w.star_offsets, H + 1), full(w.star, H)
    for bad_vertex in (-1, -2, H, 2 ** 31 - 1, -2 ** 31):
        assert np.array_equal(bits(WE.normals(T, np.full(H, bad_vertex, np.int32), off, star)), bits(fn)), bad_vertex
    seen = 0
    for bad_off in (off[::-1].copy(), np.full(H + 1, -1, np.int32), np.full(H + 1, 2 ** 31 - 1, np.int32), np.arange(H + 1, 0, -1, dtype=np.int32),
                    np.arange(H + 1, dtype=np.int32) + 1):
        got = WE.normals(T, vertex, bad_off, star)
        lo, hi = bad_off[vertex], bad_off[vertex + 1]
        unusable = ~((lo >= 0) & (lo <= hi) & (hi <= H))
        assert np.array_equal(bits(got).reshape(-1, 3)[unusable], bits(fn).reshape(-1, 3)[unusable])
        seen += int(unusable.all())
    assert seen >= 3
    for bad_star in (-1, H, 2 ** 31 - 1, -2 ** 31):
        assert np.array_equal(bits(WE.normals(T, vertex, off, np.full(H, bad_star, np.int32))), bits(fn)), bad_star
    # one bad entry spoils exactly the corners of its vertex
    star2 = star.copy()
    star2[off[5]] = H
    got = WE.normals(T, vertex, off, star2)
    spoiled = (vertex == 5).repeat(3).reshape(n, 9)
    assert np.array_equal(bits(got)[spoiled], bits(fn)[spoiled]) and np.array_equal(bits(got)[~spoiled], bits(good)[~spoiled])


def test_a_live_sliver_poisons_its_vertices():
    T = TS.tri36(TS.triangles("dead"))
    w = _w("dead")
    got = WE.normals(T, w.vertex, w.star_offsets, w.star).reshape(-1, 3)
    sliver = [int(w.vertex[3 * TS.SLIVER_ID + k]) for k in range(3)]
    poisoned = np.isin(w.vertex, sliver)
    assert np.isnan(got[poisoned]).all() and poisoned.sum() > 3
    clean = (w.vertex >= 0) & ~poisoned
    assert np.isfinite(got[clean]).all() and clean.any()
    # a corner of a triangle that takes no part gets the face normal of its own triangle, whatever that is
    fn = np.repeat(WE.face_normals(T), 3, axis=0)
    assert np.array_equal(bits(got[w.vertex < 0]), bits(fn[w.vertex < 0]))

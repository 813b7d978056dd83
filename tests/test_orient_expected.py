"""The host restatement of the mesh orientation (tests/orient_expected.py) held to what include/ezrt_orient.h states, on every case of
tests/orient_scenes.py, with the topology of tests/topology_expected.py.  Needs no GPU and no library: this is where every fixture is
shown to behave as the device tests assume."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_expected as OE  # noqa: E402
import orient_scenes as OS  # noqa: E402
import topology_expected as TE  # noqa: E402

_cache = {}


def _topo(V):
    t = TE.topology(V, components=True)
    return t


def _case(name, bunny_small):
    """(vertices, topology, orient with outward 0, with outward 1), computed once"""
    if name not in _cache:
        V = OS.triangles(name, bunny_small)
        t = _topo(V)
        _cache[name] = (V, t, OE.orient(V, t.twin, t.edge_class, False), OE.orient(V, t.twin, t.edge_class, True))
    return _cache[name]


def _oriented_set(V):
    """the multiset of oriented triangles: every triangle as its vertex keys rotated to start at the smallest"""
    K, _ = TE.keys(V)
    out = []
    for k in K:
        i = k.index(min(k))
        out.append((k[i], k[(i + 1) % 3], k[(i + 2) % 3]))
    return out


@pytest.mark.parametrize("name", OS.NAMES)
def test_structure(bunny_small, name):
    V, t, o0, o1 = _case(name, bunny_small)
    n = V.shape[0]
    for o in (o0, o1):
        assert np.array_equal(o.takes, t.live)                                 # on a topology's own arrays: the TOPO-live triangles
        dead = ~o.takes
        assert (o.patch_root[dead] == -1).all() and (o.patch[dead] == -1).all() and (o.flip[dead] == 0).all()
        P = int(o.summary[1])
        assert o.proot.shape == o.psize.shape == o.pflags.shape == o.vol6.shape == (P,)
        assert (np.diff(o.proot) > 0).all() and int(o.psize.sum()) == int(o.takes.sum()) == o.summary[0]
        for p in range(P):
            members = np.nonzero(o.patch == p)[0]
            assert members.size == o.psize[p] and members.min() == o.proot[p] and (o.patch_root[members] == o.proot[p]).all()
        # every edge of a topology with m == 2 is a link, and a patch lies inside one component
        assert np.array_equal(o.link >= 0, (t.edge_class == 2) | (t.edge_class == 3))
        live = np.nonzero(o.takes)[0]
        assert len(set(zip(o.patch[live].tolist(), t.component[live].tolist()))) == P
        assert o.summary[2] == ((o.pflags & OE.NONORIENTABLE) == 0).sum() and o.summary[3] == ((o.pflags & OE.OPEN) == 0).sum()
        assert o.summary[4] == o.flip.sum() and o.summary[5] == ((o.pflags & OE.INWARD) != 0).sum() and o.summary[7] == 0
        assert o.summary[6] == o.scale and (o.scale + 30) % 3 == 0
        # non-orientable patches are left alone, and bit 2 says where something is reversed
        for p in range(P):
            f = o.flip[o.patch == p]
            assert bool(f.any()) == bool(o.pflags[p] & OE.REWOUND)
            if o.pflags[p] & OE.NONORIENTABLE:
                assert not f.any() and not o.pflags[p] & OE.INWARD
            if o.pflags[p] & OE.OPEN:
                assert not o.pflags[p] & OE.INWARD
        assert o.flip[o.proot].tolist() == [1 if (o is o1 and f & OE.INWARD) else 0 for f in o.pflags]   # f0(root) = 0
    # outward acts on the INWARD patches alone
    assert np.array_equal(o0.pflags & 11, o1.pflags & 11) and np.array_equal(o0.patch, o1.patch)
    inward = (o0.pflags & OE.INWARD) != 0
    assert np.array_equal(o1.vol6, np.where(inward, -o0.vol6, o0.vol6)) and (o1.vol6[inward] > 0).all()
    tin = np.zeros(n, bool)
    tin[o0.takes] = inward[o0.patch[o0.takes]]
    assert np.array_equal(o1.flip, np.where(tin, 1 - o0.flip, o0.flip))


@pytest.mark.parametrize("name", OS.NAMES)
def test_q_is_exactly_negated_and_nothing_overflows(bunny_small, name):
    V, t, o0, _ = _case(name, bunny_small)
    S = o0.scale
    q, qr = OE.q_of(V, S), OE.q_of(OS.reverse(V), S)
    assert q == o0.q and qr == [-x for x in q]
    assert all(abs(x) < 2 ** 33 for x in q) and V.shape[0] < 2 ** 30
    A = np.abs(V[o0.takes][np.isfinite(V[o0.takes])]).max() if o0.takes.any() else 0.0
    E = (S + 30) // 3
    assert A < 2.0 ** E and (A == 0 or A >= 2.0 ** (E - 1))
    assert all(-2 ** 63 <= int(v) < 2 ** 63 for v in o0.vol6)


@pytest.mark.parametrize("name", OS.NAMES)
def test_reversing_every_winding(bunny_small, name):
    V, t, o0, o1 = _case(name, bunny_small)
    R = OS.reverse(V)
    tr = _topo(R)
    n = V.shape[0]
    r = (np.arange(3 * n) // 3) * 3 + 2 - np.arange(3 * n) % 3                 # what the topology header says
    assert np.array_equal(tr.edge_class, t.edge_class[r])
    assert np.array_equal(tr.twin, np.where(t.twin[r] >= 0, r[np.maximum(t.twin[r], 0)], -1))
    r0 = OE.orient(R, tr.twin, tr.edge_class, False)
    assert np.array_equal(r0.flip, o0.flip) and np.array_equal(r0.patch, o0.patch) and np.array_equal(r0.pflags & 7, o0.pflags & 7)
    assert np.array_equal(r0.vol6, -o0.vol6) and r0.scale == o0.scale
    r1 = OE.orient(R, tr.twin, tr.edge_class, True)
    a, b = OE.rewind(V, o1.flip), OE.rewind(R, r1.flip)
    sa, sb = _oriented_set(a), _oriented_set(b)
    for p in range(int(o1.summary[1])):
        if not o1.pflags[p] & (OE.OPEN | OE.NONORIENTABLE) and o1.vol6[p] != 0:
            for m in np.nonzero(o1.patch == p)[0]:
                assert sa[m] == sb[m], (name, p, m)


@pytest.mark.parametrize("name", OS.NAMES)
@pytest.mark.parametrize("outward", (False, True))
def test_rewind_and_repeat(bunny_small, name, outward):
    V, t, o0, o1 = _case(name, bunny_small)
    o = o1 if outward else o0
    W = OE.rewind(V, o.flip)
    assert np.array_equal(OE.rewind(W, o.flip).view(np.uint32), V.view(np.uint32))   # applied twice it restores the rows, on the bits
    t2 = _topo(W)
    o2 = OE.orient(W, t2.twin, t2.edge_class, outward)
    assert np.array_equal(o2.patch, o.patch) and np.array_equal(o2.pflags & 3, o.pflags & 3)
    assert o2.summary[4] == 0 and not (o2.pflags & OE.REWOUND).any() and not o2.flip.any()
    if outward:
        assert not (o2.pflags & OE.INWARD).any() and o2.summary[5] == 0
    assert np.array_equal(o2.vol6, o.vol6)                                     # the volumes reported are those of the re-wound mesh
    # no FLIPPED edge lies inside an orientable patch
    flipped = np.nonzero(t2.edge_class == 3)[0]
    assert all(o2.pflags[o2.patch[h // 3]] & OE.NONORIENTABLE for h in flipped)
    # a mesh can be made consistently wound exactly when every patch is orientable
    assert (o.summary[2] == o.summary[1]) == (t2.summary[4] == 0)
    if o.summary[2] == o.summary[1]:
        assert TE.oriented(t2) == (t2.summary[5] == 0)


def test_rewind_moves_the_normals_with_their_vertices():
    rows = np.arange(3 * 36, dtype=np.float32).reshape(3, 36)
    out = OE.rewind(rows, [0, 1, 0])
    assert np.array_equal(out[[0, 2]], rows[[0, 2]])
    want = rows[1].copy()
    want[3:6], want[6:9], want[12:15], want[15:18] = rows[1, 6:9], rows[1, 3:6], rows[1, 15:18], rows[1, 12:15]
    assert np.array_equal(out[1], want)


def test_links_read_nothing_out_of_bounds_on_garbage():
    """O2 on arrays that are no topology: ids out of range, one-sided pairs, self-pairs, classes 0, 5 and 255"""
    rng = np.random.default_rng(OS.SEED + 7)
    V = OS.triangles("torus_rev")[:600]
    t = _topo(V)
    n = V.shape[0]
    twin, cls = t.twin.copy(), t.edge_class.copy()
    twin[rng.integers(0, 3 * n, 200)] = rng.integers(-5, 3 * n + 5, 200)
    twin[:6] = [-2 ** 31, 2 ** 31 - 1, 3 * n, -1, 0, 5]
    twin[30:33] = [31, 32, 30]                                                 # self-pairs: g / 3 == t
    cls[rng.integers(0, 3 * n, 100)] = rng.choice([0, 5, 255, 2, 3], 100)
    takes, link = OE.links(twin, cls)
    assert (link[30:33] == -1).all() and (link[:4] == -1).all()
    g = link[link >= 0]
    assert (link[g] == np.nonzero(link >= 0)[0]).all() and takes[g // 3].all()  # links are symmetric
    o = OE.orient(V, twin, cls, True)
    assert o.summary[1] > 1 and (o.patch[~takes] == -1).all()


def test_the_fixtures_are_what_the_device_tests_assume(bunny_small):
    c = lambda name: _case(name, bunny_small)
    # the tetrahedra
    _, _, o0, o1 = c("tetra")
    assert o1.flip.sum() == 0 and o1.pflags.tolist() == [0] and OE.patch_volume(o1)[0] == 1 / 6
    _, _, o0, o1 = c("tetra_flip")
    assert o0.flip.tolist() == [0, 1, 1, 1] and o0.pflags.tolist() == [OE.REWOUND | OE.INWARD]
    assert o1.flip.tolist() == [1, 0, 0, 0] and o1.pflags.tolist() == [OE.REWOUND | OE.INWARD] and OE.patch_volume(o1)[0] == 1 / 6
    # the two non-orientable surfaces
    _, t, o0, o1 = c("moebius")
    assert o1.pflags.tolist() == [OE.OPEN | OE.NONORIENTABLE] and not o1.flip.any() and o1.psize.tolist() == [40]
    V, t, o0, o1 = c("klein")
    assert V.shape[0] == 512 and TE.closed(t) and t.summary[5] == 0 and t.summary[6] == 1 and t.summary[4] > 0
    assert o1.pflags.tolist() == [OE.NONORIENTABLE] and not o1.flip.any() and np.array_equal(o0.vol6, o1.vol6)
    assert o1.vol6[0] == sum(o1.q)                                             # reported as stored
    # torus and strip: one patch each; the reversed torus comes back consistently wound and outward
    for name in ("torus", "torus_rev"):
        V, t, o0, o1 = c(name)
        assert o1.summary[:4].tolist() == [8192, 1, 1, 1] and o1.vol6[0] > 0
        assert abs(OE.patch_volume(o1)[0] - 2 * np.pi ** 2 * 2 * 0.75 ** 2) < 0.5
        W = OE.rewind(V, o1.flip)
        assert TE.oriented(_topo(W)) and np.array_equal(_oriented_set(W), _oriented_set(OE.rewind(c("torus")[0], c("torus")[3].flip)))
    assert not TE.oriented(c("torus_rev")[1]) and 0 < c("torus_rev")[3].flip.sum() < 8192
    for name in ("strip", "strip_rev"):
        V, t, o0, o1 = c(name)
        assert o1.summary[:4].tolist() == [6000, 1, 1, 0] and o1.pflags[0] & OE.OPEN and np.array_equal(o0.flip, o1.flip)
    assert c("strip_rev")[2].flip.sum() > 1000
    # many patches
    V, t, o0, o1 = c("islands_rev")
    assert o1.summary[1] == 3000 and (o1.psize == 1).all() and np.array_equal(o1.proot, np.arange(3000)) and not o1.flip.any()
    V, t, o0, o1 = c("book5")
    assert t.summary[6] == 1 and o1.summary[1] == 5 and (o1.pflags == OE.OPEN).all()
    # a face stored twice
    for name in ("dup2", "dup2_same"):
        V, t, o0, o1 = c(name)
        assert (t.edge_class == (2 if name == "dup2" else 3)).all()
        assert o1.summary[:4].tolist() == [2, 1, 1, 1] and o1.vol6.tolist() == [0] and not o1.pflags[0] & OE.INWARD
        assert np.array_equal(o0.flip, o1.flip) and o1.flip.tolist() == ([0, 0] if name == "dup2" else [0, 1])
    # triangles that do not take part
    V, t, o0, o1 = c("dead")
    import topology_scenes as TS
    assert (o1.patch[list(TS.DEAD_IDS)] == -1).all() and o1.patch[TS.SLIVER_ID] >= 0 and o1.summary[0] == 9
    V, t, o0, o1 = c("signed_zero")
    assert o1.summary[1] == 1 and o1.psize.tolist() == [2]
    # the cubes: exact volumes
    V, t, o0, o1 = c("cube_pow2")
    assert o0.vol6[0] * 2 ** o0.scale == 6 * 64 and o0.pflags.tolist() == [0] and o0.scale == 3 * 3 - 30
    _, _, s0, _ = c("cube_pow2_shift")
    assert s0.scale != o0.scale and s0.vol6[0] * 2.0 ** s0.scale == 6 * 64 and s0.pflags.tolist() == [0]
    _, _, i0, i1 = c("cube_pow2_inside_out")
    assert i0.vol6[0] == -o0.vol6[0] and i0.pflags.tolist() == [OE.INWARD] and i1.pflags.tolist() == [OE.INWARD | OE.REWOUND] and i1.flip.all()
    V, t, o0, o1 = c("nested")
    assert o1.summary[1] == 2 and o1.pflags.tolist() == [0, OE.INWARD | OE.REWOUND] and o1.flip.tolist() == [0] * 12 + [1] * 12
    assert (o1.vol6 * 2.0 ** o1.scale / 6).tolist() == [64.0, 1.0] and (o0.vol6 * 2.0 ** o0.scale / 6).tolist() == [64.0, -1.0]
    # the Bunny: the same triangles under two trees
    V, t, o0, o1 = c("bunny_rev")
    assert np.array_equal(V, c("bunny_rev_not_nested")[0]) and 0 < o1.flip.sum() < V.shape[0] and o1.summary[2] == o1.summary[1]
    assert not TE.oriented(t)

"""The host restatement of the boundary loops (tests/boundary_expected.py) held to what include/ezrt_boundary.h states: the counts of
every case of tests/boundary_scenes.py, every "what follows" item, termination and at most one predecessor on arrays that are no
topology, and the cap: the capped meshes are closed and consistently wound.  No GPU, no library: numpy only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_expected as BE  # noqa: E402
import boundary_scenes as BS  # noqa: E402
import orient_expected as OE  # noqa: E402
import orient_scenes as OS  # noqa: E402
import topology_expected as TE  # noqa: E402

_cache = {}


def _case(name):
    """(rows, the restatement's topology, its boundary), computed once and shared"""
    if name not in _cache:
        T = BS.rows(name)
        t = TE.topology(T, components=False)
        _cache[name] = (T, t, BE.boundary(T, t.twin, t.edge_class))
    return _cache[name]


def _of(V):
    T = BS.TS.tri36(V)
    t = TE.topology(T, components=False)
    return T, t, BE.boundary(T, t.twin, t.edge_class)


@pytest.mark.parametrize("name", BS.NAMES)
def test_counts_and_structure(name):
    T, t, b = _case(name)
    B, L = int(b.summary[0]), int(b.summary[1])
    lens = np.diff(b.loop_offsets).tolist()
    assert B == t.summary[2] and len(lens) == L and b.loop_offsets[0] == 0 and b.loop_offsets[-1] == B   # on a topology's own arrays
    if name in BS.COUNTS:
        assert (B, lens, int(b.summary[2])) == BS.COUNTS[name]
    elif name in BS.SORTED_COUNTS:
        assert (B, sorted(lens), int(b.summary[2])) == BS.SORTED_COUNTS[name]
    else:
        assert name == "strip_rev" and L > 1000 and b.summary[2] == 0 and b.summary[4] == L   # many open paths, one end each
    assert b.summary[3] == max(lens + [0]) and b.summary[6] == b.summary[7] == 0
    bnd = (t.edge_class == 1) & np.repeat(b.takes, 3)
    assert ((b.loop >= 0) == bnd).all() and ((b.pos >= 0) == bnd).all() and (b.next[~bnd] == -1).all()
    assert sorted(b.order.tolist()) == np.nonzero(bnd)[0].tolist()
    heads = b.order[b.loop_offsets[:-1]]
    assert (np.diff(heads) > 0).all()                                          # B4: numbered by ascending head
    for l in range(L):
        m = b.order[b.loop_offsets[l]:b.loop_offsets[l + 1]]
        assert (b.loop[m] == l).all() and (b.pos[m] == np.arange(len(m))).all() and (b.next[m[:-1]] == m[1:]).all()
        if b.lflags[l] & BE.CLOSED:
            assert b.next[m[-1]] == m[0] and m[0] == m.min()                   # B3: the head of a cycle is its lowest half-edge
        else:
            assert b.next[m[-1]] == -1 and not (b.next == m[0]).any()
    if not ((t.edge_class == 3) | (t.edge_class == 4)).any():                  # every edge BOUNDARY or MANIFOLD: every loop is closed
        assert b.summary[2] == L and b.summary[4] == 0
    if name == "strip":                                                        # what the case is for
        assert 2 ** 12 < lens[0] <= 2 ** 13                                    # 13 jumping rounds
        assert 100 < T[b.order[0] // 3, 0] < 2900                              # the head lies in the middle of the strip, not at an end
    if name == "half_fan300":
        assert b.steps == 299
    if name == "pinched":                                                      # each fan keeps its own boundary, through the apex
        P = T[:, :9].reshape(-1, 3)
        assert all((P[b.order[b.loop_offsets[l]:b.loop_offsets[l + 1]]] == 0).all(1).sum() == 1 for l in range(2))
    no_area = BE.boundary(T, t.twin, t.edge_class, area=False)                 # the area group
    assert no_area.area2 is None and no_area.summary[5] == 0 and np.array_equal(no_area.order, b.order)
    assert np.array_equal(np.delete(no_area.summary, 5), np.delete(b.summary, 5))


@pytest.mark.parametrize("name", BS.NAMES)
def test_the_surface_lies_to_the_left(name):
    T, t, b = _case(name)
    V = T[:, :9].reshape(-1, 3, 3).astype(np.float64)
    for h in b.order.tolist():
        tt, e = divmod(h, 3)
        a, bb, w = V[tt, e], V[tt, (e + 1) % 3], V[tt, (e + 2) % 3]
        n = np.cross(V[tt, 1] - V[tt, 0], V[tt, 2] - V[tt, 0])
        if np.dot(n, n) > 0:                                                   # (the sliver of `dead` has no normal)
            assert np.dot(np.cross(n, bb - a), w - a) > 0                      # seen from the normal's side, left of a -> b


def _undirected(seq):
    return [frozenset(e) for e in seq]


def _cyclic_equal(a, b):
    return len(a) == len(b) and (not a or any(a[i:] + a[:i] == b for i in range(len(a))))


@pytest.mark.parametrize("name", BS.NAMES)
def test_reversal_and_permutation(name):
    T, t, b = _case(name)
    V = BS.triangles(name)
    _, _, r = _of(OS.reverse(V))
    assert r.summary.tolist() == b.summary.tolist() or name in ("strip_rev", "moebius", "book5", "dead")
    if name not in ("strip_rev", "moebius", "book5", "dead"):                  # closed loops: reversed as cyclic sequences of undirected edges
        mine, theirs = BE.edge_cycles(T, b), BE.edge_cycles(BS.TS.tri36(OS.reverse(V)), r)
        left = sorted([_undirected(s) for _, s in mine], key=lambda s: sorted(map(sorted, s)))
        right = sorted([_undirected(s)[::-1] for _, s in theirs], key=lambda s: sorted(map(sorted, s)))
        assert len(left) == len(right) and all(_cyclic_equal(x, y) for x, y in zip(left, right))
    assert sorted(map(tuple, (-r.area2).tolist())) == sorted(map(tuple, b.area2.tolist())) or name in ("strip_rev", "moebius", "book5", "dead")
    total = lambda x: [sum(int(v) for v in x.area2[:, k]) for k in range(3)]  # over all chains: every boundary half-edge once, reversed
    assert total(r) == [-v for v in total(b)]
    perm = np.random.default_rng(BS.SEED + 7).permutation(V.shape[0])
    Tp, _, p = _of(V[perm])
    assert BE.edge_cycles(Tp, p) == BE.edge_cycles(T, b)
    assert sorted(map(tuple, p.area2.tolist())) == sorted(map(tuple, b.area2.tolist())) and p.summary.tolist() == b.summary.tolist()


@pytest.mark.parametrize("name", ("lone", "signed_zero", "islands", "strip", "grid_holes", "cube_open", "tetra", "tube", "bunny", "pinched"))
def test_stokes(name):
    """consistently wound, every loop closed: the loops' area2 sum to the triangles' (p2 - p1) x (p3 - p1)"""
    T, t, b = _case(name)
    assert t.summary[4] == 0 and t.summary[5] == 0 and b.summary[2] == b.summary[1]
    V = T[:, :9].reshape(-1, 3, 3).astype(np.float64)
    tri = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]).sum(0)
    loops = np.array([sum(int(v) for v in b.area2[:, k]) for k in range(3)], np.float64) * 2.0 ** b.scale
    if name in ("lone", "signed_zero", "islands", "strip", "grid_holes", "cube_open", "tetra"):   # coordinates that are multiples of 1 / 2: exact
        assert (V * 2 == np.rint(V * 2)).all() and np.array_equal(loops, tri)
        assert np.array_equal(BE.loop_area(b).sum(0) * 2, tri)
    else:                                                                      # each of the B terms is rounded by at most 2^S2 / 2
        assert np.abs(loops - tri).max() <= (b.summary[0] + T.shape[0]) * 2.0 ** b.scale
    if name == "lone":
        assert BE.loop_area(b).tolist() == [[0.0, 0.0, 0.5]]
    if name == "grid_holes":
        assert b.scale == 2 * 4 - 30                                           # A = 8 = 0.5 * 2^4


def test_arrays_that_are_no_topology():
    """B2 on 200 seeded random twin / edge_class arrays of 50 triangles: every walk ends, no half-edge has two predecessors (chains()
    asserts it), and the outputs keep their structure"""
    rng = np.random.default_rng(BS.SEED + 9)
    V = BS.TS.islands(50)
    H = 150
    closed = 0
    for i in range(200):
        tw = rng.integers(-3, H + 3, H).astype(np.int32)
        if i % 2:                                                              # half of them with many mutual pairs, so that walks go far
            p = rng.permutation(H)
            tw[p[0::2][:70]], tw[p[1::2][:70]] = p[1::2][:70], p[0::2][:70]
        cl = rng.choice(np.array([0, 1, 2, 2, 2, 3, 4, 5, 255], np.uint8) if i % 4 < 2 else np.array([1, 2, 2, 2], np.uint8), H)
        b = BE.boundary(V, tw, cl)
        pred = np.bincount(b.next[b.next >= 0], minlength=H)
        assert pred.max(initial=0) <= 1 and b.steps < H
        assert b.loop_offsets[-1] == b.summary[0] == (b.loop >= 0).sum() and sorted(b.order.tolist()) == np.nonzero(b.loop >= 0)[0].tolist()
        closed += int(b.summary[2])
    assert closed > 0                                                          # some of them have cycles


@pytest.mark.parametrize("name", ("cube_open", "tube", "grid_holes", "bunny"))
def test_the_capped_mesh_is_closed(name):
    T, t, b = _case(name)
    cap, valid = BE.cap(T, b)
    lens = np.diff(b.loop_offsets)
    assert valid.sum() == (lens - 2).sum() and cap.shape == (b.summary[0], 36)
    assert not cap[valid == 0].view(np.uint32).any()                           # C4: +0.0f
    if name == "bunny":
        assert valid.sum() == 34
    full = BE.capped(T, b)
    t2 = TE.topology(full)
    assert TE.closed(t2) and TE.oriented(t2) and t2.summary[2] == 0 and t2.summary[4] == 0
    if name == "grid_holes":                                                   # (a disc: the cap over its rim makes a sphere of it)
        assert t2.summary[6] == 1
    o = OE.orient(full, t2.twin, t2.edge_class, False)
    assert o.summary[1] == t2.summary[6] and o.summary[2] == o.summary[3] == o.summary[1] and o.summary[4] == 0   # one closed orientable patch per component
    v = valid != 0
    h = b.order[v]
    assert np.array_equal(cap[v, 18:36].view(np.uint32), T[h // 3, 18:36].view(np.uint32))   # C3: the material of the triangle it closes against
    nb = cap[v, 9:18].view(np.uint32)                                          # on the bits: a fan triangle along a straight rim has a NaN normal
    assert np.array_equal(nb[:, 0:3], nb[:, 3:6]) and np.array_equal(nb[:, 0:3], nb[:, 6:9])
    b2 = BE.boundary(full, t2.twin, t2.edge_class)
    assert b2.summary[0] == 0 and b2.summary[1] == 0
    if name == "cube_open":
        whole = OS.rows("cube_pow2")
        tw = TE.topology(whole)
        want = OE.orient(whole, tw.twin, tw.edge_class, False)
        assert o.vol6.tolist() == want.vol6.tolist() == [6 * 64 * 2 ** -o.scale] and o.scale == want.scale
        assert np.abs(cap[v, 9:18].reshape(-1, 3) - [0, 0, 1]).max() == 0       # the cap faces +z, like the face that was taken out

"""tests/topology_expected.py, the dictionary restatement of include/ezrt_topology.h, held to what the header states -- no GPU.

* the counts of the existing fixtures, which were measured with a throw-away dictionary script written independently of the
  restatement;
* the classes the hand-built scenes of tests/topology_scenes.py are built for;
* the properties that follow from M1 .. M7: twin is an involution without fixed points, reversing every winding changes nothing,
  reversing one changes its three edges only, a permutation of the ids keeps the partition, the classes and every count, and
  closed / oriented are read off the summary."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topology_expected as TE  # noqa: E402
import topology_scenes as TS  # noqa: E402

#          n_tri live manifold boundary flipped nonmanifold components
MEASURED = {"voxel_solid": (288, 288, 432, 0, 0, 0, 1),
            "open_solid": (230, 230, 285, 120, 0, 0, 1),
            "bunny": (5300, 5300, 7929, 42, 0, 0, 3),
            "nasty": (2812, 2812, 736, 6364, 300, 0, 2201)}

_topo = {}


def _t(name, bunny_small=None):
    if name not in _topo:
        _topo[name] = TE.topology(TS.triangles(name, bunny_small))
    return _topo[name]


@pytest.mark.parametrize("name", TS.FIXTURES)
def test_the_fixtures_have_the_measured_counts(bunny_small, name):
    V = TS.triangles(name, bunny_small)
    t = _t(name, bunny_small)
    n_tri, live, manifold, boundary, flipped, nonmanifold, comps = MEASURED[name]
    s = t.summary
    assert (V.shape[0], s[0], s[3], s[2], s[4], s[5], s[6]) == (n_tri, live, manifold, boundary, flipped, nonmanifold, comps)
    assert s[1] == manifold + boundary + flipped + nonmanifold and s[7] == (2 if manifold + flipped else 1)
    assert TE.closed(t) == (name == "voxel_solid") and TE.oriented(t) == (name != "nasty")
    assert t.comp_size.sum() == live and t.live.all()


def test_the_hand_built_scenes_have_their_classes():
    s = lambda name: list(_t(name).summary)
    assert s("tetra") == [4, 6, 0, 6, 0, 0, 1, 2] and TE.closed(_t("tetra")) and TE.oriented(_t("tetra"))
    assert s("tetra_flip") == [4, 6, 0, 3, 3, 0, 1, 2] and TE.closed(_t("tetra_flip")) and not TE.oriented(_t("tetra_flip"))
    assert list(_t("tetra_flip").comp_flags) == [2]
    assert s("bowtie_edge") == [8, 11, 0, 10, 0, 1, 1, 4] and list(_t("bowtie_edge").comp_flags) == [4]
    t = _t("bowtie_edge")
    four = np.nonzero(t.mult == 4)[0]
    assert four.size == 4 and (t.twin[four] >= 0).all() and set(t.twin[four]) == set(four)   # two one way, two the other: all paired
    assert s("bowtie_vertex") == [8, 12, 0, 12, 0, 0, 2, 2] and list(_t("bowtie_vertex").comp_root) == [0, 4]
    assert list(_t("bowtie_vertex").comp_size) == [4, 4] and TE.closed(_t("bowtie_vertex"))
    t = _t("book5")
    assert s("book5") == [5, 11, 10, 0, 0, 1, 1, 5] and list(t.comp_flags) == [5]
    assert list(t.twin[0::3]) == [3, 0, 12, -1, 6]                            # F = 0 6 9, B = 3 12: 0-3, 6-12, 9 alone
    assert (t.twin[t.mult == 1] == -1).all()
    t = _t("book4_same")
    assert s("book4_same") == [4, 9, 8, 0, 0, 1, 1, 4] and list(t.twin[0::3]) == [3, 0, 9, 6]
    for name, k in (("dup5", 5), ("dup200", 200)):
        t = _t(name)
        assert s(name) == [k, 3, 0, 0, 0, 3, 1, k] and (t.mult == k).all() and (t.edge_class == 4).all()
        assert (t.twin == -1).sum() == (3 if k % 2 else 0)                     # an odd number on an edge leaves one alone
    assert s("signed_zero") == [2, 5, 4, 1, 0, 0, 1, 2]
    t = _t("dead")
    assert s("dead")[0] == 9 and not t.live[list(TS.DEAD_IDS)].any() and t.live.sum() == 9 and t.live[TS.SLIVER_ID]
    for d in TS.DEAD_IDS:
        assert list(t.twin[3 * d:3 * d + 3]) == [-1] * 3 and not t.edge_class[3 * d:3 * d + 3].any() and not t.mult[3 * d:3 * d + 3].any()
        assert t.root[d] == t.component[d] == -1
    assert s("dead")[5] == 1 and s("dead")[7] == 3 and s("dead")[6] == 1 and 4 in t.edge_class[3 * TS.SLIVER_ID:3 * TS.SLIVER_ID + 3]
    t = _t("moebius")
    assert s("moebius")[0] == 40 and s("moebius")[2] == 40 and s("moebius")[4] >= 1 and s("moebius")[5] == 0 and s("moebius")[6] == 1
    assert not TE.closed(t) and not TE.oriented(t)
    assert s("torus") == [8192, 12288, 0, 12288, 0, 0, 1, 2] and TE.closed(_t("torus")) and TE.oriented(_t("torus"))
    assert s("strip") == [6000, 12001, 6002, 5999, 0, 0, 1, 2]
    assert s("islands") == [3000, 9000, 9000, 0, 0, 0, 3000, 1] and list(_t("islands").comp_root) == list(range(3000))


def test_a_moebius_band_is_flipped_whatever_its_windings():
    V = TS.triangles("moebius").copy()
    rng = np.random.default_rng(TS.SEED + 5)
    for _ in range(20):
        W = V.copy()
        sel = rng.random(V.shape[0]) < 0.5
        W[sel] = W[sel][:, ::-1]
        assert TE.topology(W).summary[4] >= 1


@pytest.mark.parametrize("name", TS.CPU_NAMES)
def test_twin_is_an_involution_and_agrees_with_the_classes(bunny_small, name):
    t = _t(name, bunny_small)
    h = np.nonzero(t.twin >= 0)[0]
    assert np.array_equal(t.twin[t.twin[h]], h) and (t.twin[h] != h).all()
    assert (t.twin[h] // 3 != h // 3).all()                                    # never within one triangle
    assert np.array_equal(t.edge_class[t.twin[h]], t.edge_class[h]) and np.array_equal(t.mult[t.twin[h]], t.mult[h])
    assert (t.twin[t.edge_class == TE.BOUNDARY] == -1).all() and (t.twin[(t.edge_class == 2) | (t.edge_class == 3)] >= 0).all()
    assert ((t.edge_class == 0) == np.repeat(~t.live, 3)).all()
    # the pairs agree with the rule for pairs
    V = TS.triangles(name, bunny_small)
    sh, op = TE.at(V, h // 3, h % 3, t.twin[h] // 3)
    assert np.array_equal(sh, t.twin[h] % 3)
    two = t.mult[h] == 2
    assert np.array_equal(op[two] == 1, t.edge_class[h][two] == TE.MANIFOLD)
    # components: roots are the lowest ids, numbered in ascending order; neighbours share a component
    assert np.array_equal(t.comp_root, np.sort(t.comp_root)) and np.array_equal(t.root[t.live], t.comp_root[t.component[t.live]])
    assert (t.root[t.live] <= np.nonzero(t.live)[0]).all() and np.array_equal(np.bincount(t.component[t.live]), t.comp_size)
    assert np.array_equal(t.component[h // 3], t.component[t.twin[h] // 3])


def _reverse(V, sel):
    W = V.copy()
    W[sel] = W[sel][:, [0, 2, 1]]
    return W


@pytest.mark.parametrize("name", ("voxel_solid", "nasty", "tetra_flip", "book5", "dup5", "dead", "moebius", "strip"))
def test_reversing_every_winding_changes_nothing(bunny_small, name):
    V = TS.triangles(name, bunny_small)
    t, r = _t(name, bunny_small), TE.topology(_reverse(V, np.ones(V.shape[0], bool)))
    h = np.arange(3 * V.shape[0])
    rh = h // 3 * 3 + 2 - h % 3                                                # (p1, p3, p2): half-edge e lies where 2 - e lay
    assert np.array_equal(r.edge_class, t.edge_class[rh]) and np.array_equal(r.mult, t.mult[rh])
    tw = t.twin[rh]
    assert np.array_equal(r.twin, np.where(tw >= 0, tw // 3 * 3 + 2 - tw % 3, -1))
    for k in ("root", "component", "comp_root", "comp_size", "comp_flags", "summary"):
        assert np.array_equal(getattr(r, k), getattr(t, k)), k


@pytest.mark.parametrize("name", ("voxel_solid", "tetra", "torus"))
def test_reversing_one_winding_changes_its_three_edges(bunny_small, name):
    V = TS.triangles(name, bunny_small)
    t = _t(name, bunny_small)
    one = V.shape[0] // 3
    sel = np.zeros(V.shape[0], bool)
    sel[one] = True
    r = TE.topology(_reverse(V, sel))
    assert r.summary[4] == 3 and r.summary[3] == t.summary[3] - 3 and not TE.oriented(r) and TE.closed(r)
    changed = np.nonzero(r.edge_class != t.edge_class)[0]
    nb = t.twin[3 * one:3 * one + 3]
    assert set(changed) == set(range(3 * one, 3 * one + 3)) | set(int(x) for x in nb)
    assert np.array_equal(r.component, t.component) and list(r.comp_flags) == [2]


@pytest.mark.parametrize("name", ("open_solid", "nasty", "bowtie_edge", "dead", "moebius", "strip"))
def test_a_permutation_of_the_ids_keeps_the_topology(bunny_small, name):
    V = TS.triangles(name, bunny_small)
    t = _t(name, bunny_small)
    perm = np.random.default_rng(TS.SEED + 7).permutation(V.shape[0])         # new triangle i is old triangle perm[i]
    W = np.ascontiguousarray(V[perm])
    r = TE.topology(W)
    assert np.array_equal(r.summary, t.summary)
    assert np.array_equal(r.edge_class.reshape(-1, 3), t.edge_class.reshape(-1, 3)[perm]) and np.array_equal(r.mult.reshape(-1, 3), t.mult.reshape(-1, 3)[perm])
    assert TE.edge_relation(W, r) == TE.edge_relation(V, t)
    # the partition: two triangles share a component after exactly when they did before
    assert np.array_equal(r.live, t.live[perm])
    pairs = collections.Counter(zip(r.component.tolist(), t.component[perm].tolist()))
    assert len(pairs) == len(set(a for a, _ in pairs)) == len(set(b for _, b in pairs))
    assert sorted(r.comp_size.tolist()) == sorted(t.comp_size.tolist())
    # twin as a relation on edges with m <= 2
    inv = np.argsort(perm)
    old = t.twin.reshape(-1, 3)[perm]                                          # the old twin of the new triangle's half-edges, in old ids
    moved = np.where(old >= 0, inv[np.maximum(old, 0) // 3] * 3 + old % 3, -1)
    low = r.mult.reshape(-1, 3) <= 2
    assert np.array_equal(r.twin.reshape(-1, 3)[low], moved[low])


def test_the_rule_for_pairs():
    V = TS.triangles("dead")
    n = V.shape[0]
    a, e, b = np.meshgrid(np.arange(-1, n + 1), np.arange(-1, 4), np.arange(-1, n + 1), indexing="ij")
    a, e, b = a.ravel(), e.ravel(), b.ravel()
    sh, op = TE.at(V, a, e, b)
    t = _t("dead")
    bad = (a < 0) | (a >= n) | (b < 0) | (b >= n) | (e < 0) | (e > 2)
    assert (sh[bad] == -1).all() and (op[bad] == -1).all()
    ok = ~bad
    dead = np.zeros(a.size, bool)
    dead[ok] = ~t.live[a[ok]] | ~t.live[b[ok]]
    assert (sh[dead] == -1).all() and ((sh == -1) == (op == -1)).all()
    same = ok & ~dead & (a == b)
    assert np.array_equal(sh[same], e[same]) and (op[same] == 0).all()
    assert (sh[ok & ~dead] >= 0).sum() > same.sum() + 16
    sh2, op2 = TE.at(TS.triangles("signed_zero"), [0, 0, 0, 1], [0, 1, 2, 0], [1, 1, 1, 0])
    assert list(sh2) == [0, -1, -1, 0] and list(op2) == [1, -1, -1, 1]

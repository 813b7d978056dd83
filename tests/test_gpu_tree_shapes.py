"""The point and overlap queries on every tree shape a caller can pass (tests/tree_shapes.py): a median tree with leaves of one
triangle, leaves of 128, a chain of depth 63 with the re-tree off and on, a root that is a leaf, a root with two leaves, triangles
that no leaf holds, loose boxes, a leaf box that misses a vertex, and the device LBVH builder's trees.

First the route that the shape must take (prune_info: mode, records4, retreed), then closest_point (without d_max and with the
winner's own distance), nearest (k = 1 and 5, with and without the count, d_max at the third nearest's distance, and d_max = None
with the count), inside on all six axes with the crossings, signed_distance, box_overlap and tri_overlap (max_k = 0, 8, 64 with
the count), self_overlap (every triangle, and a shuffled subset of ids) and the `_at` calls on the returned rows -- each against
the numpy restatements over ALL triangles, on the bits with NaN equal to NaN: what the walks lose of a tree shows as a difference.
Then a refit that moves a scene from the walk to the sweep (a NaN vertex) and back, and a refit of the triangles that no leaf holds.
tests/test_tree_shapes.py shows on the CPU that the shapes are what their names say and that the comparisons are not vacuous."""
import os
import sys

import numpy as np
import pytest

from ezrt_amd import query, refit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_shapes as T  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(name, None) for name in T.HOST_SHAPES + T.LBVH_SHAPES if name != "chain"] + [("chain", 0), ("chain", 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


class _Env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _scene(hip, name, retree):
    """the device scene of a case"""
    tri, nodes, expect = T.shape(name)
    if retree is None:
        return hip.scene_create(tri, nodes)
    with _Env(EZRT_RETREE=retree):                                     # read at scene creation
        return hip.scene_create(tri, nodes)


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def answers(sg, Q, W, dev):
    """dict name -> numpy array: every query of tree_shapes.expected on the device scene `sg`; W gives the inputs that are derived
    from answers (the d_max arrays and the id subset)"""
    G = {}
    p, lo, hi, tris = (_gpu(Q[k], dev) for k in ("points", "lo", "hi", "tris"))
    n_tri = sg.stats()["n_tri"]
    cp = query.closest_point(sg, p)
    G["cp.tri"], G["cp.point"], G["cp.dist"], G["cp.bary"] = cp
    G["cpd.tri"], G["cpd.point"], G["cpd.dist"], G["cpd.bary"] = query.closest_point(sg, p, _gpu(W["_d_max.cp"], dev))
    dm = _gpu(W["_d_max.near"], dev)
    for k, count in T.NEAREST:
        r = query.nearest(sg, p, k, dm, count=count)
        G["near%d%d.tri" % (k, count)], G["near%d%d.dist" % (k, count)] = r.tri, r.dist
        assert (r.count is not None) == count
        if count:
            G["near%d%d.count" % (k, count)] = r.count
    G["near_all.tri"], G["near_all.dist"], G["near_all.count"] = query.nearest(sg, p, 5, None, count=True)
    at = query.closest_point_at(sg, p, G["near51.tri"])
    G["near_at.point"], G["near_at.dist"], G["near_at.bary"] = at.point, at.dist, at.bary
    for axis in T.AXES:
        G["inside%d" % axis], G["crossings%d" % axis] = query.inside(sg, p, axis, crossings=True)
    sd = query.signed_distance(sg, p)
    G["sd.tri"], G["sd.point"], G["sd.dist"], G["sd.bary"], G["sd.inside"] = sd
    for k in T.OVERLAP_K:
        G["box%d.tri" % k], G["box%d.n" % k] = query.box_overlap(sg, lo, hi, k, count=True)
        G["trio%d.tri" % k], G["trio%d.n" % k] = query.tri_overlap(sg, tris, k, count=True)
    G["box_at"] = query.box_overlap_at(sg, lo, hi, G["box8.tri"])
    G["trio_at"] = query.tri_overlap_at(sg, tris, G["trio8.tri"])
    G["self8.tri"], G["self8.n"] = query.self_overlap(sg, None, 8, count=True)
    ids = _gpu(W["_ids"], dev, np.int32)
    for k in (0, 64):
        G["self_ids%d.tri" % k], G["self_ids%d.n" % k] = query.self_overlap(sg, ids, k, count=True)
    every = torch.arange(n_tri, dtype=torch.int32, device=dev)[:, None].expand(n_tri, 8).contiguous()
    G["self_at"] = query.self_overlap_at(sg, every, G["self8.tri"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in G.items()}


def _route(sg):
    info = sg.prune_info()
    return dict(mode=info["mode"], records4=info["records4"], retreed=info["retreed"])


@pytest.mark.parametrize("name,retree", CASES, ids=["%s%s" % (n, "" if r is None else "-retree%d" % r) for n, r in CASES])
def test_every_query_on_the_bits(hip, dev, name, retree):
    tri, nodes, expect = T.shape(name)
    if name in T.LBVH_SHAPES:                                          # made on the device: checked here, not on the CPU
        facts = T.check_valid(tri, nodes)
        assert facts["nested"] and facts["holds"] and facts["uncovered"].size == 0 and facts["max_leaf"] <= expect["max_leaf"]
        assert tri.shape == T.base().shape and sorted(map(bytes, tri)) == sorted(map(bytes, T.base()))   # the base set, reordered
    sg = _scene(hip, name, retree)
    route = _route(sg)
    print("route %s%s: %s, depth %d" % (name, "" if retree is None else " EZRT_RETREE=%d" % retree, route, sg.stats()["depth"]))
    if expect["walk"]:
        assert route["mode"] != -1 and route["records4"] > 0, route   # the pruned route: the walks
    else:
        assert route["mode"] == -1 or route["records4"] == 0, route   # the sweep
    if "mode" in expect:
        assert route["mode"] == expect["mode"] and route["records4"] > 0, route   # (leaf_misses: records, but no pruning)
    if expect.get("records4") is not None:
        assert route["records4"] == expect["records4"], route
    for want in (retree, expect["retree"]):
        if want is not None:
            assert route["retreed"] == float(want), route
    if "depth" in expect:
        assert sg.stats()["depth"] == expect["depth"]
    Q, W = T.shape_queries(name), T.shape_expected(name)
    bad = T.differing(answers(sg, Q, W, dev), W)
    assert not bad, "%s: %s" % (name, ", ".join(bad))


def test_a_refit_moves_the_route_to_the_sweep_and_back(hip, dev):
    tri, nodes, expect = T.shape("sah8")
    Q, W = T.shape_queries("sah8"), T.shape_expected("sah8")
    t = int(np.bincount(W["cp.tri"][W["cp.tri"] >= 0]).argmax())
    moved = np.array(tri)
    moved[t, 4] = np.nan                                               # one vertex of a triangle that wins points: nobody's candidate now
    M = T.expected(moved, Q)
    assert (W["cp.tri"] == t).any() and not (M["cp.tri"] == t).any() and not (M["box64.tri"] == t).any()
    sg = hip.scene_create(tri, nodes)
    assert _route(sg)["mode"] != -1
    first = answers(sg, Q, W, dev)
    assert not T.differing(first, W)
    refit.refit(sg, moved)
    assert _route(sg)["mode"] == -1, _route(sg)                        # a leaf box cannot hold a NaN: the scene does not prune, swept
    bad = T.differing(answers(sg, Q, M, dev), M)
    assert not bad, ", ".join(bad)
    refit.refit(sg, np.array(tri))                                     # back: the walk again, and the first call's answers
    assert _route(sg)["mode"] != -1 and _route(sg)["records4"] > 0, _route(sg)
    again = answers(sg, Q, W, dev)
    bad = T.differing(again, first)
    assert not bad and not T.differing(again, W), ", ".join(bad)


def test_a_refit_of_the_triangles_that_no_leaf_holds(hip, dev):
    tri, nodes, expect = T.shape("uncovered")
    Q, W = T.shape_queries("uncovered"), T.shape_expected("uncovered")
    unc = expect["uncovered"]
    moved = np.array(tri)
    for v in range(3):
        moved[unc, 3 * v:3 * v + 3] += np.float32([0.25, -0.5, 0.25])  # only they move; they stay among the others
    M = T.expected(moved, Q)
    changed = [k for k in ("cp.tri", "near51.tri", "crossings0", "box8.tri", "trio8.tri", "self8.n")
               if (M[k].reshape(M[k].shape[0], -1) != W[k].reshape(M[k].shape[0], -1)).any(1).sum() >= 10]
    assert len(changed) == 6, changed                                  # the move changes answers of every kind
    sg = hip.scene_create(tri, nodes)
    assert _route(sg)["mode"] != -1
    refit.refit(sg, moved)
    assert _route(sg)["mode"] != -1 and _route(sg)["records4"] > 0     # still the walk, and the sweeps behind it
    got = answers(sg, Q, M, dev)
    bad = T.differing(got, M)
    assert not bad, ", ".join(bad)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, nodes))   # what the refit must be equal to
    assert _route(fresh)["mode"] != -1
    bad = T.differing(answers(fresh, Q, M, dev), got)
    assert not bad, ", ".join(bad)

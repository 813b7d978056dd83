"""The tree shapes of tests/tree_shapes.py, on the CPU: every pair of arrays is one that ezrt_scene_create accepts, every shape has the
property it is named for, and -- on the numpy restatements alone -- the queries of tests/test_gpu_tree_shapes.py are no
comparison of nothing: the triangles that no leaf holds decide a share of the answers, the points at the chain's deep end reach
every triangle, and misses and empty rows are the smaller half of every batch.  (The LBVH shapes need the device: they are checked
where they are made, in the GPU test.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_point_expected as E  # noqa: E402
import nearest_expected as NE  # noqa: E402
import tree_shapes as T  # noqa: E402


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_scene_create_accepts_the_arrays(name):
    tri, nodes, expect = T.shape(name)
    facts = T.check_valid(tri, nodes)                                  # parent < child < m, ranges inside, depth <= 63, leaf <= 128
    assert tri.dtype == np.float32 and tri.shape[1] == 36 and tri.shape[0] <= 1500
    assert expect["walk"] == (facts["nested"] and facts["holds"] and nodes.shape[0] > 2)
    Q = T.shape_queries(name)
    assert all(T.N_QUERIES <= Q[k].shape[0] <= 300 for k in ("points", "lo", "hi", "tris"))


def test_the_base_set():
    tri = T.base()
    assert 1000 <= tri.shape[0] <= 1500
    V = T.vertices(tri)
    twice = [V[k].tobytes() for k in range(V.shape[0])]
    assert len(twice) - len(set(twice)) == T.N_DUPLICATES              # exact duplicates: ties
    W = T.shape_expected("sah8")
    inside = W["inside0"][:T.N_QUERIES - 16]
    assert 0.1 < inside.mean() < 0.9                                   # closed solids: inside is no constant
    assert (W["self8.n"] > 0).mean() > 0.5 and (W["self8.n"] > 8).any()


def test_each_shape_has_the_property_it_is_named_for():
    facts = {name: T.check_valid(*T.shape(name)[:2]) for name in T.HOST_SHAPES}
    for name in T.HOST_SHAPES:
        assert facts[name]["nested"], name                             # every shape is nested; one leaf box misses a vertex
        assert facts[name]["holds"] == (name != "leaf_misses"), name
        assert facts[name]["uncovered"].size == (39 if name == "uncovered" else 0), name
    assert facts["sah8"]["max_leaf"] == 8 and facts["sah8"]["depth"] < 20
    tri, nodes, expect = T.shape("median1")
    assert facts["median1"]["max_leaf"] == 1 and facts["median1"]["n_leaves"] == tri.shape[0]
    tri, nodes, expect = T.shape("leaf128")
    assert facts["leaf128"]["max_leaf"] == 128 and expect["n128"] >= 1 and (nodes[1:, 3] == 128).sum() == expect["n128"]
    tri, nodes, expect = T.shape("chain")
    assert facts["chain"]["depth"] == 63 == expect["depth"] and nodes.shape[0] == 2 * 62 + 2 and tri.shape[0] == 280
    inner = [i for i in range(1, nodes.shape[0]) if nodes[i, 3] == 0]
    assert len(inner) == 62 and all(nodes[int(nodes[i, 0]), 3] > 0 for i in inner)          # a leaf on the left of every inner node
    assert all(nodes[int(nodes[i, 1]), 3] == 0 for i in inner[:-1]) and nodes[int(nodes[inner[-1], 1]), 3] > 0
    assert [int(nodes[int(nodes[i, 0]), 3]) for i in inner[:9]] == [1, 2, 3, 4, 5, 6, 7, 8, 1]
    for name, n in (("root_leaf_1", 1), ("root_leaf_8", 8)):
        tri, nodes, expect = T.shape(name)
        assert nodes.shape[0] == 2 and nodes[1, 3] == n == tri.shape[0] and facts[name]["depth"] == 1
    tri, nodes, expect = T.shape("two_leaves")
    assert nodes.shape[0] == 4 and sorted(nodes[2:, 3]) == [3, 5]
    tri, nodes, expect = T.shape("loose")
    tight = T.shape("sah8")[1]
    assert np.array_equal(nodes[:, :6], tight[:, :6]) and (nodes[1:, 6:9] <= tight[1:, 6:9]).all() and (nodes[1:, 9:12] >= tight[1:, 9:12]).all()
    assert ((nodes[1:, 6:9] < tight[1:, 6:9]) | (nodes[1:, 9:12] > tight[1:, 9:12])).any(1).all()   # every box is looser
    tri, nodes, expect = T.shape("leaf_misses")
    i = expect["missing_leaf"]
    v = T.vertices(tri)[int(nodes[i, 4]):int(nodes[i, 4] + nodes[i, 3]), :, 0].max()
    assert nodes[i, 9] < v and np.nextafter(nodes[i, 9], np.float32(np.inf)) == v            # by one ulp
    changed = np.nonzero((nodes != T.shape("sah8")[1]).any(1))[0]
    assert list(changed) == [i]


def test_the_uncovered_triangles_lie_among_the_others_and_copy_lower_indices():
    tri, nodes, expect = T.shape("uncovered")
    unc = expect["uncovered"]
    assert np.array_equal(T.check_valid(tri, nodes)["uncovered"], unc) and unc.size == 39
    assert (unc >= tri.shape[0] - T.N_APPENDED).sum() == T.N_APPENDED and (unc < expect["n_covered_by_builder"]).sum() == 2
    i = expect["cut_leaf"]                                             # the cut leaf keeps a box that still holds what it lost
    lost = T.vertices(tri)[unc[:2]].reshape(-1, 3)
    assert (lost >= nodes[i, 6:9]).all() and (lost <= nodes[i, 9:12]).all() and 1 < i < nodes.shape[0] - 1
    V = T.vertices(tri)
    covered = np.setdiff1d(np.arange(tri.shape[0]), unc)
    assert expect["copies"].size >= 10 and np.isin(expect["copies"], unc).all() and np.isin(expect["originals"], covered).all()
    assert (expect["originals"] < expect["copies"]).all() and np.array_equal(V[expect["originals"]], V[expect["copies"]])
    lo, hi = V[covered].reshape(-1, 3).min(0), V[covered].reshape(-1, 3).max(0)
    c = V[unc].mean(1)
    assert (c > lo).all() and (c < hi).all()                           # not off to one side ...
    d2 = NE.dist2_all(c, tri[covered])
    assert (np.sqrt(d2.min(1)) <= 1.0).all()                           # ... a covered triangle within one voxel of each


def _uses(rows, ids):
    return np.isin(rows, ids).any(1)


def test_a_lost_sweep_would_change_the_answers():
    """On the restatement alone: what the uncovered triangles decide.  Removing them from the array is modelled by making them
    non-finite, which keeps the indices of the others: a non-finite triangle is no candidate of any query."""
    tri, nodes, expect = T.shape("uncovered")
    Q, W = T.shape_queries("uncovered"), T.shape_expected("uncovered")
    unc = expect["uncovered"]
    n = Q["points"].shape[0]
    won = np.isin(W["cp.tri"], unc)
    assert won.sum() >= 0.1 * n, won.sum()
    for key in ("box64", "trio64"):
        rows, count = W[key + ".tri"], W[key + ".n"]
        assert _uses(rows, unc)[count > 0].mean() >= 0.1, key
    by_covered = ~np.isin(W["_ids"], unc) & (W["self_ids64.n"] > 0)     # the rows of covered queries: only the sweep lists an uncovered id there
    assert _uses(W["self_ids64.tri"], unc)[by_covered].mean() >= 0.1
    assert (np.isin(W["_ids"], unc) & (W["self_ids64.n"] > 0)).sum() >= 10             # and uncovered triangles as the queries
    assert np.isin(unc, W["_ids"]).all()                               # the id subset has every uncovered triangle as a query
    assert (_uses(W["near51.tri"], unc) & ~won).sum() >= 10            # lists that change where the winner does not: the duplicates
    gone = np.array(tri)
    gone[unc, :9] = np.nan
    L = T.expected(gone, Q, W["_ids"])
    covered = {"self8.n": ~np.isin(np.arange(tri.shape[0]), unc), "self_ids64.tri": ~np.isin(W["_ids"], unc)}
    for key, least in (("cp.tri", 10), ("near51.tri", 10), ("near51.count", 10), ("crossings0", 10), ("crossings4", 10), ("sd.dist", 10),
                       ("box8.tri", 10), ("box0.n", 10), ("trio8.tri", 10), ("trio0.n", 10), ("self8.n", 10), ("self_ids64.tri", 10)):
        a, b = W[key].reshape(W[key].shape[0], -1), L[key].reshape(W[key].shape[0], -1)
        rows = (a.view(np.uint32) != b.view(np.uint32)).any(1) if a.dtype == np.float32 else (a != b).any(1)
        changed = int((rows & covered.get(key, True)).sum())           # (self-overlap: a row whose own triangle is gone does not count)
        assert changed >= least, (key, changed)


def test_the_deep_end_points_reach_every_triangle_with_three_entries_pending_per_record():
    tri, nodes, expect = T.shape("chain")
    Q, W = T.shape_queries("chain"), T.shape_expected("chain")
    deep = Q["deep"]
    assert deep.stop - deep.start == 16 and deep.start == T.N_QUERIES
    assert (W["near_all.count"][deep] == tri.shape[0]).all()           # d_max = None, count = True: every triangle is counted
    assert (Q["lo"][-1] == T.vertices(tri).reshape(-1, 3).min(0)).all() and W["box0.n"][-1] == tri.shape[0]   # the box over everything
    # with the re-tree off the records are {leaf k, leaf k + 1, leaf k + 2, inner k + 3} for k = 0, 3 .. 57 (tree_shapes' docstring).
    # For these points the inner slot's box -- everything deeper -- is strictly nearer than each of the three leaves, so the walk
    # descends it first and pushes the three leaves (each within the radius, which is still +inf: the first triangle is met at
    # the bottom), and the last record {leaf 60, 61, 62} adds two: 20 * 3 + 2 = 62 entries pending there
    p = Q["points"][deep]
    lb = lambda i: (np.maximum(np.maximum(nodes[i, 6:9] - p, p - nodes[i, 9:12]), 0) ** 2).sum(1)
    inner, leaf = (lambda k: 1 + 2 * k), (lambda k: 2 + 2 * k)
    for k in range(0, 58, 3):
        assert nodes[inner(k + 3), 3] == 0 and all(nodes[leaf(k + j), 3] > 0 for j in range(3))
        assert all((lb(inner(k + 3)) < lb(leaf(k + j))).all() for j in range(3)), k
    assert expect["stack_need_cp"] == 20 * 3 + 2 and (expect["stack_need_cp"] + 1) * 2 * 64 * 4 == 32256 <= 64 * 1024


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_misses_and_empty_rows_are_the_smaller_half(name):
    """Where the GPU test accepts a miss or an empty row, at most half of the batch is one -- for the seeds of tree_shapes.SEEDS."""
    tri, nodes, expect = T.shape(name)
    W = T.shape_expected(name)
    share = {"closest_point": (W["cp.tri"] < 0).mean(), "closest_point, d_max": (W["cpd.tri"] < 0).mean(),
             "box_overlap": (W["box0.n"] == 0).mean(), "tri_overlap": (W["trio0.n"] == 0).mean(),
             "self_overlap": (W["self8.n"] == 0).mean(), "self_overlap, ids": (W["self_ids0.n"] == 0).mean(),
             "inside": (np.stack([W["crossings%d" % a] for a in T.AXES]).sum(0) == 0).mean()}     # no crossing on any axis
    for k, count in T.NEAREST:
        share["nearest %d %s" % (k, count)] = (W["near%d%d.tri" % (k, count)][:, 0] < 0).mean()
    if tri.shape[0] == 1:                                              # one triangle crosses no other: the rows are empty by definition
        assert share.pop("self_overlap") == 1.0 and share.pop("self_overlap, ids") == 1.0
    if tri.shape[0] <= 8:
        # a handful of triangles: the axis rays of the 257 points of the generator cross none of them, and 300 points a call leave
        # room for 40 more -- so not half of the batch, but every one of the 40 points next to the triangles has a crossing, and
        # both answers occur on an axis
        near = T.shape_queries(name)["near"]
        crossed = np.stack([W["crossings%d" % a][near] for a in T.AXES])
        assert near.stop - near.start == T.N_NEAR == 40 and (crossed.sum(0) > 0).all()
        assert any(8 <= W["inside%d" % a][near].sum() <= 32 for a in T.AXES)
        assert share.pop("inside") <= 0.9
    assert max(share.values()) <= 0.5, share
    assert (W["cp.tri"] < 0).sum() == 16                               # the 16 points that are not finite, and only they
    assert (W["_d_max.near"] == np.float32(0.75)).sum() >= 64 and np.isfinite(W["_d_max.near"]).mean() > 0.9
    ties = E.closest_point(T.shape_queries(name)["points"], tri, with_ties=True)[4]
    if tri.shape[0] > 8:
        assert (ties > 1).mean() > 0.2                                 # winners decided by the lowest index


@pytest.mark.parametrize("name", [n for n in T.HOST_SHAPES if n not in ("root_leaf_1", "root_leaf_8", "two_leaves")])
def test_the_tie_points_have_boxes_at_the_radius(name):
    """The tie points: the distance h, the radius h * h of d_max = h, the winner's dist2 and the lb of the winner's own bounding box
    are one float32.  With leaves of one triangle (median1) the leaf boxes are those bounding boxes: EVERY candidate within the
    radius is then below a box at lb == radius, so a walk that skipped on lb >= radius would answer with a miss."""
    tri, nodes, expect = T.shape(name)
    Q, W = T.shape_queries(name), T.shape_expected(name)
    ties = Q["ties"]
    p, h = Q["points"][ties], Q["tie_h"]
    assert p.shape[0] == T.N_TIES and set(h) == {np.float32(0.25), np.float32(0.5)}
    assert np.array_equal(W["cp.dist"][ties], h) and np.array_equal(W["_d_max.cp"][ties], h) and np.array_equal(W["_d_max.near"][ties], h)
    assert (W["cp.tri"][ties] >= 0).all() and np.array_equal(W["cpd.tri"][ties], W["cp.tri"][ties])
    V = T.vertices(tri)
    d2 = NE.dist2_all(p, tri)
    lb = T.box_lb(p[:, None, :], V.min(1)[None], V.max(1)[None])
    within = d2 <= (h * h)[:, None]
    assert np.array_equal(within.sum(1), W["near51.count"][ties]) and (within.sum(1) >= 1).all()
    assert (lb[within] == np.broadcast_to((h * h)[:, None], lb.shape)[within]).all()   # every one of them at lb == radius, none below
    if name not in ("chain", "uncovered"):                             # (their strip and their subset keep fewer of the copies)
        assert (within.sum(1) >= 2).sum() >= T.N_TIES // 2             # an exact copy shares the distance: the lowest id wins
    if name == "median1":
        leaf = nodes[1:][nodes[1:, 3] == 1]
        first = leaf[:, 4].astype(int)
        assert leaf.shape[0] == tri.shape[0] and np.array_equal(leaf[:, 6:9], V.min(1)[first]) and np.array_equal(leaf[:, 9:12], V.max(1)[first])


# ---- the rays of tests/test_gpu_tree_shapes_rays.py: conditions on the inputs, on the CPU oracle alone -- they hit, the tie rays tie
# (across leaves, and for the higher index on the median tree), slot 0 of the restated all-hits list is the oracle's closest hit, the
# triangles that no leaf holds change the answers, and the chain's rays leave 48 entries pending

LARGE = [n for n in T.HOST_SHAPES if n not in ("root_leaf_1", "root_leaf_8", "two_leaves")]
TIES_AT_LEAST = dict(sah8=0.5, median1=0.5, leaf128=0.5, chain=0.5, loose=0.5, leaf_misses=0.5, uncovered=0.4)


_same = T.RS.same_bits                                                  # equal on the bits, NaN equal to NaN


def _leaf_of(nodes, n_tri):
    """int [n_tri]: the node whose leaf holds each triangle (-1: none)"""
    leaf = np.full(n_tri, -1)
    for i in range(1, nodes.shape[0]):
        if nodes[i, 3] > 0:
            leaf[int(nodes[i, 4]):int(nodes[i, 4] + nodes[i, 3])] = i
    return leaf


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_the_rays_hit_and_slot_0_is_the_oracles_closest_hit(oracle, name):
    tri, nodes, expect = T.shape(name)
    Q, X = T.ray_queries(name), T.ray_expected(oracle, name)
    n = Q["rays"].shape[0]
    sizes = {k: v.stop - v.start for k, v in Q.items() if isinstance(v, slice)}
    assert n % 64 == 1 and 500 <= n <= 1100 and sum(sizes.values()) == n, sizes
    large = tri.shape[0] > 8
    assert sizes["broad"] == T.N_BROAD and sizes["near"] == T.N_NEAR_RAYS
    assert sizes["ties"] == (T.N_TIE_RAYS if large else 0) and sizes["on_uncovered"] == (T.N_ON_UNCOVERED if name == "uncovered" else 0)
    assert (sizes["deep"], sizes["shallow"]) == ((T.N_CHAIN_DEEP, T.N_CHAIN_SHALLOW) if name == "chain" else (0, 0)) and sizes["pad"] < 64
    hit = X["closest.tri"] >= 0
    count = X["all64.count"]
    print("%s: %d rays %s; hits: near %.3f, batch %.3f; all-hits count > 5: %.3f, largest %d" % (
        name, n, sizes, hit[Q["near"]].mean(), hit.mean(), (count > 5).mean(), count.max()))
    assert hit[Q["near"]].mean() >= 0.95 and 0.2 <= hit.mean() <= 0.99
    assert count.max() <= 64
    if large:
        assert (count > 5).mean() >= 0.05
    # slot 0 of the restated list is the oracle's own closest hit, on every ray: the restatement is pinned to ezrt_query_hits here
    assert np.array_equal(X["all64.tri"][:, 0], X["closest.tri"]) and _same(X["all64.t"][:, 0], X["closest.t"])
    assert np.array_equal(count > 0, X["occluded"]) and np.array_equal(X["all1.count"], count)
    for key in T.T_MAX:                                                # ... and under every derived t_max
        assert np.array_equal(X["all64[%s].tri" % key][:, 0], X["closest[%s].tri" % key]), key
        assert _same(X["all64[%s].t" % key][:, 0], X["closest[%s].t" % key]) and np.array_equal(X["all2[%s].count" % key] > 0, X["occluded[%s]" % key])
    assert not X["occluded[own]"].any() and np.array_equal(X["occluded[above]"], hit) and not X["occluded[nan]"].any()
    if large:
        assert 0 < X["occluded[second]"].sum() < hit.sum()             # the second hit's t: admits the first unless the two tie


@pytest.mark.parametrize("name", LARGE)
def test_the_tie_rays_tie_at_the_nearest_hit(oracle, name):
    tri, nodes, expect = T.shape(name)
    Q, X = T.ray_queries(name), T.ray_expected(oracle, name)
    ties = Q["ties"]
    ids, t = X["all64.tri"][ties], X["all64.t"][ties]
    tied = (ids[:, 1] >= 0) & (t[:, 0] == t[:, 1])
    leaf = _leaf_of(nodes, tri.shape[0])
    across = tied & (leaf[ids[:, 0]] != leaf[np.maximum(ids[:, 1], 0)])
    higher = across & (ids[:, 0] > ids[:, 1])
    print("%s: of %d tie rays, tied at the nearest hit %.3f, partners in different leaves %.3f, and the winner has the higher index %.3f"
          % (name, tied.size, tied.mean(), across.mean(), higher.mean()))
    assert tied.mean() >= TIES_AT_LEAST[name]
    if name == "median1":
        assert higher.mean() >= 0.5                                    # where "the lower index wins" is the wrong answer
    if name == "chain":
        assert across.mean() >= 0.3


def test_the_ray_contract_differs_from_the_point_queries_on_triangles_that_no_leaf_holds(oracle):
    """A ray sees the triangles below a leaf and no others: for a share of the rays aimed at the uncovered triangles, a brute force
    over ALL triangles has an uncovered one nearest while hitBVH on the caller's tree answers another distance (or a miss)."""
    tri, nodes, expect = T.shape("uncovered")
    Q, X = T.ray_queries("uncovered"), T.ray_expected(oracle, "uncovered")
    on = Q["on_uncovered"]
    table = T.AE._tables(oracle, tri, nodes, Q["rays"][on])[1]         # hitTriangle's t of every triangle, EZ_INF: no hit
    nearest = table.argmin(1)
    differs = np.isin(nearest, expect["uncovered"]) & (table.min(1) < T.MISS_T) & (table.min(1) != X["closest.t"][on])
    print("uncovered: %d of %d aimed rays have an uncovered triangle nearest and another answer from the tree" % (differs.sum(), differs.size))
    assert differs.size == 128 and differs.sum() >= 32
    assert not np.isin(X["all64.tri"], expect["uncovered"]).any()     # no list names a triangle that no leaf holds


def test_the_chain_rays_leave_entries_pending_on_the_callers_nodes(oracle):
    tri, nodes, expect = T.shape("chain")
    Q = T.ray_queries("chain")
    depth = {}
    for key in ("deep", "shallow"):
        rays = Q["rays"][Q[key]]
        assert (rays[:, 4:] == 0).all() and (np.abs(rays[:, 3]) == 1).all()   # parallel to x
        depth[key] = T.pending_depth(nodes, T.AE._tables(oracle, tri, nodes, rays)[0])
        assert np.array_equal(depth[key], T.pending_depth(nodes, T.slab(rays, nodes)))   # (the numpy slab test that chose them agrees)
    both = np.concatenate([depth["deep"], depth["shallow"]])
    print("chain: deepest pending count %d from the deep end, %d from the shallow end; %d rays at 40 or more"
          % (depth["deep"].max(), depth["shallow"].max(), (both >= 40).sum()))
    assert (both >= 40).sum() >= 16 and both.max() <= expect["depth"] - 1


# ---- the frames of tests/test_gpu_tree_shapes_frames.py: conditions on the inputs, on the CPU oracle alone -- the small frame (64 x 48,
# 4 spp, 3 bounces, synthetic_hdr(64, 32) with its cache, integrators 50 and 51) hits the shape and reaches the last bounce, holds no NaN,
# shows which of two byte-identical triangles won, shows that the uncovered triangles are never seen, and does not depend on the tree
# where the leaves hold the same triangles.  These are conditions, not measurements of the code under test.

FRAME_INTEGRATORS = (50, 51)
TINY = ("root_leaf_1", "root_leaf_8", "two_leaves")
WITH_COPIES = [n for n in T.HOST_SHAPES if n not in TINY]
_frames = {}


def _oracle_scene(oracle, arrays):
    so = oracle.scene_create(*arrays)
    so.set_env(*T.frame_env())
    return so


def _frame(oracle, key, arrays, name, integ):
    """the oracle's small frame of `arrays` with the camera of `name`, rendered once"""
    if (key, name, integ) not in _frames:
        _frames[(key, name, integ)] = _oracle_scene(oracle, arrays).render(T.frame_params(name, integ))
    return _frames[(key, name, integ)]


def test_a_copy_never_carries_its_originals_material():
    for name in T.HOST_SHAPES:
        tri, nodes = T.coloured(name)
        plain = T.shape(name)[0]
        assert np.array_equal(tri[:, :18], plain[:, :18]) and nodes is T.shape(name)[1] and not tri.flags.writeable
        pairs = T.copy_pairs(tri)
        assert pairs.shape[0] == (0 if name in TINY else 24 if name == "chain" else T.N_DUPLICATES), name
        assert (tri[pairs[:, 0], 18:36] != tri[pairs[:, 1], 18:36]).any(1).all(), name      # the point of the function
        sw = T.swapped(name)[0]
        assert np.array_equal(sw[pairs[:, 0], 18:36], tri[pairs[:, 1], 18:36]) and np.array_equal(sw[pairs[:, 1], 18:36], tri[pairs[:, 0], 18:36])
        rest = np.setdiff1d(np.arange(tri.shape[0]), pairs)
        assert np.array_equal(sw[rest], tri[rest]) and np.array_equal(sw[:, :18], tri[:, :18])
        if tri.shape[0] > 8:
            base_colour = np.unique(tri[:, 21:24], axis=0).shape[0]
            varied = (tri[:, 24:36] != plain[:, 24:36]).any(1).mean()                          # roughness, metallic, specular, clearcoat, anisotropy
            lights = (tri[:, 18:21] > 0).any(1).mean()
            print("%s: %d base colours of %d triangles, %.3f with varied lobes, %.3f emissive" % (name, base_colour, tri.shape[0], varied, lights))
            assert base_colour == tri.shape[0] and 0.15 <= varied <= 0.35 and 1 / 32 <= lights <= 1 / 8
    assert set(T.CAMERAS) == set(T.HOST_SHAPES + T.LBVH_SHAPES)


@pytest.mark.parametrize("name", T.HOST_SHAPES)
def test_the_frames_hit_the_shape_reach_the_last_bounce_and_hold_no_nan(oracle, name):
    so = _oracle_scene(oracle, T.coloured(name))
    for integ in FRAME_INTEGRATORS:
        hit, last = [], []
        for frame in range(T.FRAME_SPP):                               # the samples of the small frame, one audit each
            ids = so.render_paths(T.frame_params(name, integ, spp=1, frame0=frame), want_colour=False)[0]
            ids = ids.reshape(T.FRAME_W * T.FRAME_H, -1)
            hit.append((ids[:, 0] >= 0).mean())
            last.append(int((ids[:, -1] >= -1).sum()))                 # (-2: the slot was never traced)
        print("%s, integrator %d: primary rays that hit %.2f .. %.2f, paths at the last bounce %d .. %d of %d"
              % (name, integ, min(hit), max(hit), min(last), max(last), T.FRAME_W * T.FRAME_H))
        if name == "root_leaf_1":
            assert min(hit) > 0.05
        else:
            assert min(hit) >= 0.7 and min(last) >= (20 if name in TINY else 100)
        f = _frame(oracle, "coloured", T.coloured(name), name, integ)
        assert not np.isnan(f).any() and float(f[..., :3].max()) > 0.1


@pytest.mark.parametrize("name", WITH_COPIES)
def test_the_tie_winner_shows_in_the_frame(oracle, name):
    """coloured against swapped: the two frames differ only where a path met an original or its copy -- a renderer that lets the
    wrong one of the two win draws the swapped frame."""
    for integ in FRAME_INTEGRATORS:
        a = _frame(oracle, "coloured", T.coloured(name), name, integ)
        b = _frame(oracle, "swapped", T.swapped(name), name, integ)
        differ = int((~T.same_pixels(a, b)).sum())
        print("%s, integrator %d: %d of %d pixels (%.1f %%) depend on the winner of a tie" % (name, integ, differ, a.shape[0] * a.shape[1],
                                                                                          100.0 * differ / (a.shape[0] * a.shape[1])))
        assert differ >= 0.02 * a.shape[0] * a.shape[1]


def test_the_uncovered_triangles_show_in_the_frame(oracle):
    """Uniform materials (the two arrays order the triangles differently): the frame of `uncovered` against the same triangles under
    a tree that covers all of them."""
    tri, nodes = T.covered_again()
    assert T.check_valid(tri, nodes)["uncovered"].size == 0
    key = lambda a: sorted(a[k].tobytes() for k in range(a.shape[0]))  # noqa: E731
    assert key(tri) == key(T.shape("uncovered")[0])
    for integ in FRAME_INTEGRATORS:
        a = _frame(oracle, "plain", T.shape("uncovered")[:2], "uncovered", integ)
        b = _frame(oracle, "covered_again", (tri, nodes), "uncovered", integ)
        differ = int((~T.same_pixels(a, b)).sum())
        print("uncovered, integrator %d: %d of %d pixels (%.1f %%) differ from the frame of a tree that covers every triangle"
              % (integ, differ, a.shape[0] * a.shape[1], 100.0 * differ / (a.shape[0] * a.shape[1])))
        assert differ >= 0.03 * a.shape[0] * a.shape[1]


def test_the_tree_alone_changes_no_pixel(oracle):
    """Uniform materials: loose boxes, a leaf box that misses a vertex and leaves of one triangle hold the triangles that sah8's
    leaves hold -- the frames are sah8's on the bits (a tie's two partners carry one material here)."""
    for integ in FRAME_INTEGRATORS:
        want = _frame(oracle, "plain", T.shape("sah8")[:2], "sah8", integ)
        for name in ("loose", "leaf_misses", "median1"):
            assert T.CAMERAS[name] == T.CAMERAS["sah8"]
            differ = int((~T.same_pixels(_frame(oracle, "plain", T.shape(name)[:2], name, integ), want)).sum())
            print("%s, integrator %d: %d pixels differ from sah8's frame" % (name, integ, differ))
            assert differ == 0


@pytest.mark.parametrize("name", ["median1", "leaf128", "chain"])
def test_the_frames_meet_ties_whose_partners_lie_in_different_leaves(oracle, name):
    """Where a leaf parts an original from its copy, "the lower index wins" is no rule: the audited frames (integrators 50 and 51, frames
    0 and 7) have ray slots that go to the copy -- the higher index -- of such a pair, and slots that go to the original."""
    tri, nodes = T.coloured(name)
    leaf = _leaf_of(nodes, tri.shape[0])
    pairs = T.copy_pairs(tri)
    across = pairs[leaf[pairs[:, 0]] != leaf[pairs[:, 1]]]
    so = _oracle_scene(oracle, (tri, nodes))
    to_copy = to_original = 0
    for integ in FRAME_INTEGRATORS:
        for frame in (0, 7):
            ids = so.render_paths(T.frame_params(name, integ, spp=1, frame0=frame), want_colour=False)[0]
            to_copy += int(np.isin(ids, across[:, 1]).sum())
            to_original += int(np.isin(ids, across[:, 0]).sum())
    print("%s: %d of %d pairs lie across leaves; %d ray slots of the audited frames go to their copies, %d to their originals"
          % (name, across.shape[0], pairs.shape[0], to_copy, to_original))
    assert across.shape[0] >= 3 and to_copy >= 20 and to_original >= 20

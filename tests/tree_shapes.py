"""Tree shapes a caller can pass to scene_create, and the queries and expected answers of the point and overlap queries on them
(tests/test_tree_shapes.py on the CPU, tests/test_gpu_tree_shapes.py on the device; a helper, no test).

The thirteen query kernels run on two walks over the 4-wide records (ezrt_point_queries.h: point_walk, slot_walk) and promise an
answer that does not depend on the tree.  The other GPU tests create their scenes from host SAH trees with leaves of 4 or 8; the
shapes here are what such trees never are -- and every one is a pair of arrays that ezrt_scene_create accepts (check_valid).

The base set (base(), 1 209 triangles, every coordinate a multiple of 1/4): the closed voxel solid of tests/inside_scenes.py four
times -- at the origin, translated by (0.5, 0.5, 0.5) so that the two cut each other, and that pair again 8 further along x --, the
defect triangles of tests/self_overlap_scenes.py (twin, fold, fan, blades) and 48 exact duplicates of triangles of the solids: ties
for the point queries, s = 3 pairs for the self-overlap.

shape(name) -> (tri [n, 36], nodes [m, 12], expect); expect["walk"] says whether the pruned route must run, expect["retree"] what
prune_info()["retreed"] must be (None: not asserted), the other entries are facts of the shape:

  sah8          the control: buildBVHwithSAH(8)
  median1       buildBVH(1): every leaf one triangle (count field 0), 1 208 inner nodes
  leaf128       leaves of exactly 128 triangles (count field 0x7f): the host SAH with leaf_n = 128 where it makes one, else nodes
                built by hand over runs of 128 of the triangles sorted along x
  chain         62 inner nodes, inner node k with a leaf on the left and inner node k + 1 on the right, the last with two leaves:
                depth 63, the deepest that scene_create accepts.  63 leaves of 1, 2 .. 8, 1, 2 .. triangles (280 in all) over a
                strip of the base set sorted along x.  Created with EZRT_RETREE=0 and with 1 (expect["retree_settings"]).
                With the re-tree off the records are a collapse of these very nodes (ezrt_scene_build.hip, "a record per reachable
                cut root"): the cut of inner node k starts as {leaf k, inner k + 1}, splits its only inner slot twice and ends as
                {leaf k, leaf k + 1, leaf k + 2, inner k + 3}, m = 4 -- so the records are rooted at inner nodes 0, 3 .. 57 (20 of
                them) and at inner node 60, whose cut {leaf 60, inner 61} splits once into the three leaves 60, 61, 62 (m = 3, no
                inner slot left).  stack_need_cp = the fold of (m - 1 + deepest child) = 20 * 3 + 2 = 62 pending entries: a stack
                column of (62 + 1) * 2 * 64 * 4 B = 32 256 B of LDS per wave for point_walk.
  root_leaf_1, root_leaf_8   the root is a leaf (nodes.shape[0] == 2): no inner node, no records, swept
  two_leaves    a root with leaves of 3 and 5 triangles: one record with two unused slots
  uncovered     sah8 over the base set without 37 of its triangles, which are appended behind the builder's array and are in no
                leaf; one leaf in the middle of the node array has its n reduced by 2 and keeps its box: 39 triangles that only
                the sweeps behind the walks reach (expect["uncovered"]).  12 of the 37 are duplicates of covered triangles, which
                have lower indices; the other 25 are faces of the solids.
  loose         sah8 with every face of every box moved outwards by a random amount, then made nested again bottom-up
  leaf_misses   sah8 with one leaf's BB.x one ulp below a vertex it holds: still nested, but the scene does not prune -- swept
  lbvh1, lbvh3  build.build_lbvh(base, 1 or 3): the device builder's trees; they need the device, shape() builds them on demand

queries(tri, nodes, seed, expect) -> dict: 257 points, boxes and triangles (a full wave and a partial one in every launch) from the
generators of the other tests, and per shape: for `chain` 16 points beyond the deep end of the strip -- every record's inner slot is
then the nearest, so the walk goes down first and leaves the three leaves of each record pending -- and a box over the whole scene;
for `uncovered` 32 points, boxes and triangles on the uncovered triangles; for every shape of more than 8 triangles 8 tie points
(_tie_points: the distance, the radius and the lb of the winner's box are one float32), for the others 40 points next to their
triangles (_points_next_to: crossings that are not zero).

expected(tri, Q) -> dict name -> array: every query of the GPU test by the numpy restatements (tests/*_expected.py) over ALL
triangles; the entries that begin with "_" are inputs derived from answers (the d_max arrays, the id subset)."""
import numpy as np

import box_overlap_expected as BE
import box_overlap_scenes as BS
import closest_point_expected as E
import inside_expected as IE
import inside_scenes as IS
import nearest_expected as NE
import self_overlap_expected as SE
import self_overlap_scenes as SS
import tri_overlap_expected as TE
import tri_overlap_scenes as TS

from ezrt_amd import scene as S

F = np.float32
HOST_SHAPES = ("sah8", "median1", "leaf128", "chain", "root_leaf_1", "root_leaf_8", "two_leaves", "uncovered", "loose", "leaf_misses")
LBVH_SHAPES = ("lbvh1", "lbvh3")
SEEDS = dict(sah8=11, median1=12, leaf128=13, chain=14, root_leaf_1=15, root_leaf_8=16, two_leaves=17, uncovered=18, loose=19,
             leaf_misses=20, lbvh1=21, lbvh3=22)
N_QUERIES = 257
N_SOLIDS = 4
N_DUPLICATES = 48
N_CHAIN_INNER = 62
N_APPENDED = 37
N_APPENDED_DUPLICATES = 12
N_TIES = 8
N_NEAR = 40

_cache = {}


# ---- the base set

def _base_vertices():
    """(P float32 [n, 3, 3], first index of the duplicates, the index each duplicate copies)"""
    b = IS.boundary_triangles(IS.occupancy())
    solids = [b, b + SS.SHIFT, b + F([8, 0, 0]), b + F([8, 0, 0]) + SS.SHIFT]
    plain = np.concatenate(solids + [np.roll(b[:1], 1, axis=1), SS._defects()]).astype(F)
    n_solid = N_SOLIDS * b.shape[0]
    of = np.random.default_rng(7).permutation(n_solid)[:N_DUPLICATES]
    P = np.concatenate([plain, plain[of]]).astype(F)
    assert np.array_equal(P * 4, np.round(P * 4))
    return P, plain.shape[0], of


def base():
    """float32 [1209, 36]: the base set, in construction order (solids, twin, defects, duplicates)"""
    if "base" not in _cache:
        _cache["base"] = IS.tri36(_base_vertices()[0])
    return _cache["base"]


# ---- node arrays

def vertices(tri):
    return np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)


def _host(T, sah, leaf):
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(T, F))
    (hs.buildBVHwithSAH if sah else hs.buildBVH)(leaf)
    return hs.encode()


def _leaf_row(P, index, n):
    v = P[index:index + n].reshape(-1, 3)
    return [0, 0, 0, n, index, 0, *v.min(0), *v.max(0)]


def nodes_over(P, runs):
    """float32 [m, 12]: a balanced tree, in pre-order, over the leaves `runs` = [(index, n), ...] of triangles P [*, 3, 3]; row 0 is
    the unused sentinel, row 1 the root"""
    rows = [[0.0] * 12]

    def make(lo, hi):
        i = len(rows)
        if hi - lo == 1:
            rows.append(_leaf_row(P, *runs[lo]))
            return i
        rows.append(None)
        mid = (lo + hi) // 2
        l, r = make(lo, mid), make(mid, hi)
        box = np.array([rows[l][6:], rows[r][6:]])
        rows[i] = [l, r, 0, 0, 0, 0, *box[:, :3].min(0), *box[:, 3:].max(0)]
        return i

    make(0, len(runs))
    return np.array(rows, F)


def _sorted_along_x(T):
    P = vertices(T)
    return T[np.lexsort((np.arange(P.shape[0]), P.mean(1)[:, 0]))]


def _leaf128():
    tri, nodes = _host(base(), True, 128)
    if not (nodes[1:, 3] == 128).any():
        tri = _sorted_along_x(base())
        n = tri.shape[0]
        nodes = nodes_over(vertices(tri), [(i, min(128, n - i)) for i in range(0, n, 128)])
    return tri, nodes, dict(walk=True, retree=None, n128=int((nodes[1:, 3] == 128).sum()))


def _chain():
    P, n_plain, _ = _base_vertices()
    c = P[:n_plain].mean(1)
    strip = np.nonzero((c[:, 1] >= 3.0) & (c[:, 1] < 4.5))[0]                      # a strip along x, through all four solids
    strip = strip[np.lexsort((strip, c[strip, 0]))]
    sizes = [1 + k % 8 for k in range(N_CHAIN_INNER + 1)]
    n = sum(sizes)                                                                  # 280
    strip = strip[np.linspace(0, strip.size - 1, n - 24).astype(int)]             # thinned evenly to 256 ...
    assert np.unique(strip).size == n - 24
    T = base()[np.concatenate([strip, strip[5::10][:24]])]                          # ... and 24 of them again: ties
    tri = _sorted_along_x(T)                                                        # (a duplicate comes right behind its original)
    Q = vertices(tri)
    first = np.concatenate([[0], np.cumsum(sizes)])
    lo = np.stack([Q[first[k]:].reshape(-1, 3).min(0) for k in range(len(sizes))])  # the box of leaves k ..
    hi = np.stack([Q[first[k]:].reshape(-1, 3).max(0) for k in range(len(sizes))])
    nodes = np.zeros((1 + 2 * N_CHAIN_INNER + 1, 12), F)
    for k in range(N_CHAIN_INNER):
        i = 1 + 2 * k                                                               # inner node k, followed by its left leaf
        nodes[i] = [i + 1, i + 2, 0, 0, 0, 0, *lo[k], *hi[k]]
        nodes[i + 1] = _leaf_row(Q, first[k], sizes[k])
    nodes[2 * N_CHAIN_INNER + 1] = _leaf_row(Q, first[-2], sizes[-1])
    return tri, nodes, dict(walk=True, retree=None, retree_settings=(0, 1), depth=N_CHAIN_INNER + 1, stack_need_cp=62, chain=True)


def _crossing_pairs(n_pairs):
    """indices into base(): n_pairs disjoint pairs of triangles that cross each other"""
    if "cross_base" not in _cache:
        _cache["cross_base"] = SE.crosses(base())
    cross = _cache["cross_base"]
    out, used = [], set()
    for i in range(0, cross.shape[0], 29):
        k = [int(j) for j in np.nonzero(cross[i])[0] if j not in used]
        if i not in used and k and len(out) < 2 * n_pairs:
            out += [i, k[0]]
            used |= {i, k[0]}
    assert len(out) == 2 * n_pairs
    return np.array(out)


def _small(sizes):
    n = sum(sizes)
    T = base()[:1] if n == 1 else base()[_crossing_pairs(n // 2)]
    tri = np.ascontiguousarray(T, F)
    first = np.concatenate([[0], np.cumsum(sizes)])
    nodes = nodes_over(vertices(tri), [(int(first[k]), sizes[k]) for k in range(len(sizes))])
    walk = len(sizes) > 1
    return tri, nodes, dict(walk=walk, retree=None, records4=None if walk else 0)


def _uncovered():
    P, n_plain, of = _base_vertices()
    b = n_plain - 9                                                                 # the faces of the solids
    rng = np.random.default_rng(23)
    dup = n_plain + rng.permutation(N_DUPLICATES)[:N_APPENDED_DUPLICATES]           # duplicates: their originals stay covered
    free = np.setdiff1d(np.arange(b), of)                                           # faces that nothing duplicates
    face = rng.permutation(free)[:N_APPENDED - N_APPENDED_DUPLICATES]
    gone = rng.permutation(np.concatenate([dup, face]))
    keep = np.setdiff1d(np.arange(P.shape[0]), gone)
    tri, nodes = _host(base()[keep], True, 8)
    n_cov = tri.shape[0]
    tri = np.ascontiguousarray(np.concatenate([tri, base()[gone]]), F)
    V = vertices(tri)
    first_copy = {V[k].tobytes(): k for k in range(n_cov - 1, -1, -1)}              # the lowest covered index of each triangle
    leaves = [i for i in range(1, nodes.shape[0]) if nodes[i, 3] >= 3]
    leaves = leaves[len(leaves) // 2:]
    cut = [i for i in leaves                                                        # a leaf whose last two triangles nothing copies
           if not any(first_copy.get(V[t].tobytes(), -1) in (int(nodes[i, 4] + nodes[i, 3]) - 2, int(nodes[i, 4] + nodes[i, 3]) - 1)
                      for t in range(n_cov, tri.shape[0]))][0]
    nodes = nodes.copy()
    nodes[cut, 3] -= 2                                                              # its box stays: a superset, still valid
    end = int(nodes[cut, 4] + nodes[cut, 3])
    unc = np.concatenate([[end, end + 1], np.arange(n_cov, tri.shape[0])]).astype(np.int32)
    copies = np.array([t for t in range(n_cov, tri.shape[0]) if V[t].tobytes() in first_copy], np.int32)
    return tri, nodes, dict(walk=True, retree=None, uncovered=unc, cut_leaf=cut, n_covered_by_builder=n_cov, copies=copies,
                            originals=np.array([first_copy[V[t].tobytes()] for t in copies], np.int32))


def _loose():
    tri, nodes = _host(base(), True, 8)
    nodes = nodes.copy()
    rng = np.random.default_rng(31)
    m = nodes.shape[0]
    nodes[1:, 6:9] -= rng.uniform(0.0, 0.5, (m - 1, 3)).astype(F) * (rng.random((m - 1, 3)) < 0.8)   # some faces stay tight
    nodes[1:, 9:12] += rng.uniform(0.0, 0.5, (m - 1, 3)).astype(F) * (rng.random((m - 1, 3)) < 0.8)
    for i in range(m - 1, 0, -1):                                                   # children have higher ids: bottom-up
        if nodes[i, 3] == 0:
            l, r = int(nodes[i, 0]), int(nodes[i, 1])
            nodes[i, 6:9] = np.minimum(nodes[i, 6:9], np.minimum(nodes[l, 6:9], nodes[r, 6:9]))
            nodes[i, 9:12] = np.maximum(nodes[i, 9:12], np.maximum(nodes[l, 9:12], nodes[r, 9:12]))
    return tri, nodes, dict(walk=True, retree=None)


def _leaf_misses():
    tri, nodes = _host(base(), True, 8)
    nodes = nodes.copy()
    leaves = [i for i in range(1, nodes.shape[0]) if nodes[i, 3] > 0]
    i = leaves[len(leaves) // 2]
    v = vertices(tri)[int(nodes[i, 4]):int(nodes[i, 4] + nodes[i, 3])]
    nodes[i, 9] = np.nextafter(v[:, :, 0].max(), F(-np.inf), dtype=F)
    return tri, nodes, dict(walk=False, retree=None, mode=-1, missing_leaf=i)


def _lbvh(leaf):
    from ezrt_amd import build
    tri, nodes = build.build_lbvh(base(), leaf)[:2]
    return np.ascontiguousarray(tri, F), np.ascontiguousarray(nodes, F), dict(walk=True, retree=None, max_leaf=leaf)


def shape(name):
    """(tri [n, 36], nodes [m, 12], expect) of the named shape, built once"""
    if name not in _cache:
        if name == "sah8":
            made = _host(base(), True, 8) + (dict(walk=True, retree=1),)
        elif name == "median1":
            made = _host(base(), False, 1) + (dict(walk=True, retree=None, max_leaf=1),)
        elif name == "leaf128":
            made = _leaf128()
        elif name == "chain":
            made = _chain()
        elif name == "root_leaf_1":
            made = _small([1])
        elif name == "root_leaf_8":
            made = _small([8])
        elif name == "two_leaves":
            made = _small([3, 5])
        elif name == "uncovered":
            made = _uncovered()
        elif name == "loose":
            made = _loose()
        elif name == "leaf_misses":
            made = _leaf_misses()
        else:
            assert name in LBVH_SHAPES, name
            made = _lbvh(int(name[4:]))
        tri, nodes, expect = made
        tri, nodes = np.ascontiguousarray(tri, F), np.ascontiguousarray(nodes, F)
        tri.setflags(write=False)
        nodes.setflags(write=False)
        _cache[name] = (tri, nodes, expect)
    return _cache[name]


# ---- what ezrt_scene_create asks of caller arrays, and what the records will reach

def check_valid(tri, nodes):
    """Asserts that scene_create accepts the arrays -- parent < child < m, leaf ranges inside the triangle array, depth <= 63,
    leaf <= 128 -- and returns dict(depth, max_leaf, n_leaves, nested, holds, uncovered): the facts of the reachable tree."""
    n_tri, m = tri.shape[0], nodes.shape[0]
    V = vertices(tri)
    assert nodes.dtype == F and nodes.shape[1] == 12 and m >= 2
    depth = np.zeros(m, int)
    depth[1] = 1
    held = np.zeros(n_tri, int)
    nested = holds = True
    leaves = []
    for i in range(1, m):
        n, index = int(nodes[i, 3]), int(nodes[i, 4])
        if n > 0:
            assert nodes[i, 3] == n and nodes[i, 4] == index and 0 <= index and index + n <= n_tri and n <= 128, i
            if depth[i]:
                leaves.append(n)
                held[index:index + n] += 1
                v = V[index:index + n].reshape(-1, 3)
                holds &= bool((v >= nodes[i, 6:9]).all() and (v <= nodes[i, 9:12]).all())
        else:
            l, r = int(nodes[i, 0]), int(nodes[i, 1])
            assert nodes[i, 0] == l and nodes[i, 1] == r and i < l < m and i < r < m, i
            if depth[i]:
                for c in (l, r):
                    assert depth[c] == 0, "node %d has two parents" % c
                    depth[c] = depth[i] + 1
                    if i > 1:                                                      # (the root's own box is never tested)
                        nested &= bool((nodes[c, 6:9] >= nodes[i, 6:9]).all() and (nodes[c, 9:12] <= nodes[i, 9:12]).all())
    assert depth.max() <= 63
    assert held.max() <= 1, "a triangle in two leaves"
    return dict(depth=int(depth.max()), max_leaf=max(leaves), n_leaves=len(leaves), nested=nested, holds=holds,
                uncovered=np.nonzero(held == 0)[0].astype(np.int32))


# ---- the queries

def box_lb(p, lo, hi):
    """float32: closest_point_box of point_walk -- the squared distance of p to the box [lo, hi], in the kernel's order of operations"""
    g = np.maximum(np.maximum(lo - p, p - hi), F(0)).astype(F)
    return ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]).astype(F) + g[..., 2] * g[..., 2]).astype(F)


def _tie_points(tri, n):
    """(points [n, 3], h [n]): points at h = 1/4 or 1/2 straight off the inside of an axis-aligned triangle, kept where that
    triangle's plane is the nearest thing: every coordinate is a multiple of 1/16, so the distance h, the radius h * h that d_max = h
    gives, the winner's dist2 and the lb of the winner's own bounding box are one float32 on the bits.  A walk that skips a box at
    lb == radius instead of descending it loses these winners.  Triangles that have an exact copy come first: with leaves of one
    triangle the two copies are in different leaves, both at lb == radius."""
    V = vertices(tri)
    seen, copied = {}, []
    for t in range(V.shape[0]):
        first = seen.setdefault(V[t].tobytes(), t)
        if first != t:
            copied.append(first)
    order = np.concatenate([np.array(copied, int), np.setdiff1d(np.arange(V.shape[0]), copied)[::7]])
    order = np.array([t for t in order if (V[t] == V[t, :1]).all(0).sum() == 1][:160])
    axis = np.array([int(np.argmax((V[t] == V[t, :1]).all(0))) for t in order])
    q = (V[order, 0] * F(0.5) + V[order, 1] * F(0.25) + V[order, 2] * F(0.25)).astype(F)
    found, hs = [], []
    for h in (0.25, -0.25, 0.5, -0.5):
        p = q.copy()
        p[np.arange(order.size), axis] += F(h)
        win, _, dist = E.closest_point(p, tri)[:3]
        ok = (dist == F(abs(h))) & (box_lb(p, V[win].min(1), V[win].max(1)) == F(h * h)) & (win == order)
        found.append(p[ok][:n // 4])
        hs.append(np.full(found[-1].shape[0], abs(h), F))
    found, hs = np.concatenate(found), np.concatenate(hs)
    assert found.shape[0] == n, found.shape
    return found, hs


def _points_next_to(V, n):
    """float32 [n, 3]: points 1/16 off the inside of the triangles V, along every axis at once: for a scene of a handful of
    triangles, where the other points' axis rays cross nothing -- a ray back along an axis that is not parallel to the triangle
    crosses it"""
    t = np.arange(n) % V.shape[0]
    w = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], F)[(np.arange(n) // V.shape[0]) % 3]
    q = (V[t] * w[:, :, None]).sum(1).astype(F)
    sign = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]], F)[np.arange(n) % 4]
    return (q + sign * F(0.0625)).astype(F)


def queries(tri, nodes, seed, expect=None):
    """dict: points [n, 3], lo, hi [n', 3], tris [n'', 9] (float32; the first 257 of each from the generators of the other tests),
    and the index ranges of the extras: deep (chain), on_uncovered (uncovered), ties with their distances tie_h (more than 8 triangles),
    near (8 triangles or fewer)"""
    expect = expect or {}
    V = vertices(tri)
    pts, first_bad = E.points_for(tri, nodes, seed)
    pts = np.concatenate([pts[:N_QUERIES - 16], pts[first_bad:first_bad + 16]])    # 16 of the points that are expected to miss
    lo, hi = (x[:N_QUERIES] for x in BS.boxes_for(tri, nodes, seed + 100))
    tris = TS.tris_for(tri, nodes, seed + 200)[:N_QUERIES]
    Q = dict(deep=slice(0, 0), on_uncovered=slice(0, 0), ties=slice(0, 0), near=slice(0, 0))
    rng = np.random.default_rng(seed + 300)
    if expect.get("chain"):
        flat = V.reshape(-1, 3)
        end, mid = flat.max(0), (flat.min(0) + flat.max(0)) * F(0.5)
        deep = np.stack([end[0] + rng.integers(1, 17, 16) * 0.25, mid[1] + rng.integers(-8, 9, 16) * 0.125,
                         mid[2] + rng.integers(-8, 9, 16) * 0.125], 1)
        Q["deep"] = slice(pts.shape[0], pts.shape[0] + 16)
        pts = np.concatenate([pts, deep.astype(F)])
        lo, hi = np.concatenate([lo, flat.min(0)[None]]), np.concatenate([hi, flat.max(0)[None]])
    if "uncovered" in expect:
        unc = expect["uncovered"]
        plain = np.setdiff1d(unc, expect["copies"])                               # first those that no covered triangle equals
        t = np.resize(np.concatenate([plain, expect["copies"]]), 32)
        w = rng.dirichlet((4, 4, 4), 32).astype(F)
        on = (V[np.resize(plain, 32)] * w[:, :, None]).sum(1).astype(F)           # (on a copy a point's winner is the covered original)
        Q["on_uncovered"] = slice(pts.shape[0], pts.shape[0] + 32)
        pts = np.concatenate([pts, on])
        lo, hi = np.concatenate([lo, V[t].min(1)]), np.concatenate([hi, V[t].max(1)])
        tris = np.concatenate([tris, np.roll(V[t], 1, axis=1).reshape(-1, 9)])
    if V.shape[0] > 8:
        at, h = _tie_points(tri, N_TIES)
        Q["ties"], Q["tie_h"] = slice(pts.shape[0], pts.shape[0] + N_TIES), h
        pts = np.concatenate([pts, at])
    else:
        Q["near"] = slice(pts.shape[0], pts.shape[0] + N_NEAR)
        pts = np.concatenate([pts, _points_next_to(V, N_NEAR)])
    Q.update(points=np.ascontiguousarray(pts, F), lo=np.ascontiguousarray(lo, F), hi=np.ascontiguousarray(hi, F),
             tris=np.ascontiguousarray(tris, F), seed=seed, select=expect.get("uncovered"))
    return Q


def shape_queries(name):
    if ("Q", name) not in _cache:
        tri, nodes, expect = shape(name)
        _cache[("Q", name)] = queries(tri, nodes, SEEDS[name], expect)
    return _cache[("Q", name)]


# ---- the expected answers

AXES = range(6)
NEAREST = ((1, False), (1, True), (5, False), (5, True))
OVERLAP_K = (0, 8, 64)


def id_subset(n_tri, seed, select=None):
    """a shuffled subset of at most 200 triangle ids, `select` among them"""
    rng = np.random.default_rng(seed + 400)
    ids = rng.permutation(n_tri)[:200]
    if select is not None:
        ids[:len(select)] = select
        ids = np.unique(ids)
    return np.ascontiguousarray(rng.permutation(ids), np.int32)


def closest_point_at(points, tri, ids):
    """(point [n, k, 3], dist [n, k], bary [n, k, 2]) of ids [n, k]: what ezrt_closest_point_at_device writes"""
    V = vertices(tri)
    n, k = ids.shape
    point, dist, bary = np.zeros((n, k, 3), F), np.full((n, k), np.inf, F), np.zeros((n, k, 2), F)
    for j in range(k):
        t = np.clip(ids[:, j], 0, V.shape[0] - 1)
        with np.errstate(all="ignore"):
            q, v, w, dd = (x[:, 0] for x in E.per_triangle(points[:, None, :], V[t, None, 0], V[t, None, 1], V[t, None, 2]))
            ok = (ids[:, j] >= 0) & np.isfinite(dd)
            point[:, j] = np.where(ok[:, None], q, 0)
            bary[:, j] = np.where(ok[:, None], np.stack([v, w], 1), 0)
            dist[:, j] = np.where(ok, np.sqrt(np.where(ok, dd, 0)), np.inf)
    return point, dist, bary


def expected(tri, Q, self_ids=None):
    """dict name -> array: the answers of every query of tests/test_gpu_tree_shapes.py (its `answers`), by the restatements; `self_ids`
    overrides the id subset of the self-overlap, for a comparison with another array's answers"""
    W = {}
    pts, n_tri = Q["points"], tri.shape[0]
    cp = E.closest_point(pts, tri)
    W["cp.tri"], W["cp.point"], W["cp.dist"], W["cp.bary"] = cp
    W["_d_max.cp"] = cp[2].copy()                                                  # the winner's own distance
    W["cpd.tri"], W["cpd.point"], W["cpd.dist"], W["cpd.bary"] = E.closest_point(pts, tri, W["_d_max.cp"])
    d2 = NE.dist2_all(pts, tri)
    third = NE.nearest(pts, tri, min(3, n_tri), d2=d2)[1][:, -1]                   # the distance of the third nearest: triangles AT the radius
    W["_d_max.near"] = np.where(np.arange(pts.shape[0]) % 4 == 3, F(0.75), third).astype(F)
    W["_d_max.near"][Q["ties"]] = cp[2][Q["ties"]]                                 # the tie points: boxes AT the radius
    for k, count in NEAREST:
        ids, dist, cnt = NE.nearest(pts, tri, k, W["_d_max.near"], d2=d2)
        W["near%d%d.tri" % (k, count)], W["near%d%d.dist" % (k, count)] = ids, dist
        if count:
            W["near%d%d.count" % (k, count)] = cnt
    W["near_all.tri"], W["near_all.dist"], W["near_all.count"] = NE.nearest(pts, tri, 5, None, d2=d2)
    W["near_at.point"], W["near_at.dist"], W["near_at.bary"] = closest_point_at(pts, tri, W["near51.tri"])
    crossings, inside = IE.all_axes(pts, tri)
    for axis in AXES:
        W["inside%d" % axis], W["crossings%d" % axis] = inside[axis], crossings[axis]
    W["sd.tri"], W["sd.point"], W["sd.bary"], W["sd.inside"] = cp[0], cp[1], cp[3], inside[0]
    W["sd.dist"] = (cp[2].view(np.uint32) | (inside[0].astype(np.uint32) << 31)).view(F)
    for key, over in (("box", BE.overlaps(Q["lo"], Q["hi"], tri)), ("trio", TE.overlaps(Q["tris"], tri))):
        rows, count = TE.lowest(over, 64)
        for k in OVERLAP_K:
            W["%s%d.tri" % (key, k)], W["%s%d.n" % (key, k)] = rows[:, :k], count
        W["%s_at" % key] = (rows[:, :8] >= 0).astype(np.uint8)
    at = (BE.at(np.repeat(Q["lo"], 8, 0), np.repeat(Q["hi"], 8, 0), tri, W["box8.tri"].reshape(-1)),
          TE.at(np.repeat(Q["tris"], 8, 0), tri, W["trio8.tri"].reshape(-1)))
    assert np.array_equal(at[0], W["box_at"].reshape(-1)) and np.array_equal(at[1], W["trio_at"].reshape(-1))
    cross = SE.crosses(tri)
    W["self8.tri"], W["self8.n"] = SE.rows_of(cross, None, 8)
    select = Q["select"]
    if select is not None:                                                         # with the uncovered triangles, 40 covered ones that cross them
        select = np.concatenate([select, np.setdiff1d(np.nonzero(cross[select].any(0))[0], select)[:40]])
    W["_ids"] = id_subset(n_tri, Q["seed"], select) if self_ids is None else self_ids
    for k in (0, 64):
        W["self_ids%d.tri" % k], W["self_ids%d.n" % k] = SE.rows_of(cross, W["_ids"], k)
    W["self_at"] = (W["self8.tri"] >= 0).astype(np.uint8)
    assert np.array_equal(SE.at(tri, np.repeat(np.arange(n_tri), 8), W["self8.tri"].reshape(-1)), W["self_at"].reshape(-1))
    return W


def shape_expected(name):
    if ("W", name) not in _cache:
        _cache[("W", name)] = expected(shape(name)[0], shape_queries(name))
    return _cache[("W", name)]


def differing(got, want):
    """the names of `want` (inputs aside) whose arrays differ from `got`'s: floats on the bits with NaN equal to NaN, the others by
    value and dtype kind"""
    bad = []
    for key in want:
        if key.startswith("_"):
            continue
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if b.dtype == F:
            a = np.ascontiguousarray(a, F)
            same = a.shape == b.shape and bool(np.all((a.view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
        else:
            same = a.shape == b.shape and a.dtype.kind in "iub" and np.array_equal(a.astype(np.int64), b.astype(np.int64))
        if not same:
            bad.append("%s (%d of %d)" % (key, int((a != b).sum()) if a.shape == b.shape else -1, b.size))
    return bad


# ---- the rays (tests/test_tree_shapes.py on the CPU, tests/test_gpu_tree_shapes_rays.py on the device)
#
# The ray contract is hitBVH on the CALLER's arrays: unlike the point and overlap queries above, the answer depends on the leaves --
# a triangle that no leaf holds is never seen, and of two triangles at one distance the one whose leaf the reference reaches first
# wins.  ray_queries(name) -> dict: rays [n, 6] (n = a whole number of waves plus one ray) and the index range of every part:
#   broad   257 rays of allhits_scenes.broad_rays (random, axis-parallel and one-zero-component rays with origins on vertex planes,
#           unnormalised directions, rays that are not tame); the scenes of 8 triangles or fewer, which such rays hit 4 to 9 % of the
#           time, get 257 near rays in their place, every eighth of them reversed (it leaves its triangle behind: the misses)
#   near    256 rays aimed at a random interior point (barycentrics >= 0.1: hitTriangle is strict, a point on an edge is a miss) of a
#           random triangle, in a random direction, from 0.05 to 0.6 in front of it
#   ties    128 rays aimed the same way at triangles that have a byte-identical copy (shapes of more than 8 triangles)
#   on_uncovered   128 rays aimed the same way at the triangles that no leaf holds (`uncovered`)
#   deep, shallow   64 + 32 rays parallel to x that enter the chain from beyond its deep and its shallow end, on the lines of a 1/8
#           grid (offset by 0.03: on no vertex plane) over the strip's y / z extent whose walk by the reference's rule leaves the most
#           entries pending on the caller's nodes (pending_depth)
#   pad     near rays up to the next whole number of waves plus one (`chain`: 641 + 96 = 737 rays, 32 more)
# ray_expected(oracle, name) -> dict name -> array: every answer of the GPU test from the CPU oracle's query_hits and the restated
# all-hits lists on the caller's arrays; the entries that begin with "_" are the t_max arrays derived from the answers.
import allhits_expected as AE  # noqa: E402
import allhits_scenes as AS  # noqa: E402
import test_surface_restatement as RS  # noqa: E402

N_BROAD, N_NEAR_RAYS, N_TIE_RAYS, N_ON_UNCOVERED, N_CHAIN_DEEP, N_CHAIN_SHALLOW = 257, 256, 128, 128, 64, 32
ALL_HITS_K = (64, 1, 2, 5)
SURFACE_FORMS = (3, 4, 50)
T_MAX = ("own", "below", "above", "second", "inf", "nan", "zero", "negative")
MISS_T = AE.EZ_INF


def copied(tri):
    """int [k]: the lowest index of every triangle that has a byte-identical copy in the array"""
    V, first, twice = vertices(tri), {}, set()
    for t in range(V.shape[0]):
        if first.setdefault(V[t].tobytes(), t) != t:
            twice.add(first[V[t].tobytes()])
    return np.array(sorted(twice), int)


def aimed_rays(V, ids, rng):
    """float32 [n, 6]: ray i crosses triangle ids[i] at an interior point, in a random direction, 0.05 to 0.6 from its origin"""
    n = len(ids)
    w = 0.1 + 0.7 * rng.dirichlet((1, 1, 1), n)
    p = (V[ids].astype(np.float64) * w[:, :, None]).sum(1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([p - d * rng.uniform(0.05, 0.6, (n, 1)), d], 1).astype(F)


def slab(rays, nodes):
    """float32 [n_rays, n_nodes]: hitAABB restated in numpy, for choosing rays only (the tests use the oracle's own table)"""
    with np.errstate(all="ignore"):
        S, inv = rays[:, None, :3], (F(1) / rays[:, 3:])[:, None, :]
        f, n = (nodes[None, :, 9:12] - S) * inv, (nodes[None, :, 6:9] - S) * inv
        t1, t0 = np.maximum(f, n).min(2), np.minimum(f, n).max(2)
        return np.where(t1 >= t0, np.where(t0 > 0, t0, t1), F(-1)).astype(F)


def pending_depth(nodes, A):
    """int [n_rays]: the most entries the reference's walk (near child first, ties right-first; allhits_expected.visit_lists) has
    pending on the nodes, per row of the hitAABB table A [n_rays, n_nodes]"""
    left, right, cnt = (nodes[:, k].astype(int).tolist() for k in (0, 1, 3))
    out = []
    for a in A.tolist():
        stack, deepest = [1], 0
        while stack:
            top = stack.pop()
            deepest = max(deepest, len(stack))
            if cnt[top] > 0:
                continue
            l, r = left[top], right[top]
            if a[l] > 0.0 and a[r] > 0.0:
                stack += [r, l] if a[l] < a[r] else [l, r]
            elif a[l] > 0.0 or a[r] > 0.0:
                stack.append(l if a[l] > 0.0 else r)
        out.append(deepest)
    return np.array(out)


def _chain_lines(V, nodes):
    """(deep [64, 6], shallow [32, 6]): the lines along x with the most entries pending, entered from either end"""
    flat = V.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    y, z = np.meshgrid(np.arange(lo[1] + 0.03, hi[1], 0.125), np.arange(lo[2] + 0.03, hi[2], 0.125), indexing="ij")
    out = []
    for x, dx, n in ((hi[0] + 1.0, -1.0, N_CHAIN_DEEP), (lo[0] - 1.0, 1.0, N_CHAIN_SHALLOW)):
        rays = np.zeros((y.size, 6), F)
        rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 3] = x, y.ravel(), z.ravel(), dx
        out.append(rays[np.argsort(-pending_depth(nodes, slab(rays, nodes)), kind="stable")[:n]])
    return out


def ray_queries(name):
    if ("R", name) not in _cache:
        tri, nodes, expect = shape(name)
        V, rng = vertices(tri), np.random.default_rng(SEEDS[name] + 500)
        parts, Q, n = [], {}, 0

        def add(key, rays):
            nonlocal n
            Q[key] = slice(n, n + rays.shape[0])
            parts.append(rays)
            n += rays.shape[0]

        near = lambda k: aimed_rays(V, rng.integers(0, V.shape[0], k), rng)  # noqa: E731
        if V.shape[0] > 8:
            add("broad", AS.broad_rays(tri, rng, N_BROAD))
        else:
            away = near(N_BROAD)
            away[::8, 3:] *= F(-1)                                                  # every eighth leaves its triangle behind: misses
            add("broad", away)
        add("near", near(N_NEAR_RAYS))
        twice = copied(tri)
        add("ties", aimed_rays(V, rng.choice(twice, N_TIE_RAYS), rng) if V.shape[0] > 8 else near(0))
        unc = expect.get("uncovered", np.zeros(0, int))
        plain = np.setdiff1d(unc, expect.get("copies", []))                       # first those that no covered triangle equals
        add("on_uncovered", aimed_rays(V, np.resize(np.concatenate([plain, plain, unc]), N_ON_UNCOVERED), rng) if unc.size else near(0))
        deep, shallow = _chain_lines(V, nodes) if expect.get("chain") else (near(0), near(0))
        add("deep", deep)
        add("shallow", shallow)
        add("pad", near(-(n - 1) % 64))
        Q["rays"] = np.ascontiguousarray(np.concatenate(parts), F)
        Q["rays"].setflags(write=False)
        assert Q["rays"].shape == (n, 6) and n % 64 == 1
        _cache[("R", name)] = Q
    return _cache[("R", name)]


def filtered(tri, t, t_max):
    """the contract's closest (tri, t) and occluded from the oracle's hits: tri >= 0 and t < t_max"""
    with np.errstate(invalid="ignore"):
        hit = (tri >= 0) if t_max is None else (tri >= 0) & (t < t_max)
    return np.where(hit, tri, -1).astype(np.int32), np.where(hit, t, MISS_T).astype(F), hit


def ray_lists(oracle, name):
    """the visit lists of the shape's rays (allhits_expected.visit_lists), computed once"""
    if ("V", name) not in _cache:
        tri, nodes, _ = shape(name)
        _cache[("V", name)] = AE.visit_lists(oracle, tri, nodes, ray_queries(name)["rays"])
    return _cache[("V", name)]


def ray_expected(oracle, name):
    if ("X", name) in _cache:
        return _cache[("X", name)]
    tri, nodes, _ = shape(name)
    rays = ray_queries(name)["rays"]
    n = rays.shape[0]
    to, do = oracle.scene_create(tri, nodes).query_hits(rays)
    visits = ray_lists(oracle, name)
    lists = AE.expected_all_hits(oracle, tri, nodes, rays, None, visits=visits)
    up, down = F(np.inf), F(-np.inf)
    X = {"_t_max.own": do.copy(), "_t_max.below": np.nextafter(do, down), "_t_max.above": np.nextafter(do, up),
         "_t_max.second": np.array([t[1] if t.size > 1 else (t[0] if t.size else F(1)) for ids, t in lists], F),
         "_t_max.inf": np.full(n, np.inf, F), "_t_max.nan": np.full(n, np.nan, F), "_t_max.zero": np.zeros(n, F),
         "_t_max.negative": -np.random.default_rng(SEEDS[name] + 600).uniform(0.0, 3.0, n).astype(F)}
    for key in (None,) + T_MAX:
        t_max = None if key is None else X["_t_max." + key]
        tag = "" if key is None else "[%s]" % key
        X["closest%s.tri" % tag], X["closest%s.t" % tag], X["occluded%s" % tag] = filtered(to, do, t_max)
        bounded = lists if key is None else AE.expected_all_hits(oracle, tri, nodes, rays, t_max, visits=visits)
        for K in ALL_HITS_K:
            X["all%d%s.tri" % (K, tag)], X["all%d%s.t" % (K, tag)], X["all%d%s.count" % (K, tag)] = AE.rows(bounded, K)
    for form in SURFACE_FORMS:
        X["surface%d.point" % form], X["surface%d.normal" % form], X["surface%d.inside" % form] = RS.restate(tri, rays, to, do, form >= 50)
    _cache[("X", name)] = X
    return X


# ---- the frames (tests/test_tree_shapes.py on the CPU, tests/test_gpu_tree_shapes_frames.py on the device)
#
# What a rendered frame of a shape needs.  Every triangle of the base set carries one material, so a frame of shape(name) could not
# show which of two byte-identical triangles won a tie.  coloured(name) gives every triangle a material of its own -- a copy never
# its original's --, swapped(name) exchanges the materials of every original and its copy (only for the CPU condition that the
# winner shows in the frame), CAMERAS has a camera per shape.
import zlib  # noqa: E402

# (eye, target) of the camera that looks at the shape.  The shapes over the base set share median1's but leaf128, which looks at the
# far pair of solids: its leaves of 128 part 3 of the 48 originals from their copies, and only there does a path meet such a pair (32
# ray slots of the audited frames go to the copy, 285 to the original).  The tiny shapes look at their handful of triangles from close by
_BASE_CAMERA = ((10.67, 6.67, 9.67), (6.67, 3.67, 3.67))
_TINY_CAMERA = ((1.78, 4.67, 2.38), (1.67, 5.0, 2.33))
CAMERAS = dict(chain=((3.5, 5.67, 6.67), (6.5, 3.67, 3.67)), median1=_BASE_CAMERA, leaf128=((14.67, 6.67, 7.67), (11.67, 4.17, 4.17)), root_leaf_8=_TINY_CAMERA,
               two_leaves=_TINY_CAMERA, sah8=_BASE_CAMERA, uncovered=_BASE_CAMERA, loose=_BASE_CAMERA, leaf_misses=_BASE_CAMERA,
               lbvh1=_BASE_CAMERA, lbvh3=_BASE_CAMERA, root_leaf_1=((2.28, 2.87, 2.57), (1.0, 2.67, 2.67)))
FRAME_W, FRAME_H, FRAME_SPP, FRAME_BOUNCES = 64, 48, 4, 3
EMISSIVE_ONE_IN, VARIED_ONE_IN = 16, 4


def _look_at(eye, target):
    """(eye, cameraRotate) of a camera at `eye` that looks at `target`: the columns of the rotation are right, up and back"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(f, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = right, np.cross(right, f), -f
    return eye.astype(np.float32), m.T.ravel().astype(np.float32)


def material_of(vertex_bytes, index):
    """float32 [18]: the material of triangle `index`, from a generator seeded with the triangle's bytes and its index -- so a
    byte-identical copy, which has another index, draws another material.  The base colour always varies; one triangle in 4 also
    draws roughness, metallic, specular, clearcoat and anisotropy (what integrator 52 samples), one in 16 is a light."""
    rng = np.random.default_rng([zlib.crc32(vertex_bytes), index])
    kind = rng.integers(0, 1 << 30)
    kw = dict(baseColor=tuple(float(x) for x in rng.uniform(0.1, 0.95, 3)))
    if kind % VARIED_ONE_IN == 0:
        kw.update(roughness=float(rng.uniform(0.2, 0.9)), metallic=float(rng.uniform(0.0, 0.9)), specular=float(rng.uniform(0.1, 0.9)),
                  clearcoat=float(rng.uniform(0.0, 1.0)), anisotropic=float(rng.uniform(0.0, 0.9)))
    if (kind // VARIED_ONE_IN) % EMISSIVE_ONE_IN == 0:
        kw.update(emissive=tuple(float(x) for x in rng.uniform(0.5, 4.0, 3)))
    return S.Material.disney(**kw).to18()


def copy_pairs(tri):
    """int [k, 2]: (original, copy) of every triangle that has a byte-identical copy at a higher index"""
    V, first, pairs = vertices(tri), {}, []
    for t in range(V.shape[0]):
        o = first.setdefault(V[t].tobytes(), t)
        if o != t:
            pairs.append((o, t))
    pairs = np.array(pairs, int).reshape(-1, 2)
    assert np.unique(pairs).size == pairs.size                                      # pairs, no triples: an exchange is well defined
    return pairs


def coloured(name):
    """(tri [n, 36], nodes): the shape's arrays with a material per triangle in columns 18:36; positions, normals and nodes are the
    shape's own.  The LBVH shapes colour the arrays the device builder returned."""
    if ("C", name) not in _cache:
        tri, nodes, _ = shape(name)
        V = vertices(tri)
        out = np.array(tri)
        for t in range(out.shape[0]):
            out[t, 18:36] = material_of(V[t].tobytes(), t)
        out.setflags(write=False)
        _cache[("C", name)] = (out, nodes)
    return _cache[("C", name)]


def swapped(name):
    """(tri, nodes): coloured(name) with the materials of every original and its copy exchanged"""
    if ("S", name) not in _cache:
        tri, nodes = coloured(name)
        out = np.array(tri)
        pairs = copy_pairs(tri)
        out[pairs[:, 0], 18:36], out[pairs[:, 1], 18:36] = tri[pairs[:, 1], 18:36], tri[pairs[:, 0], 18:36]
        out.setflags(write=False)
        _cache[("S", name)] = (out, nodes)
    return _cache[("S", name)]


def covered_again():
    """(tri, nodes): the triangle set of `uncovered` under a tree that covers all of it (buildBVHwithSAH(8) over the whole array)"""
    if "covered_again" not in _cache:
        _cache["covered_again"] = _host(shape("uncovered")[0], True, 8)
    return _cache["covered_again"]


def frame_env():
    """(hdr, cache) of the frames: synthetic_hdr(64, 32) and its importance cache"""
    if "env" not in _cache:
        from ezrt_amd import scenes
        hdr = scenes.synthetic_hdr(64, 32)
        _cache["env"] = (hdr, S.calculateHdrCache(hdr))
    return _cache["env"]


def frame_params(name, integ, w=FRAME_W, h=FRAME_H, spp=FRAME_SPP, bounces=FRAME_BOUNCES, frame0=0, camera=None, **kw):
    from ezrt_amd import trace
    return trace.make_params(w, h, *_look_at(*CAMERAS[camera or name]), integ, bounces, spp=spp, frame0=frame0,
                             env_clamp=10.0 if integ == 3 else 0.0, **kw)


def same_pixels(a, b):
    """bool [h, w]: the pixels of two frames that are equal on the bits in every channel"""
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(-1)

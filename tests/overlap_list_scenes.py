"""The constructed scene of the overlap-list tests (tests/test_gpu_overlap_list.py; a helper, no test): rows of an EXACT length.

A line of M disjoint triangles, triangle at position x = 0 .. M - 1 spanning [x - 1/4, x + 1/4] on x, 0 .. 1/2 on y, at z = 0.  The box
[-1/2, L - 1/2] on x (and [-1, 1] on y and z) touches exactly the L triangles at positions below L, whatever the tree.  The positions
are a fixed permutation of the ids, so a row's ids are not a range, and no traversal meets them in ascending order -- a tree built over
the line visits positions, not ids.  M is a few hundred more than the library's tile_max, so one row can be on either side of every
limit of ezrt_overlap_list_limits: kept sorted while it is filled, sorted in LDS, sorted in global memory.

line_scene(kind, M) -> (tri [M, 36], nodes) as scene_create takes them, under the trees a caller can pass (tests/tree_shapes.py builds
the same kinds over its own base set):
  sah8, median1   HostScene: buildBVHwithSAH(8), buildBVH(1) -- the builders reorder the triangles, ids follow the returned array
  leaf128         tree_shapes.nodes_over: a balanced tree over runs of 128 of the array sorted by position (ids then ARE in walk
                  order: the case in which an appended row is already sorted)
  runs5_shuffled  nodes_over: runs of 5 consecutive ids of the shuffled array -- every leaf box spans the whole line, the walk prunes
                  nothing, and leaf ranges are visited in an order that is neither id nor position order
  leaf_misses     sah8 with one leaf's box an ulp short of a vertex: the scene does not prune, the sweep route
  loose           sah8 with every face of every box moved outwards by a random amount, then made nested again bottom-up
  uncovered       sah8 over the line without 37 of its triangles, which are appended behind the builder's array and are in no leaf, and
                  one leaf with its n reduced by 2: 39 triangles that only the sweep behind the walk reaches
  lbvh3           build.build_lbvh(tri, 3): the device builder's tree (needs the device)"""
import numpy as np

import inside_scenes as IS
import tree_shapes as T

F = np.float32
KINDS = ("sah8", "median1", "leaf128", "runs5_shuffled", "leaf_misses", "loose", "uncovered", "lbvh3")
N_APPENDED = 37
_cache = {}


def line(M, seed=25):
    """float32 [M, 36]: triangle k of the array stands at position perm[k]"""
    pos = np.random.default_rng(seed).permutation(M).astype(F)
    P = np.zeros((M, 3, 3), F)
    P[:, 0, 0], P[:, 1, 0], P[:, 2, 0] = pos - F(0.25), pos + F(0.25), pos
    P[:, 2, 1] = 0.5
    return IS.tri36(P)


def position(tri):
    """int [M]: the position of every triangle of an array made by line_scene"""
    return np.ascontiguousarray(tri, F).reshape(-1, 36)[:, 6].astype(int)


def line_scene(kind, M):
    if (kind, M) not in _cache:
        tri = line(M)
        if kind == "sah8":
            made = T._host(tri, True, 8)
        elif kind == "median1":
            made = T._host(tri, False, 1)
        elif kind == "leaf128":
            tri = tri[np.argsort(position(tri))]
            made = tri, T.nodes_over(T.vertices(tri), [(i, min(128, M - i)) for i in range(0, M, 128)])
        elif kind == "runs5_shuffled":
            made = tri, T.nodes_over(T.vertices(tri), [(i, min(5, M - i)) for i in range(0, M, 5)])
        elif kind == "leaf_misses":
            tri, nodes = T._host(tri, True, 8)
            nodes = nodes.copy()
            leaves = [i for i in range(1, nodes.shape[0]) if nodes[i, 3] > 0]
            i = leaves[len(leaves) // 2]
            v = T.vertices(tri)[int(nodes[i, 4]):int(nodes[i, 4] + nodes[i, 3])]
            nodes[i, 9] = np.nextafter(v[:, :, 0].max(), F(-np.inf), dtype=F)
            made = tri, nodes
        elif kind == "loose":
            tri, nodes = T._host(tri, True, 8)
            nodes = nodes.copy()
            rng = np.random.default_rng(31)
            m = nodes.shape[0]
            nodes[1:, 6:9] -= rng.uniform(0.0, 0.5, (m - 1, 3)).astype(F) * (rng.random((m - 1, 3)) < 0.8)
            nodes[1:, 9:12] += rng.uniform(0.0, 0.5, (m - 1, 3)).astype(F) * (rng.random((m - 1, 3)) < 0.8)
            for i in range(m - 1, 0, -1):                                   # children have higher ids: bottom-up
                if nodes[i, 3] == 0:
                    l, r = int(nodes[i, 0]), int(nodes[i, 1])
                    nodes[i, 6:9] = np.minimum(nodes[i, 6:9], np.minimum(nodes[l, 6:9], nodes[r, 6:9]))
                    nodes[i, 9:12] = np.maximum(nodes[i, 9:12], np.maximum(nodes[l, 9:12], nodes[r, 9:12]))
            made = tri, nodes
        elif kind == "uncovered":
            gone = np.random.default_rng(23).permutation(M)[:N_APPENDED]
            keep = np.setdiff1d(np.arange(M), gone)
            covered, nodes = T._host(tri[keep], True, 8)
            nodes = nodes.copy()
            leaves = [i for i in range(1, nodes.shape[0]) if nodes[i, 3] >= 3]
            nodes[leaves[len(leaves) // 2], 3] -= 2                         # its box stays: a superset, still valid
            made = np.concatenate([covered, tri[gone]]), nodes
        else:
            assert kind == "lbvh3", kind
            from ezrt_amd import build
            made = build.build_lbvh(tri, 3)[:2]
        tri, nodes = np.ascontiguousarray(made[0], F), np.ascontiguousarray(made[1], F)
        assert sorted(position(tri)) == list(range(M))
        _cache[(kind, M)] = (tri, nodes)
    return _cache[(kind, M)]


def seam_lengths(insert_max, tile_max, M):
    """the row lengths at every seam, in the order of the issue: each once"""
    want = [0, 1, 2, 63, 64, 65, insert_max - 1, insert_max, insert_max + 1, tile_max - 1, tile_max, tile_max + 1, M]
    out = []
    for L in want:
        if 0 <= L <= M and L not in out:
            out.append(L)
    return out


def boxes(lengths):
    """(lo, hi) float32 [n, 3]: box i touches exactly the triangles at positions below lengths[i]"""
    L = np.asarray(lengths, np.float64)
    lo = np.tile(F([-0.5, -1, -1]), (L.size, 1))
    hi = np.stack([L - 0.5, np.ones_like(L), np.ones_like(L)], 1).astype(F)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def rows_of(over):
    """(offsets int64 [n + 1], ids int32 [total]) of a boolean query x triangle matrix: np.nonzero of every line"""
    over = np.asarray(over, bool)
    offsets = np.concatenate([[0], np.cumsum(over.sum(1))]).astype(np.int64)
    return offsets, np.nonzero(over)[1].astype(np.int32)

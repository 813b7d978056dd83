"""The all-hits lists of include/ezrt_multihit.h restated in numpy on the CPU oracle's intersectors (a helper of the tests, no test).

For one ray, V = the triangles the reference's hitBVH (P5/fsh:254-306) hands to hitTriangle, in the order it reaches them: near
child first, ties right-first, leaf ranges ascending, no pruning.  H = the members of V that hitTriangle accepts with
t < min(t_max, EZ_INF) (a NaN t_max: none), stably sorted by t.

Two tables decide everything: hitAABB over (ray, node) and hitTriangle's distance over (ray, triangle), both from the oracle's
ezrt_debug_math (ops 10 and 11) on the nine position floats of the encoded triangles and the boxes of the encoded nodes.  The
stack walk per ray is hit_bvh of oracle/ezrt_oracle.c:236-280 with the tables in place of the calls.  Nothing of the product is used.
"""
import numpy as np

EZ_INF = np.float32(114514.0)


def _tables(oracle_lib, tri, nodes, rays, chunk=128):
    """(A [n_rays, n_nodes], T [n_rays, n_tri]) float32: hitAABB of every node's box, hitTriangle's t (EZ_INF: no hit)"""
    P9 = np.ascontiguousarray(tri[:, :9], np.float32)
    B6 = np.ascontiguousarray(nodes[:, 6:12], np.float32)
    n, nn, nt = rays.shape[0], B6.shape[0], P9.shape[0]
    A = np.empty((n, nn), np.float32)
    T = np.empty((n, nt), np.float32)
    for r0 in range(0, n, chunk):
        r = rays[r0:r0 + chunk]
        k = r.shape[0]
        A[r0:r0 + k] = oracle_lib.debug_math(10, np.repeat(r, nn, axis=0), np.tile(B6, (k, 1)), n=k * nn).reshape(k, nn)
        T[r0:r0 + k] = oracle_lib.debug_math(11, np.repeat(r, nt, axis=0), np.tile(P9, (k, 1)), n=k * nt).reshape(k, nt)
    return A, T


def visit_lists(oracle_lib, tri, nodes, rays):
    """Per ray (ids int32, t float32): the triangles of V that hitTriangle accepts, in visit order, with their distances."""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 36)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 12)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    A, T = _tables(oracle_lib, tri, nodes, rays)
    left = nodes[:, 0].astype(np.int64).tolist()                   # (int) truncation, as get_node
    right = nodes[:, 1].astype(np.int64).tolist()
    cnt = nodes[:, 3].astype(np.int64).tolist()
    first = nodes[:, 4].astype(np.int64).tolist()
    inf = float(EZ_INF)
    out = []
    for i in range(rays.shape[0]):
        a = A[i].tolist()                                          # (float32 -> double is exact: the comparisons are the oracle's)
        order = []
        stack = [1]
        while stack:
            top = stack.pop()
            if cnt[top] > 0:
                order.extend(range(first[top], first[top] + cnt[top]))
                continue
            l, r = left[top], right[top]
            d1 = a[l] if l > 0 else inf
            d2 = a[r] if r > 0 else inf
            if d1 > 0.0 and d2 > 0.0:
                if d1 < d2:
                    stack.append(r)
                    stack.append(l)
                else:
                    stack.append(l)
                    stack.append(r)
            elif d1 > 0.0:
                stack.append(l)
            elif d2 > 0.0:
                stack.append(r)
        ids = np.asarray(order, np.int32)
        t = T[i, ids] if ids.size else np.zeros(0, np.float32)
        hit = t < EZ_INF                                           # op 11 answers EZ_INF for "not hit"; nothing at or beyond it counts
        out.append((ids[hit], t[hit]))
    return out


def expected_all_hits(oracle_lib, tri, nodes, rays, t_max, visits=None):
    """Per ray (ids int32, t float32): H sorted by t, equal t in visit order.  t_max: None or one float per ray.  `visits`: the
    result of visit_lists for the same scene and rays (it does not depend on t_max), to share it among calls."""
    if visits is None:
        visits = visit_lists(oracle_lib, tri, nodes, rays)
    out = []
    for i, (ids, t) in enumerate(visits):
        if t_max is not None:
            tm = np.float32(t_max[i])
            bound = np.float32(min(tm, EZ_INF))
            keep = np.zeros(t.shape, bool) if np.isnan(tm) else t < bound
            ids, t = ids[keep], t[keep]
        o = np.argsort(t, kind="stable")
        out.append((ids[o], t[o]))
    return out


def rows(lists, max_hits):
    """(tri int32 [n, max_hits], t float32 [n, max_hits], count int32 [n]): the outputs of ezrt_query_all_hits_device for the lists"""
    n = len(lists)
    tri = np.full((n, max_hits), -1, np.int32)
    t = np.full((n, max_hits), EZ_INF, np.float32)
    count = np.zeros(n, np.int32)
    for i, (ids, tt) in enumerate(lists):
        k = min(ids.size, max_hits)
        tri[i, :k] = ids[:k]
        t[i, :k] = tt[:k]
        count[i] = ids.size
    return tri, t, count

"""The mesh topology of include/ezrt_topology.h (rules M1 to M7) restated with Python dictionaries -- a helper, no test.  numpy only.

topology(tri) takes the scene's triangle rows ([n, 36] or [n, 9] or [n, 3, 3] float32) and returns every array of the device call;
at(tri, tri_a, edge_a, tri_b) is the rule for pairs.  Nothing here looks at a tree, and nothing is computed in floating point: a
vertex is the tuple of its three bit patterns with -0 replaced by +0, a half-edge is h = 3 t + e, an edge is a frozenset of two
vertices.  tests/test_topology_expected.py holds it to the properties the header states."""
import collections

import numpy as np

BOUNDARY, MANIFOLD, FLIPPED, NONMANIFOLD = 1, 2, 3, 4
Topology = collections.namedtuple("Topology", "twin edge_class mult root component comp_root comp_size comp_flags summary live")


def vertices(tri):
    """float32 [n, 3, 3]"""
    T = np.ascontiguousarray(tri, np.float32)
    if T.ndim == 2 and T.shape[1] == 36:
        T = T[:, :9]
    return np.ascontiguousarray(T.reshape(-1, 3, 3))


def keys(tri):
    """M1 and M2: (keys: a list of three tuples per triangle, live bool [n])"""
    V = vertices(tri)
    B = V.view(np.uint32).copy()
    B[B == 0x80000000] = 0
    fin = ((B & 0x7F800000) != 0x7F800000).all(axis=(1, 2))
    K = [[tuple(int(x) for x in B[t, v]) for v in range(3)] for t in range(V.shape[0])]
    live = np.array([bool(fin[t]) and len(set(K[t])) == 3 for t in range(V.shape[0])], bool)
    return K, live


def topology(tri, components=True):
    K, live = keys(tri)
    n = len(K)
    twin = np.full(3 * n, -1, np.int32)
    cls = np.zeros(3 * n, np.uint8)
    mult = np.zeros(3 * n, np.int32)
    edges = collections.OrderedDict()                                          # M3: edge -> [(h, start key)] in ascending h
    for t in range(n):
        if live[t]:
            for e in range(3):
                edges.setdefault(frozenset((K[t][e], K[t][(e + 1) % 3])), []).append((3 * t + e, K[t][e]))
    counts = [0, 0, 0, 0, 0]
    for members in edges.values():
        m = len(members)
        start0 = members[0][1]
        F = [h for h, s in members if s == start0]                             # M5: by direction, each ascending
        B = [h for h, s in members if s != start0]
        if m == 1:
            c = BOUNDARY
        elif m == 2:
            c = MANIFOLD if len(B) == 1 else FLIPPED
        else:
            c = NONMANIFOLD
        counts[c] += 1
        k = min(len(F), len(B))
        pairs = list(zip(F[:k], B[:k]))
        U = F[k:] + B[k:]                                                      # one of the two is empty
        pairs += [(U[i], U[i + 1]) for i in range(0, len(U) - 1, 2)]
        for a, b in pairs:
            twin[a], twin[b] = b, a
        for h, _ in members:
            cls[h], mult[h] = c, m
    root = np.full(n, -1, np.int32)
    component = np.full(n, -1, np.int32)
    comp_root, comp_size, comp_flags = [], [], []
    if components:                                                             # M6
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for members in edges.values():
            a = find(members[0][0] // 3)
            for h, _ in members[1:]:
                b = find(h // 3)
                a, b = min(a, b), max(a, b)
                parent[b] = a
        for t in range(n):
            if live[t]:
                root[t] = find(t)
        comp_root = sorted(set(int(r) for r in root if r >= 0))
        number = {r: c for c, r in enumerate(comp_root)}
        comp_size, comp_flags = [0] * len(comp_root), [0] * len(comp_root)
        for t in range(n):
            if live[t]:
                c = number[int(root[t])]
                component[t] = c
                comp_size[c] += 1
                for e in range(3):
                    comp_flags[c] |= {BOUNDARY: 1, MANIFOLD: 0, FLIPPED: 2, NONMANIFOLD: 4}[int(cls[3 * t + e])]
    summary = np.array([int(live.sum()), len(edges), counts[1], counts[2], counts[3], counts[4], len(comp_root),
                        int(mult.max()) if n else 0], np.int64)
    return Topology(twin, cls, mult, root, component, np.array(comp_root, np.int32), np.array(comp_size, np.int32),
                    np.array(comp_flags, np.uint8), summary, live)


def closed(topo):
    return bool(topo.summary[2] == 0 and topo.summary[5] == 0)


def oriented(topo):
    return bool(topo.summary[4] == 0 and topo.summary[5] == 0)


def at(tri, tri_a, edge_a, tri_b):
    """(shared int8 [k], opposite int8 [k])"""
    K, live = keys(tri)
    n = len(K)
    shared = np.full(len(tri_a), -1, np.int8)
    opposite = np.full(len(tri_a), -1, np.int8)
    for i, (a, ea, b) in enumerate(zip(tri_a, edge_a, tri_b)):
        a, ea, b = int(a), int(ea), int(b)
        if not (0 <= a < n and 0 <= b < n and 0 <= ea <= 2 and live[a] and live[b]):
            continue
        a0, a1 = K[a][ea], K[a][(ea + 1) % 3]
        for e in range(3):
            b0, b1 = K[b][e], K[b][(e + 1) % 3]
            if {a0, a1} == {b0, b1}:
                shared[i], opposite[i] = e, 1 if a0 == b1 else 0
    return shared, opposite


def edge_relation(tri, topo):
    """the edges without ids: the multiset of (edge as a frozenset of keys, class, m) over the half-edges of live triangles -- what a
    permutation of the ids must keep"""
    K, live = keys(tri)
    rel = collections.Counter()
    for t in range(len(K)):
        if live[t]:
            for e in range(3):
                rel[(frozenset((K[t][e], K[t][(e + 1) % 3])), int(topo.edge_class[3 * t + e]), int(topo.mult[3 * t + e]))] += 1
    return rel

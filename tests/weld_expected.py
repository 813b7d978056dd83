"""The vertex weld and the smooth normals of include/ezrt_vertices.h (rules W1 to W7, N1 to N4) restated with Python dictionaries and
float32 numpy -- a helper, no test.  numpy only.

weld(tri) takes the scene's triangle rows ([n, 36] or [n, 9] or [n, 3, 3] float32) and returns every array of the device call,
trimmed to V and L; at(tri, corner_a, corner_b) is the rule for pairs; edge_mult(tri, w) is W4's m(v, w) as a dictionary;
normals(tri, vertex, star_offsets, star) is N1 to N4: floats 9-17 of every row, one IEEE float32 operation per numpy operation, in the
order the header states.  W1 to W7 compute nothing in floating point: a vertex is the tuple of its three bit patterns with -0 replaced
by +0 (topology_expected.keys).  tests/test_weld_expected.py holds it to the properties the header states and pins the normals
against the host's readObj."""
import collections

import numpy as np

import topology_expected as TE

Weld = collections.namedtuple("Weld", "vertex vert_corner star_offsets star fans vert_flags summary live")
F = np.float32


def _others(c):
    t3 = c // 3 * 3
    k = c - t3
    return t3 + (k + 1) % 3, t3 + (k + 2) % 3


def weld(tri):
    K, live = TE.keys(tri)
    n = len(K)
    vertex = np.full(3 * n, -1, np.int32)
    number = {}                                                                # W2: key -> v, in order of the first (lowest) corner
    vert_corner = []
    stars = []
    for c in range(3 * n):
        if not live[c // 3]:
            continue
        key = K[c // 3][c % 3]
        if key not in number:
            number[key] = len(vert_corner)
            vert_corner.append(c)
            stars.append([])
        vertex[c] = number[key]
        stars[number[key]].append(c)                                           # W3: ascending, c is
    V = len(vert_corner)
    star_offsets = np.zeros(V + 1, np.int32)
    star_offsets[1:] = np.cumsum([len(s) for s in stars])
    star = np.array([c for s in stars for c in s], np.int32)
    fans = np.zeros(V, np.int32)
    flags = np.zeros(V, np.uint8)
    for v, s in enumerate(stars):
        m = collections.Counter()                                              # W4
        for c in s:
            for o in _others(c):
                m[int(vertex[o])] += 1
        parent = {c: c for c in s}                                             # W5

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        by_other = {}
        for c in s:
            for o in _others(c):
                w = int(vertex[o])
                if w in by_other:
                    parent[find(c)] = find(by_other[w])
                else:
                    by_other[w] = c
        fans[v] = len({find(c) for c in s})
        flags[v] = (1 if any(x == 1 for x in m.values()) else 0) | (2 if any(x >= 3 for x in m.values()) else 0) | (4 if fans[v] > 1 else 0)
    summary = np.array([len(star), V, max([len(s) for s in stars], default=0), int((flags & 1 != 0).sum()), int((flags & 2 != 0).sum()),
                        int((flags & 4 != 0).sum()), 0, 0], np.int64)
    return Weld(vertex, np.array(vert_corner, np.int32), star_offsets, star, fans, flags, summary, live)


def edge_mult(w):
    """W4: {(v, other vertex): m(v, other vertex)} from the stars alone"""
    m = collections.Counter()
    for v in range(len(w.vert_corner)):
        for c in w.star[w.star_offsets[v]:w.star_offsets[v + 1]]:
            for o in _others(int(c)):
                m[(v, int(w.vertex[o]))] += 1
    return m


def at(tri, corner_a, corner_b):
    """same int8 [k]"""
    K, live = TE.keys(tri)
    H = 3 * len(K)
    same = np.full(len(corner_a), -1, np.int8)
    for i, (a, b) in enumerate(zip(corner_a, corner_b)):
        a, b = int(a), int(b)
        if 0 <= a < H and 0 <= b < H and live[a // 3] and live[b // 3]:
            same[i] = 1 if K[a // 3][a % 3] == K[b // 3][b % 3] else 0
    return same


def _normalize(a):
    """a * (1.0f / sqrtf(dot(a, a))), dot = (x x + y y) + z z"""
    d = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    inv = F(1.0) / np.sqrt(d)
    return a * inv[:, None]


def face_normals(tri):
    """N1: float32 [n, 3]"""
    P = TE.vertices(tri)
    with np.errstate(all="ignore"):
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        assert c.dtype == np.float32
        return _normalize(c)


def _padded(x, size):
    x = np.asarray(x, np.int64).reshape(-1)
    out = np.zeros(size, np.int64)
    out[:min(size, x.size)] = x[:size]
    return out


def normals(tri, vertex, star_offsets, star):
    """N1 to N4: float32 [n, 9], the floats 9-17 of every row.  The weld arrays may be trimmed (they are padded with zeros to their
    full sizes, as the wrapper pads them) and may hold anything."""
    fn = face_normals(tri)
    n = fn.shape[0]
    H = 3 * n
    vertex, off, star = _padded(vertex, H), _padded(star_offsets, H + 1), _padded(star, H)
    usable = (vertex >= 0) & (vertex < H)                                      # N4, per corner
    vs = np.unique(vertex[usable])                                             # corners of one vertex share one sum
    lo, hi = off[vs], off[vs + 1]
    good = (lo >= 0) & (lo <= hi) & (hi <= H)
    S = np.zeros((vs.size, 3), F)                                              # N2: from +0
    with np.errstate(all="ignore"):
        for r in range(int((hi - lo)[good].max()) if good.any() else 0):
            act = np.nonzero(good & (hi - lo > r))[0]
            e = star[lo[act] + r]
            bad = (e < 0) | (e >= H)
            good[act[bad]] = False
            act, e = act[~bad], e[~bad]
            S[act] = S[act] + fn[e // 3]
        N = _normalize(S)
    out = np.repeat(fn, 3, axis=0)                                             # N1 wherever nothing better is known
    idx = np.minimum(np.searchsorted(vs, vertex), max(vs.size - 1, 0))
    ok = usable.copy()                                                         # (every usable vertex[c] is in vs)
    ok[ok] = good[idx[ok]]
    out[ok] = N[idx[ok]]
    return np.ascontiguousarray(out.reshape(n, 9))

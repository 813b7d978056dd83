"""The boundary loops and the cap of include/ezrt_boundary.h (rules B1 to B8 and C1 to C4) restated on the host -- a helper, no test.
numpy and Python integers only.

boundary(tri, twin, edge_class, area) takes the scene's triangle rows ([n, 36] or [n, 9] or [n, 3, 3] float32) and the two arrays of a
topology (or any garbage of that size: B2 reads nothing out of bounds) and returns every array of the device call; cap(rows, b) is
ezrt_cap_rows_device: the rows 0 .. B - 1 and cap_valid.  The successor is found by a sequential walk (B2), the paths from their
heads and the cycles by a sequential search in ascending order (B3), B7 with numpy float64 in exactly the written order and Python
integers for the sums.  tests/test_boundary_expected.py holds it to the properties the header states."""
import collections

import numpy as np

import weld_expected as WE

CLOSED = 1
Boundary = collections.namedtuple("Boundary", "next loop pos order loop_offsets lflags area2 summary takes scale steps")


def vertices(tri):
    """float32 [n, 3, 3]"""
    T = np.ascontiguousarray(tri, np.float32)
    if T.ndim == 2 and T.shape[1] == 36:
        T = T[:, :9]
    return np.ascontiguousarray(T.reshape(-1, 3, 3))


def successors(twin, edge_class):
    """B1 and B2: (takes bool [n], boundary bool [3 n], next int32 [3 n], the longest walk in steps)"""
    tw = [int(x) for x in np.asarray(twin).reshape(-1)]
    cl = [int(x) for x in np.asarray(edge_class).reshape(-1)]
    H = len(tw)
    n = H // 3
    takes = [all(1 <= cl[3 * t + e] <= 4 for e in range(3)) for t in range(n)]
    nxt = np.full(H, -1, np.int32)
    bnd = np.zeros(H, bool)
    longest = 0
    for h in range(H):
        t, e = divmod(h, 3)
        if not (takes[t] and cl[h] == 1):
            continue
        bnd[h] = True
        c = 3 * t + (e + 1) % 3
        for step in range(H):                                                  # bounded by 3 n_tri steps; never reached (B2)
            if cl[c] == 1:
                nxt[h] = c
                break
            if cl[c] != 2:
                break
            g = tw[c]
            if not (0 <= g < H and g // 3 != c // 3 and takes[g // 3] and cl[g] == 2 and tw[g] == c):
                break
            c = 3 * (g // 3) + (g % 3 + 1) % 3
        else:
            raise AssertionError("a walk of 3 n_tri steps: B2 says there is none")
        longest = max(longest, step)
    return np.array(takes, bool), bnd, nxt, longest


def scale(V, takes):
    """B6: S2 = 2 E - 30, E the frexp exponent of the largest finite |coordinate| of the triangles that take part"""
    B = V[takes].view(np.uint32) & np.uint32(0x7FFFFFFF)
    B = B[(B & 0x7F800000) != 0x7F800000]
    A = float(B.max().view(np.float32)) if B.size else 0.0
    E = int(np.frexp(np.float64(A))[1]) if A != 0.0 else 0
    return 2 * E - 30


def cross_r(a, b, S2):
    """B7: r of half-edges with starts a and ends b (float32 [m, 3]): m lists of three Python ints"""
    with np.errstate(all="ignore"):
        a, b = a.astype(np.float64), b.astype(np.float64)
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        r = np.rint(np.ldexp(c, -S2))                                          # round to nearest even
    return [[int(x) if np.isfinite(y) else 0 for x, y in zip(rr, cc)] for rr, cc in zip(r, c)]


def chains(bnd, nxt):
    """B3, B4: [(head, [members in order], closed)] in ascending order of the heads"""
    H = nxt.shape[0]
    pred = np.full(H, -1, np.int64)
    for h in np.nonzero(nxt >= 0)[0]:
        assert pred[nxt[h]] == -1 and bnd[nxt[h]], "two predecessors: B2 says there are none"
        pred[nxt[h]] = h
    seen = np.zeros(H, bool)
    out = []
    for h in np.nonzero(bnd)[0]:                                               # the paths, from their heads
        if pred[h] == -1:
            m = [int(h)]
            while nxt[m[-1]] >= 0:
                m.append(int(nxt[m[-1]]))
            seen[m] = True
            out.append((int(h), m, False))
    for h in np.nonzero(bnd)[0]:                                               # what is left are cycles; ascending: h is the lowest member
        if not seen[h]:
            m = [int(h)]
            while nxt[m[-1]] != h:
                m.append(int(nxt[m[-1]]))
                assert len(m) <= H
            seen[m] = True
            out.append((int(h), m, True))
    assert seen[bnd].all() and sum(len(m) for _, m, _ in out) == int(bnd.sum())
    return sorted(out)


def boundary(tri, twin, edge_class, area=True):
    V = vertices(tri)
    n = V.shape[0]
    takes, bnd, nxt, steps = successors(twin, edge_class)
    assert takes.shape[0] == n
    H = 3 * n
    ch = chains(bnd, nxt)
    loop = np.full(H, -1, np.int32)
    pos = np.full(H, -1, np.int32)
    order, offsets, lflags = [], [0], []
    for l, (_, m, closed) in enumerate(ch):
        loop[m] = l
        pos[m] = np.arange(len(m))
        order += m
        offsets.append(len(order))
        lflags.append(CLOSED if closed else 0)
    S2, area2 = 0, None
    if area:
        S2 = scale(V, takes)
        P = V.reshape(-1, 3)
        area2 = np.zeros((len(ch), 3), np.int64)
        for l, (_, m, _) in enumerate(ch):
            m = np.array(m)
            r = cross_r(P[m], P[3 * (m // 3) + (m % 3 + 1) % 3], S2)
            s = [sum(x[k] for x in r) for k in range(3)]
            assert all(-2 ** 63 <= x < 2 ** 63 for x in s)
            area2[l] = s
    summary = np.array([int(bnd.sum()), len(ch), sum(lflags), max([len(m) for _, m, _ in ch] + [0]), int((bnd & (nxt < 0)).sum()), S2, 0, 0],
                       np.int64)
    return Boundary(nxt, loop, pos, np.array(order, np.int32), np.array(offsets, np.int32), np.array(lflags, np.uint8), area2, summary, takes,
                    S2, steps)


def cap(rows, b):
    """C1 to C4 on truthful loops arrays: (cap float32 [B, 36], cap_valid uint8 [B])"""
    R = np.ascontiguousarray(rows, np.float32).reshape(-1, 36)
    B = int(b.summary[0])
    out = np.zeros((B, 36), np.float32)
    valid = np.zeros(B, np.uint8)
    P = R[:, :9].reshape(-1, 3)
    for j in range(B):
        h = int(b.order[j])
        l, p = int(b.loop[h]), int(b.pos[h])
        lo = int(b.loop_offsets[l])
        k = int(b.loop_offsets[l + 1]) - lo
        if not (b.lflags[l] & CLOSED and k >= 3 and 1 <= p <= k - 2 and lo + p == j):
            continue
        head = int(b.order[lo])
        out[j, 0:3], out[j, 3:6], out[j, 6:9] = P[head], P[3 * (h // 3) + (h % 3 + 1) % 3], P[h]   # C2: (H, end(h), start(h))
        out[j, 18:36] = R[h // 3, 18:36]
        valid[j] = 1
    m = valid != 0
    if m.any():
        out[m, 9:18] = np.tile(WE.face_normals(out[m]), 3)                     # C3: N1 of the new triangle, three times
    return out, valid


def capped(rows, b):
    """the caller's rows and the valid rows of the cap: the closed mesh"""
    c, v = cap(rows, b)
    return np.concatenate([np.ascontiguousarray(rows, np.float32).reshape(-1, 36), c[v != 0]])


def loop_area(b):
    """float64 [L, 3]: area2 * 2 ** S2 / 2"""
    return b.area2.astype(np.float64) * 2.0 ** (b.scale - 1)


def edge_cycles(tri, b):
    """the loops without ids: a sorted list of (closed, canonical sequence of directed edges as pairs of vertex keys) -- a cycle is
    rotated to start at its smallest edge; what a permutation of the triangle ids must keep"""
    V = vertices(tri).view(np.uint32).copy()
    V[V == 0x80000000] = 0
    K = [tuple(int(x) for x in v) for v in V.reshape(-1, 3)]
    out = []
    for l in range(len(b.lflags)):
        m = [int(h) for h in b.order[b.loop_offsets[l]:b.loop_offsets[l + 1]]]
        seq = [(K[h], K[3 * (h // 3) + (h % 3 + 1) % 3]) for h in m]
        if b.lflags[l] & CLOSED:
            i = seq.index(min(seq))
            seq = seq[i:] + seq[:i]
        out.append((bool(b.lflags[l] & CLOSED), tuple(seq)))
    return sorted(out)

"""The plane clipping of include/ezrt_clip.h (rules K1 to K8) restated in numpy on tests/plane_expected.py -- a helper, no test.

The sides are plane_expected.sides (P2), the new positions plane_expected.edge_point (P4); K5's interpolation is written out here,
one numpy operation per rounding (numpy never contracts).  clip(rows, plane) returns every array of the two device calls;
candidates(...) is K8, the fill over offsets that no count call left.  tests/test_clip_expected.py holds all of it to the properties
the header states."""
import collections

import numpy as np

import plane_expected as PE

F = np.float32
D = np.float64
Clip = collections.namedtuple("Clip", "offsets summary out src cut_edge count kind")
NONE, WHOLE, ONE_UP, ONE_DOWN = 0, 1, 2, 3


def rows36(rows):
    return np.ascontiguousarray(rows, F).reshape(-1, 36)


def new_vertex(X, nX, sx, Y, nY, sy):
    """K4, K5: (position float32 [r, 3], normal float32 [r, 3]) of the new vertex on the edges with the ends X and Y, their corner
    normals and their sides, one UP and one DOWN, whichever way round"""
    P = PE.edge_point(X, sx, Y, sy)
    sw = PE._less(Y, X)                                                        # A < B in P4's order of the values
    sa, sb = np.where(sw, sy, sx), np.where(sw, sx, sy)
    a, b = np.where(sw[:, None], nY, nX), np.where(sw[:, None], nX, nY)
    with np.errstate(all="ignore"):
        t = sa / (sa - sb)
        l = (a.astype(D) + t[:, None] * (b.astype(D) - a.astype(D))).astype(F)
    n = np.where((sa == 0.0)[:, None], a, np.where((sb == 0.0)[:, None], b, l))
    assert n.dtype == F
    return P, n


def pieces(rows, plane):
    """K2 .. K6 row by row: (count int64 [n], kind [n], finite bool [n], live bool, and per emitted piece in output order: out float32
    [T, 36], src int32 [T], cut_edge int8 [T])"""
    R = rows36(rows)
    n = R.shape[0]
    p = np.ascontiguousarray(plane, F).reshape(4)
    live = bool(PE.live(p[None])[0])
    V, N = R[:, :9].reshape(n, 3, 3), R[:, 9:18].reshape(n, 3, 3)
    s = PE.sides(p[None], V)[0]                                                # [n, 3]
    fin = np.isfinite(V).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        up = s >= 0.0
    nup = up.sum(1)
    ok = fin & live
    whole, one_up, one_dn = ok & (nup == 3), ok & (nup == 1), ok & (nup == 2)
    i = np.where(one_up, np.argmax(up, 1), np.argmax(~up, 1))                  # U, or D
    r = np.arange(n)
    i1, i2 = (i + 1) % 3, (i + 2) % 3
    s0, s1, s2 = s[r, i], s[r, i1], s[r, i2]
    up_piece = one_up & (s0 != 0.0)                                            # (U, q0, q1); with s(U) == 0 the row only touches
    first, second = one_dn & (s2 != 0.0), one_dn & (s1 != 0.0)                 # (a, b, Pb) when s(b) != 0; (a, Pb, Pa) when s(a) != 0
    count = whole.astype(np.int64) + up_piece + first + second
    kind = np.where(whole, WHOLE, np.where(up_piece, ONE_UP, np.where(first | second, ONE_DOWN, NONE)))
    cut = np.nonzero(up_piece | first | second)[0]
    # both kinds need the same two points once U or D is vertex 0: E01 of edge 0 -> 1 and E20 of edge 2 -> 0
    V0, V1, V2 = V[cut, i[cut]], V[cut, i1[cut]], V[cut, i2[cut]]
    N0, N1, N2 = N[cut, i[cut]], N[cut, i1[cut]], N[cut, i2[cut]]
    E01, M01 = new_vertex(V0, N0, s0[cut], V1, N1, s1[cut])
    E20, M20 = new_vertex(V2, N2, s2[cut], V0, N0, s0[cut])
    start = np.cumsum(count) - count                                           # K6: ascending source row, then the piece order of K3
    T = int(count.sum())
    out, src, edge = np.zeros((T, 36), F), np.full(T, -1, np.int32), np.full(T, -1, np.int8)

    def put(m, shift, a, na, b, nb, c, nc, e):
        """the piece (a, b, c) of the cut rows cut[m], `shift` output rows behind the row's first"""
        k = cut[m]
        to = start[k] + shift[m]
        out[to] = np.concatenate([a[m], b[m], c[m], na[m], nb[m], nc[m], R[k, 18:]], 1)
        src[to] = k
        edge[to] = e[m] if isinstance(e, np.ndarray) else e
    w = np.nonzero(whole)[0]
    out[start[w]], src[start[w]] = R[w], w
    zero = np.zeros(cut.size, np.int64)
    put(up_piece[cut], zero, V0, N0, E01, M01, E20, M20, 1)
    put(first[cut], zero, V1, N1, V2, N2, E20, M20, np.where(s1[cut] == 0.0, 2, -1).astype(np.int8))
    put(second[cut], first[cut].astype(np.int64), V1, N1, E20, M20, E01, M01, 1)
    assert (src >= 0).all()
    return count, kind, fin, live, out, src, edge


def clip(rows, plane):
    """the count call and the fill call with capacity = T"""
    count, kind, fin, live, out, src, edge = pieces(rows, plane)
    n = count.shape[0]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(count)
    whole, cutr = kind == WHOLE, (kind == ONE_UP) | (kind == ONE_DOWN)
    summary = np.array([offsets[n], whole.sum(), cutr.sum(), (fin & (count == 0)).sum(), (~fin).sum(), (edge >= 0).sum(), int(live), 0], np.int64)
    assert summary[1] + summary[2] + summary[3] + summary[4] == n and out.shape[0] == offsets[n]
    return Clip(offsets, summary, out, src, edge, count, kind)


def candidates(c, offsets, capacity):
    """K8 over any offsets: a list of (output row, piece) -- piece p of the truthful answer `c` (a Clip) must be written to the output
    row -- for every source row that passes the three tests; every other output row must stay untouched"""
    off = np.asarray(offsets, np.int64)
    out = []
    for k in np.nonzero(c.count)[0]:
        n = int(c.count[k])
        o, o1 = int(off[k]), int(off[k + 1])
        if o >= 0 and o + n <= capacity and o1 - o == n:
            out += [(o + j, int(c.offsets[k]) + j) for j in range(n)]
    return out


def cut_segments(c):
    """float32 [n_cut, 2, 3]: the cut edges start to end, in row order"""
    r = np.nonzero(c.cut_edge >= 0)[0]
    e = c.cut_edge[r].astype(np.int64)
    V = c.out[:, :9].reshape(-1, 3, 3)
    return np.stack([V[r, e], V[r, (e + 1) % 3]], 1).reshape(-1, 2, 3)


def canonical_cycles(points, loop_offsets):
    """the sorted list of cyclic point sequences (points float32 [B, 3], loop l at loop_offsets[l] .. loop_offsets[l + 1]), each rotated
    to start at its least point by the bytes of the bit patterns: what plane_loops_expected.canonical_cycles returns of a section"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    out = []
    for lo, hi in zip(loop_offsets[:-1], loop_offsets[1:]):
        keys = [p.tobytes() for p in P[int(lo):int(hi)]]
        k = keys.index(min(keys))
        out.append(tuple(keys[k:] + keys[:k]))
    return sorted(out)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN (K5: the sign and payload of a NaN normal are not part of the contract)"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()

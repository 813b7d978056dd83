"""The subdivision of include/ezrt_subdivide.h (rules S1 to S9) restated in float32 numpy -- a helper, no test.  numpy only.

subdivide(rows, mode, twin, edge_class, vertex, star_offsets, star, vert_flags) returns (out float32 [4 n, 36], summary int64 [8], rule
int8 [3 n], interior bool [3 n]).  One numpy operation per rounding, in the order the header writes them (numpy never contracts).  The
six arrays may be trimmed (they are padded with zeros to their full sizes, as the wrapper pads them) and may hold anything: S3, S4 and
S7 say what then happens.  A vertex's term is computed once and shared by its corners, as the header's T; the corner's own position
is multiplied in per corner.  tests/test_subdiv_expected.py holds all of it to the properties the header states."""
import numpy as np

import weld_expected as WE

F = np.float32
MIDPOINT, LOOP = 0, 1
KEEP, SMOOTH, BORDER = 7, 5, 6                                                 # the rule of a corner, by its number in the header
PIECES = ((0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5))                          # S1: 0-2 are P0 P1 P2, 3-5 are E0 E1 E2
NEXT = np.array([1, 2, 0])


def rows36(rows):
    return np.ascontiguousarray(rows, F).reshape(-1, 36)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()


def _keys(P):
    """M1: the bit patterns, -0 as +0"""
    B = bits(P).copy()
    B[B == 0x80000000] = 0
    return B


def _padded(x, size):
    x = np.asarray(x).astype(np.int64).reshape(-1)
    out = np.zeros(size, np.int64)
    out[:min(size, x.size)] = x[:size]
    return out


def _beta(k):
    return F(0.1875) if k == 3 else F(0.375) / F(k)


def _star_term(P, H, lo, hi, star, edge_class, flag):
    """S4 to S7 of one vertex with usable offsets: (rule, T float32 [3]); T is (beta * 0.5f) * S or 0.125f * B"""
    if flag > 1:
        return KEEP, None
    S = np.zeros(3, F)                                                         # from +0
    r = 0
    for j in range(lo, hi):
        o = int(star[j])
        if o < 0 or o >= H:
            return KEEP, None                                                  # S4: not usable
        t, k = divmod(o, 3)
        ka, kb = (k + 1) % 3, (k + 2) % 3
        pa, pb = P[t, ka], P[t, kb]
        if flag == 0:
            S = S + (pa + pb)                                                  # S5: the inner sum first
        else:
            if edge_class[o] == 1:                                             # the half-edge that leaves the corner
                S = S + pa
                r += 1
            if edge_class[3 * t + kb] == 1:                                    # the half-edge that enters it
                S = S + pb
                r += 1
    if flag == 0:
        return SMOOTH, (_beta(hi - lo) * F(0.5)) * S
    if r != 2:
        return KEEP, None
    return BORDER, F(0.125) * S


def subdivide(rows, mode=MIDPOINT, twin=None, edge_class=None, vertex=None, star_offsets=None, star=None, vert_flags=None):
    T = rows36(rows)
    n = T.shape[0]
    H = 3 * n
    P = np.ascontiguousarray(T[:, :9].reshape(n, 3, 3))
    N = np.ascontiguousarray(T[:, 9:18].reshape(n, 3, 3))
    rule = np.full(H, KEEP, np.int8)
    interior = np.zeros(H, bool)
    with np.errstate(all="ignore"):
        newP = P.copy()                                                        # S2, S7: on the bits
        ab = P + P[:, NEXT]
        E = ab * F(0.5)                                                        # S2
        if mode == LOOP and n:
            twin, edge_class, vertex = _padded(twin, H), _padded(edge_class, H), _padded(vertex, H)
            star_offsets, star, vert_flags = _padded(star_offsets, H + 1), _padded(star, H), _padded(vert_flags, H)
            # S3
            h = np.arange(H)
            t, e = h // 3, h % 3
            g = twin
            ok = ((edge_class == 2) | (edge_class == 3)) & (g >= 0) & (g < H)
            gs = np.where(ok, g, 0)
            tg, eg = gs // 3, gs % 3
            ok &= tg != t
            K = _keys(P)
            ka, kb, qa, qb = K[t, e], K[t, (e + 1) % 3], K[tg, eg], K[tg, (eg + 1) % 3]
            eq = lambda x, y: (x == y).all(axis=1)
            ok &= (eq(ka, qa) & eq(kb, qb)) | (eq(ka, qb) & eq(kb, qa))
            c, d = P[t, (e + 2) % 3], P[tg, (eg + 2) % 3]
            Ei = F(0.375) * ab.reshape(H, 3) + F(0.125) * (c + d)
            E = np.where(ok[:, None], Ei, E.reshape(H, 3)).reshape(n, 3, 3)
            interior = ok
            # S4 to S7
            usable = (vertex >= 0) & (vertex < H)
            p = P.reshape(H, 3)
            out_p = newP.reshape(H, 3)
            corners = np.nonzero(usable)[0]
            corners = corners[np.argsort(vertex[corners], kind="stable")]      # the corners of one vertex share one walk of its star
            vs, first = np.unique(vertex[corners], return_index=True)
            for v, i0, i1 in zip(vs.tolist(), first.tolist(), first.tolist()[1:] + [corners.size]):
                lo, hi = int(star_offsets[v]), int(star_offsets[v + 1])
                if not (0 <= lo < hi <= H):
                    continue
                r, term = _star_term(P, H, lo, hi, star, edge_class, int(vert_flags[v]))
                if r == KEEP:
                    continue
                idx = corners[i0:i1]
                if r == SMOOTH:
                    k = hi - lo
                    w = F(1.0) - F(k) * _beta(k)
                else:
                    w = F(0.75)
                out_p[idx] = w * p[idx] + term[None, :]
                rule[idx] = r
            newP = out_p.reshape(n, 3, 3)
        assert newP.dtype == F and E.dtype == F
        pts = np.concatenate([newP, E], axis=1)                                # [n, 6, 3]
        out = np.empty((n, 4, 36), F)
        for j, piece in enumerate(PIECES):
            out[:, j, 0:9] = pts[:, piece].reshape(n, 9)
            out[:, j, 18:] = T[:, 18:]                                         # S1: the source row's material
        if mode == LOOP:
            fn = WE.face_normals(out.reshape(4 * n, 36))                       # S8: N1 of the output row
            out[:, :, 9:18] = np.tile(fn, (1, 3)).reshape(n, 4, 9)
        else:
            nrm = np.concatenate([N, (N + N[:, NEXT]) * F(0.5)], axis=1)       # S2
            for j, piece in enumerate(PIECES):
                out[:, j, 9:18] = nrm[:, piece].reshape(n, 9)
    summary = np.array([4 * n, int((rule == SMOOTH).sum()), int((rule == BORDER).sum()), int((rule == KEEP).sum()), int(interior.sum()),
                        int((~interior).sum()), mode, 0], np.int64)
    return np.ascontiguousarray(out.reshape(4 * n, 36)), summary, rule, interior


def loop(rows, topo, weld):
    """LOOP mode with the arrays of topology_expected.topology and weld_expected.weld (or of the device calls)"""
    return subdivide(rows, LOOP, topo.twin, topo.edge_class, np.asarray(weld.vertex).reshape(-1), weld.star_offsets, weld.star, weld.vert_flags)

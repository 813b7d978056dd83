"""The smoothing of include/ezrt_smooth.h (rules U1 to U9) restated in float32 numpy -- a helper, no test.  numpy only.

smooth(rows, edge_class, vertex, star_offsets, star, vert_flags, steps, lam, mu, flags) returns (out float32 [n, 36], summary int64 [8],
rule int8 [3 n], X float32 [3 n, 3]): the rule every corner is under and the final state by slot.  One numpy operation per rounding,
in the order the header writes them (numpy never contracts).  The five arrays may be trimmed (they are padded with zeros to their full
sizes, as the wrapper pads them) and may hold anything: U2 and U4 say what then happens.  The state of a vertex lives in the SLOT of
its first corner f, the state of any other corner in its own; a step gathers through slots, so that what a corner of a kept or
unusable vertex holds is read as U3 says.  tests/test_smooth_expected.py holds all of it to the properties the header states."""
import numpy as np

import weld_expected as WE

F = np.float32
PIN_BORDER = 1
STEPS_MAX = 1024
KEPT, SMOOTH, BORDER = 0, 1, 2                                                # the rule of a vertex (U4); every corner that is not ACTIVE counts as KEPT
TAUBIN = (0.5, -0.53)


def rows36(rows):
    return np.ascontiguousarray(rows, F).reshape(-1, 36)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()


def _padded(x, size):
    x = np.asarray(x).astype(np.int64).reshape(-1)
    out = np.zeros(size, np.int64)
    out[:min(size, x.size)] = x[:size]
    return out


def plan(n, edge_class, vertex, star_offsets, star, vert_flags, flags=0):
    """U2, U4: (slot int64 [3 n], rule int8 [3 n] by corner, moving: [(f, rule, terms)] in ascending f, n_active).  terms of a SMOOTH
    vertex: int64 [k, 2], the corners pa(c') and pb(c') over its star; of a BORDER vertex: int64 [2], the two corners of U7 in the
    walk's order.  (Corners, not yet slots: the slot of a corner needs every vertex's verdict.)"""
    H = 3 * n
    edge_class, vertex = _padded(edge_class, H), _padded(vertex, H)
    star_offsets, star, vert_flags = _padded(star_offsets, H + 1), _padded(star, H), _padded(vert_flags, H)
    slot = np.arange(H, dtype=np.int64)
    rule = np.full(H, KEPT, np.int8)
    moving = []
    n_active = 0
    named = np.unique(vertex[(vertex >= 0) & (vertex < H)])                    # only stars of vertices that a corner names are walked
    for v in named.tolist():
        lo, hi = int(star_offsets[v]), int(star_offsets[v + 1])
        if not (0 <= lo < hi <= H):
            continue
        entries = star[lo:hi]
        if (entries < 0).any() or (entries >= H).any():
            continue                                                           # U2 (S4): not usable
        f = int(entries[0])
        if vertex[f] != v:
            continue                                                           # U2: not active
        n_active += 1
        mine = vertex == v
        slot[mine] = f
        t, k = entries // 3, entries % 3
        ca, cb = 3 * t + (k + 1) % 3, 3 * t + (k + 2) % 3
        flag = int(vert_flags[v])
        if flag == 0:
            rule[mine] = SMOOTH
            moving.append((f, SMOOTH, np.stack([ca, cb], 1)))
        elif flag == 1 and not (flags & PIN_BORDER):
            terms = []
            for i in range(entries.size):
                if edge_class[entries[i]] == 1:                                # the half-edge that leaves the corner
                    terms.append(int(ca[i]))
                if edge_class[cb[i]] == 1:                                     # the half-edge that enters it: 3 t + kb
                    terms.append(int(cb[i]))
            if len(terms) == 2:
                rule[mine] = BORDER
                moving.append((f, BORDER, np.asarray(terms, np.int64)))
    moving.sort(key=lambda m: m[0])
    return slot, rule, moving, n_active


def smooth(rows, edge_class, vertex, star_offsets, star, vert_flags, steps=1, lam=0.5, mu=None, flags=0):
    T = rows36(rows)
    n = T.shape[0]
    H = 3 * n
    lam = F(lam)
    mu = lam if mu is None else F(mu)
    assert 1 <= steps <= STEPS_MAX and np.isfinite(lam) and np.isfinite(mu) and not (flags & ~PIN_BORDER)
    slot, rule, moving, n_active = plan(n, edge_class, vertex, star_offsets, star, vert_flags, flags)
    X = np.ascontiguousarray(T[:, :9].reshape(H, 3)).copy()                    # U3: x_0 by slot, a corner's own position in its own slot
    sm = [m for m in moving if m[1] == SMOOTH]
    bd = [m for m in moving if m[1] == BORDER]
    fs = np.asarray([m[0] for m in sm], np.int64)
    fb = np.asarray([m[0] for m in bd], np.int64)
    ks = np.asarray([m[2].shape[0] for m in sm], np.int64)
    kmax = int(ks.max()) if ks.size else 0
    A = np.zeros((fs.size, kmax), np.int64)
    B = np.zeros((fs.size, kmax), np.int64)
    for i, m in enumerate(sm):
        A[i, :ks[i]], B[i, :ks[i]] = slot[m[2][:, 0]], slot[m[2][:, 1]]
    TB = slot[np.asarray([m[2] for m in bd], np.int64).reshape(-1, 2)]
    den = (2 * ks).astype(F)[:, None]                                          # (float)(2 * k)
    with np.errstate(all="ignore"):
        for j in range(steps):
            w = mu if j & 1 else lam                                           # U5
            new = X.copy()
            if fs.size:                                                        # U6
                S = np.zeros((fs.size, 3), F)
                for i in range(kmax):
                    at = ks > i
                    S[at] = S[at] + (X[A[at, i]] + X[B[at, i]])
                m = S / den
                x = X[fs]
                new[fs] = x + w * (m - x)
            if fb.size:                                                        # U7
                Bs = (np.zeros((fb.size, 3), F) + X[TB[:, 0]]) + X[TB[:, 1]]
                m = Bs * F(0.5)
                x = X[fb]
                new[fb] = x + w * (m - x)
            assert new.dtype == F
            X = new
        out = T.copy()
        moved = rule != KEPT
        P = out[:, :9].reshape(H, 3).copy()
        P[moved] = X[slot[moved]]                                              # U8: every other corner keeps its own bits
        out[:, :9] = P.reshape(n, 9)
        out[:, 9:18] = np.tile(WE.face_normals(out), (1, 3))                   # U1: N1 of the output row
    summary = np.array([n, int((rule == SMOOTH).sum()), int((rule == BORDER).sum()), int((rule == KEPT).sum()), n_active, steps, flags, 0], np.int64)
    return out, summary, rule, X


def smooth_of(rows, topo, weld, **kw):
    """with the arrays of topology_expected.topology and weld_expected.weld (or of the device calls)"""
    return smooth(rows, topo.edge_class, np.asarray(weld.vertex).reshape(-1), weld.star_offsets, weld.star, weld.vert_flags, **kw)


def work_bytes(n):
    """the header's formula"""
    if n <= 0:
        return 8
    H = 3 * n
    blocks = (H + 255) // 256
    return (H * 45 + 8 * (blocks + 1) + 8 * ((blocks + 2047) // 2048 + 1) + 7) // 8 * 8


def shortest_edge(rows):
    V = rows36(rows)[:, :9].reshape(-1, 3, 3).astype(np.float64)
    return float(np.sqrt(((V - V[:, [1, 2, 0]]) ** 2).sum(-1)).min())


def distinct_vertices(rows):
    V = rows36(rows)[:, :9].reshape(-1, 3) + F(0.0)
    return len({p.tobytes() for p in V})

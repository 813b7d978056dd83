"""The decimation of include/ezrt_decimate.h (rules D1 to D10) restated in numpy -- a helper, no test.  numpy only.

decimate(rows, grid4, flags) returns a Dec: cell int32 [3 n] (D3), cell_corner int32 [n_cells], cell_point float32 [n_cells, 3] (D4,
D5), offsets int64 [n + 1] and summary int64 [8] (D9), out float32 [T, 36] and src int32 [T] (D8), kind int8 [n] (0 kept, 1 collapsed,
2 duplicate, 3 takes no part) and kept bool [n_cells, 3] (the components that D5 kept).  One numpy operation per rounding, in the order
the header writes them, in float64 where the header says double (numpy never contracts); the sums are int64; the cells, their lowest
corners and the duplicates come from np.unique over sorted integer rows.  There is no tolerance anywhere.

row_of(rows, cell, cell_point) is D8 for EVERY source row from arrays that need not be a count's, and candidates(n, cell, offsets,
capacity) the (output row, source row) pairs that D10 lets through: together they say what a fill writes whatever it is handed.
tests/test_decimate_expected.py holds all of it to the properties the header states."""
import collections

import numpy as np

import weld_expected as WE

F = np.float32
D = np.float64
DEDUP = 1
KEPT, COLLAPSED, DUPLICATE, NO_PART = 0, 1, 2, 3

Dec = collections.namedtuple("Dec", "cell cell_corner cell_point offsets summary out src kind kept")


def rows36(rows):
    return np.ascontiguousarray(rows, F).reshape(-1, 36)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()


def keys(P):
    """M1: the bit patterns, -0 as +0"""
    B = bits(P).copy()
    B[B == 0x80000000] = 0
    return B


def live(grid4):
    """D1"""
    g = np.asarray(grid4, F).reshape(4)
    return bool(np.isfinite(g).all() and g[3] > 0)


def fixed(P, grid4):
    """D2: (part bool [n], U int64 [n, 3, 3]) of positions float32 [n, 3, 3]; U is 0 where the row takes no part"""
    g = np.asarray(grid4, F).reshape(4)
    n = P.shape[0]
    if not live(g):
        return np.zeros(n, bool), np.zeros((n, 3, 3), np.int64)
    with np.errstate(all="ignore"):
        u = (P.astype(D) - g[:3].astype(D)[None, None, :]) / D(g[3])
        w = u * D(16777216.0)
        ok = (w >= D(-2.0 ** 44)) & (w < D(2.0 ** 44))                         # a NaN is in no range
        part = np.isfinite(P).reshape(n, 9).all(1) & ok.reshape(n, 9).all(1)
        U = np.where(part[:, None, None], np.floor(np.where(ok, w, 0.0)), 0.0).astype(np.int64)
    return part, U


def row_of(rows, cell, cell_point):
    """D8 of every source row whose three cells are in range of cell_point (other rows: zeros): float32 [n, 36]"""
    T = rows36(rows)
    n = T.shape[0]
    c = np.asarray(cell, np.int64).reshape(n, 3)
    pts = np.ascontiguousarray(cell_point, F).reshape(-1, 3)
    ok = ((c >= 0) & (c < pts.shape[0])).all(1)
    out = np.zeros((n, 36), F)
    out[ok, 0:9] = pts[c[ok]].reshape(-1, 9)
    out[ok, 9:18] = np.tile(WE.face_normals(out[ok]), (1, 3))                  # N1 of the OUTPUT positions, for all three corners
    out[ok, 18:] = T[ok, 18:]
    return out


def candidates(n, cell, offsets, capacity):
    """D10: the (output row, source row) pairs a fill writes, from arrays that need not be a count's"""
    c = np.asarray(cell, np.int64).reshape(n, 3)
    o = [int(x) for x in np.asarray(offsets).reshape(-1)[:n + 1]]
    H = 3 * n
    out = []
    for t in range(n):
        x, y, z = (int(v) for v in c[t])
        if min(x, y, z) < 0 or max(x, y, z) >= H or x == y or y == z or x == z:
            continue
        if o[t] >= 0 and o[t] + 1 <= capacity and o[t + 1] - o[t] == 1:
            out.append((o[t], t))
    return out


def decimate(rows, grid4, flags=DEDUP):
    assert flags in (0, DEDUP)
    T = rows36(rows)
    n = T.shape[0]
    H = 3 * n
    g = np.asarray(grid4, F).reshape(4)
    P = np.ascontiguousarray(T[:, :9].reshape(n, 3, 3))
    part, U = fixed(P, g)
    cell = np.full(H, -1, np.int32)
    corners = np.nonzero(np.repeat(part, 3))[0]                                # ascending
    Uc = U.reshape(H, 3)[corners]
    ic, qc = Uc >> 24, Uc & 0xFFFFFF                                           # D2: arithmetic shift
    n_cells = 0
    cell_corner = np.zeros(0, np.int32)
    cell_point = np.zeros((0, 3), F)
    kept = np.zeros((0, 3), bool)
    if corners.size:
        assert ic.min() >= -2 ** 20 and ic.max() < 2 ** 20
        _, first, inv = np.unique(ic, axis=0, return_index=True, return_inverse=True)   # first: the lowest corner, the input ascends
        inv = inv.reshape(-1)
        order = np.argsort(first, kind="stable")                               # D3: numbered by ascending lowest corner
        number = np.empty(order.size, np.int64)
        number[order] = np.arange(order.size)
        j = number[inv]
        n_cells = order.size
        cell[corners] = j
        cell_corner = corners[first[order]].astype(np.int32)
        i_cell = ic[first[order]]
        N = np.bincount(j, minlength=n_cells).astype(np.int64)
        S = np.zeros((n_cells, 3), np.int64)
        np.add.at(S, j, qc)                                                    # D4: exact
        K = keys(P).reshape(H, 3)[corners]
        lo = np.full((n_cells, 3), 0xFFFFFFFF, np.uint32)
        hi = np.zeros((n_cells, 3), np.uint32)
        np.minimum.at(lo, j, K)
        np.maximum.at(hi, j, K)
        with np.errstate(all="ignore"):
            m = S.astype(D) / N.astype(D)[:, None]
            f = m * D(2.0 ** -24)
            s = i_cell.astype(D) + f
            p = s * D(g[3])
            x = (g[:3].astype(D)[None, :] + p).astype(F)
        kept = lo == hi                                                        # D5
        cell_point = np.where(kept, lo.view(F), x).astype(F)
    c3 = cell.reshape(n, 3).astype(np.int64)
    survive = part & (c3[:, 0] != c3[:, 1]) & (c3[:, 1] != c3[:, 2]) & (c3[:, 0] != c3[:, 2])
    kind = np.where(part, np.where(survive, KEPT, COLLAPSED), NO_PART).astype(np.int8)
    if flags & DEDUP:
        rows_s = np.nonzero(survive)[0]
        if rows_s.size:
            _, first = np.unique(np.sort(c3[rows_s], axis=1), axis=0, return_index=True)   # the lowest row of every unordered triple
            dup = np.ones(rows_s.size, bool)
            dup[first] = False
            kind[rows_s[dup]] = DUPLICATE
    keep = kind == KEPT
    offsets = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    src = np.nonzero(keep)[0].astype(np.int32)
    with np.errstate(all="ignore"):
        out = row_of(T, cell, np.concatenate([cell_point, np.zeros((H - n_cells, 3), F)]))[src]
    summary = np.array([int(keep.sum()), int((kind == COLLAPSED).sum()), int((kind == DUPLICATE).sum()), int((kind == NO_PART).sum()), n_cells,
                        int(kept.all(1).sum()), flags, int(live(g))], np.int64)
    return Dec(cell, cell_corner, np.ascontiguousarray(cell_point, F), offsets, summary, np.ascontiguousarray(out, F), src, kind, kept)


def grid_of(rows, div, margin=0.013):
    """the grid of the header's table: the origin at the mesh minimum minus `margin`, h the largest extent / div (float32 [4])"""
    V = rows36(rows)[:, :9].reshape(-1, 3)
    V = V[np.isfinite(V).all(1)].astype(D)
    lo, hi = V.min(0), V.max(0)
    return np.append(lo - margin, (hi - lo).max() / div).astype(F)


def closed(out):
    """every undirected edge (by M1 key) of the rows is in exactly two of them"""
    K = keys(rows36(out)[:, :9].reshape(-1, 3, 3)).astype(np.int64)
    count = collections.Counter()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        for x, y in zip(map(tuple, K[:, a].tolist()), map(tuple, K[:, b].tolist())):
            count[(x, y) if x < y else (y, x)] += 1
    return bool(count) and all(v == 2 for v in count.values())

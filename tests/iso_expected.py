"""The isosurface extraction of include/ezrt_isosurface.h (rules G1 to G9) restated in numpy -- a helper, no test.  numpy only.

iso(values, grid8, material18) returns an Iso: offsets int64 [n_blocks + 1] and summary int64 [8] (G8), out float32 [T, 36] and cell
int32 [T] (G7), counts int64 [n_cells] (G5), and tet int8 [T], piece int8 [T], edges int64 [T, 3, 2] -- the tet, the piece and, per
vertex of the row, the two grid vertex indices (G1) of the edge its point lies on -- for the tests of the properties.  One numpy
operation per rounding, in the order the header writes them, in float64 where the header says double (numpy never contracts).  The
cells of one (tet, mask, piece) case are handled together, so a 65^3 grid takes seconds.  There is no tolerance anywhere.

derive_exchange() re-derives the winding table of G5 from midpoints; block_rows(I, b) and candidates(I, offsets, capacity) say what
a fill writes whatever offsets it is handed (G9).  tests/test_iso_expected.py holds all of it to the properties the header states."""
import collections
import itertools

import numpy as np

import weld_expected as WE

F = np.float32
D = np.float64
BLOCK = 256

Iso = collections.namedtuple("Iso", "offsets summary out cell counts tet piece edges")

AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
PERMS = tuple(itertools.permutations(range(3)))                                # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
EVEN = (True, False, False, True, True, False)                                 # the parity of PERMS


def _tets():
    out = []
    for p in PERMS:
        v = [np.zeros(3, np.int64)]
        for a in p:
            v.append(v[-1] + np.array(AXES[a]))
        out.append(np.array(v))
    return np.array(out)                                                       # [6, 4, 3]: (dx, dy, dz) of T0 .. T3


TETS = _tets()
TET_COUNT = (0, 1, 2, 1, 0)                                                    # by the number of INSIDE vertices
EXCHANGED_EVEN = (2, 5, 8, 10, 11, 14)                                         # G5, as the header lists them


def pieces_of(mask):
    """G5 as written, before any exchange: a list of pieces, each three edges (a, b), a < b, of local vertices"""
    ins = [v for v in range(4) if mask >> v & 1]
    outs = [v for v in range(4) if not mask >> v & 1]
    e = lambda x, y: (min(x, y), max(x, y))
    if len(ins) == 1:
        return [[e(ins[0], j) for j in outs]]
    if len(ins) == 3:
        return [[e(outs[0], j) for j in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        return [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    return []


def exchanged(t, mask):
    """G5's table: is the piece of tet t and this mask emitted with its second and third vertex exchanged?"""
    return (mask in EXCHANGED_EVEN) == EVEN[t]


def derive_exchange():
    """bool [6, 16]: the table from geometry -- every point at its edge's midpoint, the piece exchanged when its normal as written
    faces away from the OUTSIDE vertices.  Asserts that every piece of every case has a side (no normal is perpendicular)."""
    table = np.zeros((6, 16), bool)
    for t in range(6):
        V = TETS[t].astype(D)
        for mask in range(1, 15):
            outs = [v for v in range(4) if not mask >> v & 1]
            away = []
            for piece in pieces_of(mask):
                q = np.array([(V[a] + V[b]) * 0.5 for a, b in piece])
                n = np.cross(q[1] - q[0], q[2] - q[0])
                d = np.array([np.dot(n, V[o] - q[0]) for o in outs])
                assert (d > 0).all() or (d < 0).all(), (t, mask)
                away.append(bool((d < 0).all()))
            assert len(set(away)) == 1, (t, mask)                              # both pieces of a quadrilateral agree
            table[t, mask] = away[0]
    return table


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_rows(got, want):
    """equal on the bits; a NaN is a NaN"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    return got.shape == want.shape and not ((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any()


def live(grid8):
    """G1"""
    g = np.asarray(grid8, F).reshape(8)
    return bool(np.isfinite(g[:7]).all() and (g[3:6] > 0).all())


def grid8(origin=(0, 0, 0), spacing=1.0, iso=0.0):
    h = (spacing,) * 3 if np.ndim(spacing) == 0 else tuple(spacing)
    return np.array(list(origin) + list(h) + [iso, 0.0], D).astype(F)


def positions(shape, grid):
    """G2: float32 [nz ny nx, 3]"""
    nz, ny, nx = shape
    g = np.asarray(grid, F).reshape(8).astype(D)
    with np.errstate(all="ignore"):
        x = (g[0] + np.arange(nx, dtype=D) * g[3]).astype(F)
        y = (g[1] + np.arange(ny, dtype=D) * g[4]).astype(F)
        z = (g[2] + np.arange(nz, dtype=D) * g[5]).astype(F)
    P = np.empty((nz, ny, nx, 3), F)
    P[..., 0], P[..., 1], P[..., 2] = x[None, None, :], y[None, :, None], z[:, None, None]
    return P.reshape(-1, 3)


def n_blocks_of(shape):
    nz, ny, nx = shape
    return ((nx - 1) * (ny - 1) * (nz - 1) + BLOCK - 1) // BLOCK


def classify(values, grid):
    """G3, G5: (finite bool [n_cells], byte uint8 [n_cells] -- bit dx + 2 dy + 4 dz set where that corner is INSIDE --, counts int64
    [n_cells])"""
    V = np.ascontiguousarray(values, F)
    nz, ny, nx = V.shape
    g = np.asarray(grid, F).reshape(8)
    n_cells = (nx - 1) * (ny - 1) * (nz - 1)
    fin = np.ones(n_cells, bool)
    byte = np.zeros(n_cells, np.uint8)
    with np.errstate(invalid="ignore"):
        for c in range(8):
            dx, dy, dz = c & 1, c >> 1 & 1, c >> 2
            v = V[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].reshape(-1)
            fin &= np.isfinite(v)
            byte |= (v < g[6]).astype(np.uint8) << np.uint8(c)
    counts = np.zeros(n_cells, np.int64)
    if live(g):
        for t in range(6):
            counts += np.array(TET_COUNT)[popcount4(tet_masks(byte, t))]
        counts[~fin] = 0
    return fin, byte, counts


def corner_bit(d):
    return int(d[0] + 2 * d[1] + 4 * d[2])


def tet_masks(byte, t):
    m = np.zeros(byte.shape, np.uint8)
    for v in range(4):
        m |= (byte >> np.uint8(corner_bit(TETS[t][v])) & np.uint8(1)) << np.uint8(v)
    return m


def popcount4(m):
    return (m & 1) + (m >> 1 & 1) + (m >> 2 & 1) + (m >> 3 & 1)


def iso(values, grid, material18=None):
    V = np.ascontiguousarray(values, F)
    assert V.ndim == 3
    nz, ny, nx = V.shape
    g = np.asarray(grid, F).reshape(8)
    mat = np.zeros(18, F) if material18 is None else np.ascontiguousarray(material18, F).reshape(18)
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    n_cells = max(cx, 0) * max(cy, 0) * max(cz, 0)
    nb = (n_cells + BLOCK - 1) // BLOCK
    if n_cells == 0:
        return Iso(np.zeros(1, np.int64), np.array([0, 0, 0, 0, 0, 0, int(live(g)), 0], np.int64), np.zeros((0, 36), F), np.zeros(0, np.int32),
                   np.zeros(0, np.int64), np.zeros(0, np.int8), np.zeros(0, np.int8), np.zeros((0, 3, 2), np.int64))
    fin, byte, counts = classify(V, g)
    per_block = np.zeros(nb * BLOCK, np.int64)
    per_block[:n_cells] = counts
    per_block = per_block.reshape(nb, BLOCK).sum(1)
    offsets = np.concatenate([[0], np.cumsum(per_block)]).astype(np.int64)
    T = int(offsets[-1])
    summary = np.array([T, int((counts > 0).sum()), int((fin & (counts == 0)).sum()), int((~fin).sum()), int((per_block > 0).sum()), n_cells,
                        int(live(g)), 0], np.int64)
    cells_l, tets_l, piece_l, pts_l, edge_l = [], [], [], [], []
    gd = g.astype(D)
    flat = V.reshape(-1)
    emit = fin & (counts > 0)
    for t in range(6):
        masks = tet_masks(byte, t)
        for mask in range(1, 15):
            sel = np.nonzero(emit & (masks == mask))[0]
            if sel.size == 0:
                continue
            i, r = sel % cx, sel // cx
            j, k = r % cy, r // cy
            ijk = np.stack([i, j, k], 1)                                        # [m, 3]
            for p, piece in enumerate(pieces_of(mask)):
                if exchanged(t, mask):
                    piece = [piece[0], piece[2], piece[1]]
                P = np.empty((sel.size, 3, 3), F)
                E = np.empty((sel.size, 3, 2), np.int64)
                for q, (a, b) in enumerate(piece):
                    A, B = ijk + TETS[t][a][None], ijk + TETS[t][b][None]
                    ia, ib = (A[:, 2] * ny + A[:, 1]) * nx + A[:, 0], (B[:, 2] * ny + B[:, 1]) * nx + B[:, 0]
                    assert (ia < ib).all()                                     # G4: the local order is the order of the indices
                    fA, fB = flat[ia].astype(D), flat[ib].astype(D)
                    with np.errstate(all="ignore"):
                        tt = (gd[6] - fA) / (fB - fA)                           # G6
                        for c in range(3):
                            pA = gd[c] + A[:, c].astype(D) * gd[3 + c]
                            pB = gd[c] + B[:, c].astype(D) * gd[3 + c]
                            d = pB - pA
                            P[:, q, c] = (pA + tt * d).astype(F)
                    E[:, q, 0], E[:, q, 1] = ia, ib
                cells_l.append(sel), tets_l.append(np.full(sel.size, t, np.int8)), piece_l.append(np.full(sel.size, p, np.int8))
                pts_l.append(P), edge_l.append(E)
    if T == 0:
        return Iso(offsets, summary, np.zeros((0, 36), F), np.zeros(0, np.int32), counts, np.zeros(0, np.int8), np.zeros(0, np.int8),
                   np.zeros((0, 3, 2), np.int64))
    cell = np.concatenate(cells_l)
    tet, piece, P, E = np.concatenate(tets_l), np.concatenate(piece_l), np.concatenate(pts_l), np.concatenate(edge_l)
    order = np.argsort((cell * 6 + tet) * 2 + piece, kind="stable")            # G8: cell, tet, piece
    assert order.size == T                                                     # G5: the count is the number of rows
    cell, tet, piece, P, E = cell[order], tet[order], piece[order], P[order], E[order]
    out = np.empty((T, 36), F)
    out[:, :9] = P.reshape(T, 9)
    with np.errstate(all="ignore"):
        out[:, 9:18] = np.tile(WE.face_normals(out), (1, 3))                   # G7: N1 of the OUTPUT positions, for all three corners
    out[:, 18:] = mat[None]
    return Iso(offsets, summary, out, cell.astype(np.int32), counts, tet, piece, E)


def block_rows(I, b):
    """(first, count): the rows of block b in I.out"""
    return int(I.offsets[b]), int(I.offsets[b + 1] - I.offsets[b])


def candidates(I, offsets, capacity):
    """G9: the (output row, row of I.out) pairs a fill writes, from offsets that need not be a count's"""
    o = [int(x) for x in np.asarray(offsets).reshape(-1)]
    out = []
    for b in range(I.offsets.size - 1):
        first, c = block_rows(I, b)
        if c > 0 and o[b] >= 0 and o[b] + c <= capacity and o[b + 1] - o[b] == c:
            out.extend((o[b] + r, first + r) for r in range(c))
    return out


# ---- the properties

def keys(P):
    """the bit patterns, -0 as +0 (M1 of ezrt_topology.h)"""
    B = bits(P).copy()
    B[B == 0x80000000] = 0
    return B


def topology(out):
    """of the rows with three different vertices by value: (rows, V, E, F, once_each_way) -- once_each_way: every directed edge once
    and its opposite once"""
    K = keys(np.ascontiguousarray(out, F)[:, :9].reshape(-1, 3, 3))
    _, inv = np.unique(K.reshape(-1, 3), axis=0, return_inverse=True)
    idx = inv.reshape(-1, 3).astype(np.int64)
    good = (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2])
    idx = idx[good]
    nv = np.unique(idx).size
    a = np.concatenate([idx[:, 0], idx[:, 1], idx[:, 2]])
    b = np.concatenate([idx[:, 1], idx[:, 2], idx[:, 0]])
    M = int(inv.max()) + 1 if inv.size else 1
    fwd = a * M + b
    und, cnt = np.unique(np.minimum(a, b) * M + np.maximum(a, b), return_counts=True)
    ok = bool(np.unique(fwd).size == fwd.size and np.isin(b * M + a, fwd).all() and (cnt == 2).all())
    return int(good.sum()), nv, und.size, int(good.sum()), ok


def volume(out):
    """the signed volume of the rows, in double"""
    P = np.ascontiguousarray(out, F)[:, :9].reshape(-1, 3, 3).astype(D)
    return float(np.einsum("ij,ij->i", P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0)

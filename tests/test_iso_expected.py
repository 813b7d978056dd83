"""tests/iso_expected.py, the numpy restatement of include/ezrt_isosurface.h (G1 to G9), held to the properties the header states.  Needs
no GPU and no library: what the GPU tests compare against is checked here on its own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_expected as IE  # noqa: E402
import iso_scenes as IS  # noqa: E402

F = np.float32

_cache = {}


def _iso(name, V, g):
    if name not in _cache:
        _cache[name] = IE.iso(V, g, IS.MATERIAL)
    return _cache[name]


def test_the_winding_table_from_midpoints():
    table = IE.derive_exchange()                                               # asserts that every piece of every case has a side
    assert IE.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    for t in range(6):
        sign = np.linalg.det(np.array([IE.AXES[a] for a in IE.PERMS[t]], float))
        assert (sign > 0) == IE.EVEN[t]
        for mask in range(1, 15):
            assert bool(table[t, mask]) == IE.exchanged(t, mask), (t, mask)
    even, odd = table[0, 1:15], table[1, 1:15]
    assert [m for m in range(1, 15) if table[0, m]] == [2, 5, 8, 10, 11, 14]
    assert (even != odd).all()                                                 # odd permutations: the complement
    for t in range(6):
        assert (table[t, 1:15] == (even if IE.EVEN[t] else odd)).all()
    # the restatement's rows face the OUTSIDE vertices with the points wherever they are on their edges, not only at midpoints
    V, g = IS.patterns()
    I = _iso("patterns", V, g)
    P = IE.positions(V.shape, g).astype(np.float64)
    T = I.out[:, :9].reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    flat = V.reshape(-1)
    checked = 0
    for q in range(3):
        for end in range(2):
            v = I.edges[:, q, end]
            outside = flat[v] >= g[6]
            d = np.einsum("ij,ij->i", n, P[v] - T[:, 0])
            assert (d[outside] > 0).all() and (d[~outside] < 0).all()
            checked += v.size
    assert checked == 6 * I.out.shape[0] > 0


def test_the_tets_are_the_kuhn_split():
    assert IE.TETS.shape == (6, 4, 3)
    vol = 0.0
    for t in range(6):
        T = IE.TETS[t]
        assert (T[0] == 0).all() and (T[3] == 1).all() and ((T[1:] - T[:-1]).sum(1) == 1).all()
        vol += abs(np.linalg.det((T[1:] - T[0]).astype(float))) / 6
        assert [IE.corner_bit(v) for v in T] == sorted(IE.corner_bit(v) for v in T)   # G4: the local order is the order of the indices
    assert vol == pytest.approx(1.0)
    assert [[IE.corner_bit(v) for v in T] for T in IE.TETS] == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]


def test_all_256_cell_cases_occur():
    V, g = IS.patterns()
    fin, byte, counts = IE.classify(V, g)
    assert fin.all() and np.unique(byte).size == 256
    I = _iso("patterns", V, g)
    assert int(counts.sum()) == I.out.shape[0] == int(I.summary[0]) and counts.max() <= 12
    for p in (0, 255):
        assert (counts[byte == p] == 0).all()
    assert (counts[(byte != 0) & (byte != 255)] >= 2).all()                   # a mixed cell cuts at least two of its tets


@pytest.mark.parametrize("name,euler,rows", (("sphere", 2, 3164), ("torus", 0, 3584)))
def test_closed_surfaces(name, euler, rows):
    V, g = getattr(IS, name)()
    I = _iso(name, V, g)
    n, nv, ne, nf, ok = IE.topology(I.out)
    assert n == I.out.shape[0] == rows                                         # the header's number; no row with two equal vertices
    assert ok and nv - ne + nf == euler                                        # every edge in exactly two rows, once each way
    assert IE.volume(I.out) > 0
    assert not np.isnan(I.out).any()
    assert IE.bits(I.out[:, 18:]).tolist() == [IE.bits(IS.MATERIAL).tolist()] * n
    assert np.array_equal(IE.bits(I.out[:, 9:12]), IE.bits(I.out[:, 12:15])) and np.array_equal(IE.bits(I.out[:, 9:12]), IE.bits(I.out[:, 15:18]))


def test_the_sphere_is_a_sphere():
    V, g = IS.sphere()
    I = _iso("sphere", V, g)
    r = 0.33 * 2.0
    assert IE.volume(I.out) == pytest.approx(4.0 / 3.0 * np.pi * r ** 3, rel=0.03)
    T = I.out[:, :9].reshape(-1, 3, 3).astype(np.float64)
    c = np.array([0.13, -0.09, 0.27]) * 0.125
    assert (np.einsum("ij,ij->i", I.out[:, 9:12].astype(np.float64), T.mean(1) - c) > 0).all()   # the normals face outwards


def test_padded_noise_is_closed():
    V, g = IS.noise()
    I = _iso("noise", V, g)
    n, nv, ne, nf, ok = IE.topology(I.out)
    assert ok and n == I.out.shape[0] == 27636 and nv - ne + nf == -654        # the header's numbers
    V2, g2 = IS.noise(padded=False)
    assert not IE.topology(IE.iso(V2, g2).out)[4]                              # open where it meets the border of the grid


def test_values_at_the_level_keep_the_rest_closed():
    V, g = IS.at_level()
    I = _iso("at_level", V, g)
    n, nv, ne, nf, ok = IE.topology(I.out)
    assert (n, I.out.shape[0], int((V == g[6]).sum())) == (1536, 3384, 258)   # the header's numbers: degenerate rows are emitted
    assert ok and nv - ne + nf == 2
    assert np.isnan(I.out[:, 9:18]).any()                                      # G7: a degenerate row gets NaN


def test_a_shared_edge_gives_the_same_bits():
    for name in ("sphere", "noise", "patterns"):
        V, g = getattr(IS, name)()
        I = _iso(name, V, g)
        nv = V.size
        key = (I.edges[:, :, 0] * nv + I.edges[:, :, 1]).reshape(-1)
        P = IE.bits(I.out[:, :9].reshape(-1, 3))
        order = np.argsort(key, kind="stable")
        key, P = key[order], P[order]
        same = key[1:] == key[:-1]
        assert same.sum() > key.size // 2 and (P[1:][same] == P[:-1][same]).all()


def test_every_position_lies_in_the_box_of_its_cell():
    for name in ("sphere", "torus", "noise", "at_level", "patterns"):
        V, g = getattr(IS, name)()
        I = _iso(name, V, g)
        nz, ny, nx = V.shape
        P = IE.positions(V.shape, g).reshape(nz, ny, nx, 3)
        c = I.cell.astype(np.int64)
        i, r = c % (nx - 1), c // (nx - 1)
        j, k = r % (ny - 1), r // (ny - 1)
        lo, hi = P[k, j, i], P[k + 1, j + 1, i + 1]
        T = I.out[:, :9].reshape(-1, 3, 3)
        assert (T >= lo[:, None]).all() and (T <= hi[:, None]).all(), name
        assert (np.diff(c) >= 0).all()                                         # G8: ascending cell
        same = np.diff(c) == 0
        tp = I.tet.astype(int) * 2 + I.piece
        assert (np.diff(tp)[same] > 0).all()                                   # then tet, then piece


def test_count_offsets_and_summary():
    for name in ("sphere", "noise", "patterns", "special"):
        V, g = getattr(IS, name)()
        I = _iso(name, V, g)
        nb = IE.n_blocks_of(V.shape)
        n_cells = I.counts.size
        assert I.offsets.size == nb + 1 and I.offsets[0] == 0 and I.offsets[-1] == I.out.shape[0] == I.counts.sum() == I.summary[0]
        assert np.array_equal(np.bincount(I.cell, minlength=n_cells), I.counts)
        assert I.summary[1] + I.summary[2] + I.summary[3] == n_cells == I.summary[5] and I.summary[6] == 1 and I.summary[7] == 0
        assert I.summary[4] == (np.diff(I.offsets) > 0).sum()
        for b in range(nb):
            assert I.offsets[b + 1] - I.offsets[b] == I.counts[256 * b:256 * b + 256].sum()
        assert len(IE.candidates(I, I.offsets, I.out.shape[0])) == I.out.shape[0]
        last = int(np.nonzero(np.diff(I.offsets) > 0)[0][-1])
        assert len(IE.candidates(I, I.offsets, I.out.shape[0] - 1)) == I.offsets[last]   # the last block that emits does not fit: whole or not at all


def test_non_finite_values_and_grids_that_are_not_live():
    V, g = IS.special()
    I = _iso("special", V, g)
    fin, byte, counts = IE.classify(V, g)
    assert I.summary[3] == (~fin).sum() == 8 * 3 + 1                           # three vertices inside the grid, eight cells each, and one in a corner
    assert (counts[~fin] == 0).all() and not np.isin(np.nonzero(~fin)[0], I.cell).any()
    assert np.isfinite(I.out[:, :9]).all()
    # -0 against a level of +0, and a value at the level, are outside
    flat = V.reshape(-1)
    assert (np.signbit(flat) & (flat == 0)).sum() > 10
    for q in range(3):
        a, b = flat[I.edges[:, q, 0]], flat[I.edges[:, q, 1]]
        assert ((a < 0) != (b < 0)).all()
    for name, dead in IS.not_live():
        J = IE.iso(V, dead)
        assert J.out.shape[0] == 0 and J.summary.tolist() == [0, 0, int(fin.sum()), int((~fin).sum()), 0, fin.size, 0, 0], name
        assert not J.offsets.any()
    for nx, ny, nz in IS.NO_CELLS:
        J = IE.iso(np.zeros((nz, ny, nx), F), IE.grid8())
        assert J.summary.tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and J.offsets.tolist() == [0]


def test_adding_a_constant_changes_nothing():
    V, g = IS.at_level()                                                       # integers: the sums are exact
    I = _iso("at_level", V, g)
    g2 = g.copy()
    g2[6] += 3.0
    J = IE.iso(V + F(3.0), g2, IS.MATERIAL)
    assert IE.same_rows(I.out, J.out) and np.array_equal(I.offsets, J.offsets)


def test_positions_are_g2():
    g = IE.grid8((0.1, -0.3, 2.7), (0.37, 0.11, 1.3), 0.0)
    P = IE.positions((3, 4, 5), g).reshape(3, 4, 5, 3)
    gd = g.astype(np.float64)
    for k, j, i in ((0, 0, 0), (2, 3, 4), (1, 2, 3)):
        assert P[k, j, i].tolist() == [F(gd[0] + i * gd[3]), F(gd[1] + j * gd[4]), F(gd[2] + k * gd[5])]


def test_a_65_cubed_grid_is_within_reach():
    """the restatement handles the cells of one (tet, mask, piece) case together -- at most 6 * 14 * 2 passes whatever the grid -- so the
    65^3 field of the GPU chain takes about a second; no clock is read here, since a loaded machine says nothing about the code"""
    V, g = IS.sphere(65)
    I = _iso("sphere65", V, g)
    assert I.counts.size == 64 ** 3 and I.out.shape[0] > 50000
    n, nv, ne, nf, ok = IE.topology(I.out)
    assert ok and n == I.out.shape[0] and nv - ne + nf == 2

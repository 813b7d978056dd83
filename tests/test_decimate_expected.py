"""tests/decimate_expected.py, the numpy restatement of include/ezrt_decimate.h (rules D1 to D10), held to the properties the header
states and to the integers of its table.  Needs no GPU and no library: numpy and the shipped meshes.

* the table: rows out, cells, collapsed rows and duplicates of the sphere and the bunny under six grids; the decimated sphere is closed
  at div 4 and 8; div 16 and 4096 are the identity;
* the summary identities, the numbering of D3 and the order of D9 on every size and grid the device test uses;
* a permutation of the rows leaves the set of points, the set of emitted triples and (without DEDUP) the multiset of output triangles;
* rotating rows rotates their output, reversing them reverses it;
* identity where no two vertex values share a cell, -0 becoming +0; idempotence on every shipped mesh;
* the edge cases of tests/decimate_scenes.py, each held to what the rules say of it;
* D10: what the restatement's fill writes from a count's arrays is the count's output, and capacity cuts it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_scenes as CS  # noqa: E402
import decimate_expected as DE  # noqa: E402
import decimate_scenes as DS  # noqa: E402
import subdiv_scenes as SS  # noqa: E402

F = np.float32
_cache = {}


def _dec(key, R, g, flags=DE.DEDUP):
    k = (key, flags)
    if k not in _cache:
        _cache[k] = DE.decimate(R, g, flags)
    return _cache[k]


def _positions(out):
    return DE.keys(DE.rows36(out)[:, :9])


def _triangles(out):
    """the output triangles as a sorted list of sorted vertex triples (unordered, by key)"""
    K = _positions(out).reshape(-1, 3, 3)
    return sorted(tuple(sorted(map(tuple, t.tolist()))) for t in K)


def _check(R, g, d, flags):
    """what holds of every result"""
    n = R.shape[0]
    s = d.summary.tolist()
    assert s[0] + s[1] + s[2] + s[3] == n and s[0] == d.out.shape[0] == d.src.size == int(d.offsets[n]) <= n
    assert s[6] == flags and s[7] == int(DE.live(g)) and (flags or s[2] == 0)
    assert d.offsets[0] == 0 and set(np.diff(d.offsets).tolist()) <= {0, 1} and np.array_equal(np.nonzero(np.diff(d.offsets))[0], d.src)
    assert s[4] == d.cell_corner.size == d.cell_point.shape[0] and s[5] == int(d.kept.all(1).sum())
    part = d.kind != DE.NO_PART
    assert ((d.cell.reshape(n, 3) >= 0).all(1) == part).all() and ((d.cell.reshape(n, 3) == -1).all(1) == ~part).all()
    if s[4]:
        assert (np.diff(d.cell_corner) > 0).all() and np.array_equal(d.cell[d.cell_corner], np.arange(s[4]))   # D3: by ascending lowest corner
        first = np.full(s[4], 3 * n, np.int64)
        np.minimum.at(first, d.cell[d.cell >= 0], np.nonzero(d.cell >= 0)[0])
        assert np.array_equal(first, d.cell_corner)
    V = DE.keys(R[part][:, :9]).reshape(-1, 3)
    assert s[4] <= np.unique(V, axis=0).shape[0] if V.size else s[4] == 0
    assert DE.same_rows(d.out[:, 18:], R[d.src][:, 18:])
    assert DE.same_rows(d.out[:, :9], d.cell_point[d.cell.reshape(n, 3)[d.src]].reshape(-1, 9))


@pytest.mark.parametrize("name,div,rows_out,cells,collapsed,duplicates", DS.TABLE)
def test_the_table(name, div, rows_out, cells, collapsed, duplicates):
    R = DS.shipped(name)
    g = DS.grid(R, div)
    d = _dec((name, div), R, g)
    assert d.summary.tolist()[:5] == [rows_out, collapsed, duplicates, 0, cells]
    _check(R, g, d, DE.DEDUP)
    if name == "sphere" and div in (4, 8):
        assert DE.closed(d.out) and DE.closed(R)
    if name == "bunny" and div in (8, 16):
        assert not DE.closed(d.out)
    if collapsed == 0:                                                         # the identity: one vertex value per cell
        assert d.kept.all() and np.array_equal(_positions(d.out), _positions(R)) and np.array_equal(d.src, np.arange(R.shape[0]))


@pytest.mark.parametrize("flags", (0, DE.DEDUP))
@pytest.mark.parametrize("n", DS.SIZES)
def test_summary_numbering_and_order(n, flags):
    R = DS.sized(n)
    for div in DS.GRIDS:
        g = DS.grid(R, div)
        _check(R, g, _dec(("sized", n, div), R, g, flags), flags)


@pytest.mark.parametrize("case", (("bunny", 8), ("bunny", 16), ("sphere", 4), (2049, 17), (257, 3)))
def test_a_permutation_of_the_rows(case):
    R = DS.shipped(case[0]) if isinstance(case[0], str) else DS.sized(case[0])
    g = DS.grid(R, case[1])
    perm = np.random.default_rng(DS.SEED + 1).permutation(R.shape[0])
    for flags in (0, DE.DEDUP):
        a, b = DE.decimate(R, g, flags), DE.decimate(R[perm], g, flags)
        pts = lambda d: sorted(map(tuple, DE.keys(d.cell_point).tolist()))
        assert pts(a) == pts(b) and a.summary.tolist() == b.summary.tolist()
        assert set(_triangles(a.out)) == set(_triangles(b.out))
        if not flags:
            assert _triangles(a.out) == _triangles(b.out)
            assert sorted(map(bytes, a.out[:, :9])) == sorted(map(bytes, b.out[:, :9]))   # stored order and winding included


@pytest.mark.parametrize("case", (("bunny", 8), ("sphere", 8), (2049, 17), (255, 3)))
def test_rotation_and_reversal(case):
    R = DS.shipped(case[0]) if isinstance(case[0], str) else DS.sized(case[0])
    g = DS.grid(R, case[1])
    a = DE.decimate(R, g)
    k = np.random.default_rng(DS.SEED + 2).integers(0, 3, R.shape[0])
    b = DE.decimate(CS.rotate_rows(R, k), g)
    assert np.array_equal(a.src, b.src) and a.summary.tolist() == b.summary.tolist()
    assert DE.same_rows(CS.rotate_rows(a.out, k[a.src])[:, :9], b.out[:, :9]) and DE.same_rows(a.out[:, 18:], b.out[:, 18:])
    c = DE.decimate(SS.reverse_rows(R), g)
    assert np.array_equal(a.src, c.src) and a.summary.tolist() == c.summary.tolist()
    assert DE.same_rows(SS.reverse_rows(a.out)[:, :9], c.out[:, :9]) and DE.same_rows(a.out[:, 18:], c.out[:, 18:])


def test_identity_where_no_two_values_share_a_cell():
    odd = CS.decorate(F([[(1, 2, 3), (1, 2, 3), (0, 1, 0)], [(np.nan, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 0, 0), (0, np.inf, 0), (0, 0, 1)],
                         [(0.5, 0.25, -0.0), (0.5, 0.25, 0.0), (1, 1, 1)]]), DS.SEED + 3)   # a repeated vertex (once by -0 == +0), NaN, infinity
    R = np.concatenate([SS.rows(name) for name in ("tetra", "octa", "cube_pow2", "signed_zero", "grid_pow2", "moebius")] + [odd])
    g = DS.grid(R, 8192)
    for flags in (0, DE.DEDUP):
        d = DE.decimate(R, g, flags)
        assert d.kept.all()                                                    # the premise: every cell holds one vertex value
        K = DE.keys(R[:, :9]).reshape(-1, 3, 3)
        eq = lambda i, j: (K[:, i] == K[:, j]).all(1)
        gone = ~np.isfinite(R[:, :9]).all(1) | eq(0, 1) | eq(1, 2) | eq(0, 2)
        assert d.summary[3] == int((~np.isfinite(R[:, :9]).all(1)).sum()) and d.summary[1] == int(gone.sum()) - d.summary[3]
        assert d.summary[0] == R.shape[0] - int(gone.sum()) - d.summary[2] and (flags or d.summary[2] == 0)
        assert np.array_equal(_positions(d.out), DE.keys(R[d.src][:, :9]))     # on the bits, -0 as +0
        assert not (DE.bits(d.out[:, :9]) == 0x80000000).any() and (DE.bits(R[d.src][:, :9]) == 0x80000000).any()


@pytest.mark.parametrize("name", ("sphere", "bunny", "sphere2"))
def test_idempotence(name):
    R = DS.shipped(name)
    for div in (4, 8, 16):
        g = DS.grid(R, div)
        a = DE.decimate(R, g)
        b = DE.decimate(a.out, g)
        assert DE.same_rows(b.out, a.out) and b.summary.tolist()[:4] == [a.out.shape[0], 0, 0, 0] and b.kept.all()
        pts = lambda P: sorted(map(tuple, DE.keys(P).tolist()))
        assert pts(b.cell_point) == pts(a.cell_point[np.unique(a.cell.reshape(-1, 3)[a.src])])   # the points in use, not one moved


def _edge(name, flags=DE.DEDUP):
    R, g = DS.edge(name)
    d = DE.decimate(R, g, flags)
    _check(R, g, d, flags)
    return R, g, d


def test_a_corner_on_a_face_belongs_to_the_upper_cell():
    R, g, d = _edge("on a face")
    part, U = DE.fixed(R[:, :9].reshape(-1, 3, 3), g)
    assert part.all() and (U[0, 0, 0] >> 24, U[0, 1, 0] >> 24) == (5, 4) and U[0, 0, 0] & 0xFFFFFF == 0 and U[0, 1, 0] & 0xFFFFFF == 0xFFFFFF
    assert d.cell[0] != d.cell[1] and d.cell[0] == d.cell[3] and d.summary[0] == 2


def test_negative_coordinates():
    R, g, d = _edge("negative")
    part, U = DE.fixed(R[:, :9].reshape(-1, 3, 3), g)
    assert (U[0] >> 24).tolist() == [[-1, -1, -1], [-1, -2, -1], [-2, -1, -3]] and (U[1] >> 24).tolist() == [[-4, -1, -1], [-1, -2, -1], [-1, -3, -4]]
    assert (U[0, 1] & 0xFFFFFF).tolist() == [0, 0x800000, 0xC00000] and d.cell[1] == d.cell[4] and d.summary.tolist()[:5] == [2, 0, 0, 0, 5]
    assert d.kept.all() and np.array_equal(_positions(d.out), _positions(R))   # alone in their cells: not moved


def test_minus_zero_is_plus_zero():
    R, g, d = _edge("minus zero")
    assert d.cell[0] == d.cell[3] and d.summary.tolist()[:5] == [2, 0, 0, 0, 5] and d.kept.all()
    assert (DE.bits(R[:, :9]) == 0x80000000).sum() == 8 and not (DE.bits(d.cell_point) == 0x80000000).any()
    assert np.array_equal(DE.bits(d.out[:, :9]), _positions(R))


def test_the_index_limits():
    R, g, d = _edge("index limits")
    assert d.kind.tolist() == [DE.KEPT, DE.NO_PART, DE.KEPT, DE.NO_PART, DE.NO_PART]
    part, U = DE.fixed(R[:, :9].reshape(-1, 3, 3), g)
    assert (U[0, 0, 0] >> 24, U[2, 0, 0] >> 24) == (2 ** 20 - 1, -2 ** 20) and U[0, 0, 0] == 2 ** 44 - 2 ** 23 and U[2, 0, 0] == -2 ** 44
    assert np.array_equal(_positions(d.out), _positions(R[[0, 2]]))


def test_overflow_and_a_denormal_h():
    R, g, d = _edge("u overflows")
    assert d.kind.tolist() == [DE.NO_PART, DE.KEPT] and d.summary[7] == 1
    R, g, d = _edge("h denormal")
    assert g[3] > 0 and g[3] < np.finfo(F).tiny and d.summary[7] == 1
    assert d.kind.tolist() == [DE.COLLAPSED, DE.NO_PART, DE.COLLAPSED] and d.cell.tolist() == [0, 0, 0, -1, -1, -1, 0, 1, 0]


@pytest.mark.parametrize("name", ("h zero", "h minus zero", "h negative", "h NaN", "h infinite", "origin NaN", "origin infinite"))
def test_a_grid_that_is_not_live(name):
    for flags in (0, DE.DEDUP):
        R, g, d = _edge(name, flags)
        assert d.summary.tolist() == [0, 0, 0, R.shape[0], 0, 0, flags, 0] and (d.cell == -1).all() and not d.offsets.any()


def test_rows_that_are_not_finite():
    R, g, d = _edge("NaN and Inf rows")
    bad = ~np.isfinite(R[:, :9]).all(1)
    assert bad.sum() >= 3 and ((d.kind == DE.NO_PART) == bad).all() and (d.cell.reshape(-1, 3)[bad] == -1).all()
    assert d.summary[0] > 0 and np.isfinite(d.cell_point).all()


def test_all_corners_in_one_cell():
    R, g, d = _edge("one cell")
    assert d.summary.tolist() == [0, 320, 0, 0, 1, 0, 1, 1] and not d.cell.any() and d.cell_corner.tolist() == [0]
    part, U = DE.fixed(R[:, :9].reshape(-1, 3, 3), g)
    q = (U & 0xFFFFFF).reshape(-1, 3)
    m = q.sum(0).astype(np.float64) / np.float64(960)                          # D4 once more, by hand
    want = (g[:3].astype(np.float64) + (np.float64(0) + m * 2.0 ** -24) * np.float64(g[3])).astype(F)
    assert np.array_equal(DE.bits(d.cell_point[0]), DE.bits(want))
    R2, g2 = DS.one_cell()
    d2 = DE.decimate(R2, g2)
    assert d2.summary.tolist() == [0, 20480, 0, 0, 1, 0, 1, 1]


def test_the_two_faces_of_a_thin_plate():
    R, g, d = _edge("thin plate")
    assert d.summary.tolist()[:5] == [8, 0, 8, 0, 9] and d.src.tolist() == list(range(8)) and (d.kind[8:] == DE.DUPLICATE).all()
    R, g, d0 = _edge("thin plate", 0)
    assert d0.summary.tolist()[:5] == [16, 0, 0, 0, 9] and set(_triangles(d0.out)) == set(_triangles(d.out))
    assert np.array_equal(d0.cell, d.cell) and np.array_equal(DE.bits(d0.cell_point), DE.bits(d.cell_point))
    # lower rows win: with the bottom sheet first, the bottom's windings are kept
    e = DE.decimate(R[::-1], g)
    assert e.src.tolist() == list(range(8)) and DE.same_rows(e.out, d0.out[::-1][:8])


def test_an_axis_aligned_face_stays_flat():
    R, g, d = _edge("flat face")
    assert d.summary[0] == 12 and d.summary[4] == 12 and d.summary[5] == 0
    assert d.kept[:, 2].all() and not d.kept[:, 0].all() and (DE.bits(d.cell_point[:, 2]) == DE.bits(F(0.3))).all()
    assert (DE.bits(d.out[:, [2, 5, 8]]) == DE.bits(F(0.3))).all()
    nrm = d.out[:, 9:18].reshape(-1, 3)                                        # N1 of a flat face: along z exactly, up or down with the winding
    assert not nrm[:, :2].any() and (np.abs(np.abs(nrm[:, 2]) - 1) <= 2.0 ** -23).all()


def test_the_fill_of_the_restatement():
    R = DS.sized(257)
    g = DS.grid(R, 17)
    d = DE.decimate(R, g)
    n, T = R.shape[0], int(d.summary[0])
    assert 0 < T < n
    pts = np.concatenate([d.cell_point, np.zeros((3 * n - d.cell_point.shape[0], 3), F)])
    rows = DE.row_of(R, d.cell, pts)
    assert DE.candidates(n, d.cell, d.offsets, T) == [(r, int(t)) for r, t in enumerate(d.src)] and DE.same_rows(rows[d.src], d.out)
    assert DE.candidates(n, d.cell, d.offsets, T // 2) == [(r, int(d.src[r])) for r in range(T // 2)]
    assert DE.candidates(n, d.cell, d.offsets, 0) == [] and DE.candidates(n, d.cell, d.offsets[::-1], T) == []
    bad = d.cell.copy()
    t = int(d.src[3])
    bad[3 * t] = bad[3 * t + 1]                                                # equal entries: the row is not written
    assert (3, t) not in DE.candidates(n, bad, d.offsets, T) and len(DE.candidates(n, bad, d.offsets, T)) == T - 1
    bad[3 * t] = 3 * n                                                         # out of range
    assert len(DE.candidates(n, bad, d.offsets, T)) == T - 1

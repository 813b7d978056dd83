"""Decimation on device tensors (include/ezrt_decimate.h, ezrt_amd/query.py: decimate_rows).

Every output of both calls -- cell, cell_corner, cell_point, offsets, summary; out, src -- is compared EXACTLY with
tests/decimate_expected.py, the header's rules restated in numpy and held to their properties by tests/test_decimate_expected.py.
There is no tolerance anywhere (a NaN normal is a NaN).

* row counts that straddle wave, workgroup, fill tile and scan tile, each under three grids and both flag values, over poisoned
  buffers with room behind them;
* the shipped meshes under the header's table, near one corner per cell (the fullest table) and with all 61440 corners of sphere2 in
  ONE cell (the most contended slot: the sums must come out exact);
* the edge cases of tests/decimate_scenes.py;
* `work` pre-filled with zeros, with 0xFF and with noise; two calls on two streams;
* the staged and the per-lane route of the fill (tri36 and out offset by one row, and by 4 bytes) give the same bits; capacity below
  T, offsets and cells that no count call left: rows are whole or absent, nothing outside [0, capacity) is touched;
* a chain: decimate the sphere, a scene of the rows, mesh_topology says closed; subdivide once, decimate on a fine grid: the
  subdivided positions come back on the bits;
* the wrapper, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402
import decimate_expected as DE  # noqa: E402
import decimate_scenes as DS  # noqa: E402
import orient_scenes as OS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
P = C.c_void_p
F = np.float32
POISON = -7
POISON_F = 12345.0
ROOM = 8
FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sg(hip):
    """a scene for the device and the error slot: the calls read none of its triangles"""
    return hip.scene_create(*OS.scene("cube_pow2", None))


_cache = {}


def _want(key, R, g, flags):
    """the restatement's Dec, computed once and shared"""
    k = (key, flags)
    if k not in _cache:
        _cache[k] = DE.decimate(R, g, flags)
    return _cache[k]


def _g(x, dev, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev)                        # (a copy: the scenes are handed out read-only)


def _count(lib, sg, R, grid, flags, dev, work_fill=FILL, stream=None, sync=True, work_off=0):
    """ezrt_decimate_count_device over poisoned buffers with ROOM entries behind their stated size; `work` begins work_off int64 into a
    512-byte aligned allocation"""
    n = R.shape[0]
    H = 3 * n
    d_rows = _g(np.concatenate([R, np.full((1, 36), 2.0, F)]), dev, F)          # a guard row behind the rows
    d_grid = _g(grid, dev, F)
    cell = torch.full((H + ROOM,), POISON, dtype=torch.int32, device=dev)
    corner = torch.full((H + ROOM,), POISON, dtype=torch.int32, device=dev)
    point = torch.full((H + ROOM, 3), POISON_F, dtype=torch.float32, device=dev)
    offsets = torch.full((n + 1 + ROOM,), POISON, dtype=torch.int64, device=dev)
    summary = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_decimate_work_bytes(n)
    assert wb % 8 == 0
    if isinstance(work_fill, int):
        whole = torch.full((work_off + wb // 8 + ROOM,), work_fill, dtype=torch.int64, device=dev)
    else:
        whole = torch.from_numpy(work_fill.integers(-2 ** 63, 2 ** 63 - 1, work_off + wb // 8 + ROOM, dtype=np.int64)).to(dev)
    assert whole.data_ptr() % 512 == 0
    work, head = whole[work_off:], whole[:work_off].clone()
    tail = work[wb // 8:].clone()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_decimate_count_device(sg._h, P(d_rows.data_ptr()), n, P(d_grid.data_ptr()), flags, P(cell.data_ptr()), P(corner.data_ptr()),
                                         P(point.data_ptr()), P(offsets.data_ptr()), P(summary.data_ptr()), P(work.data_ptr()), wb,
                                         P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((work[wb // 8:] == tail).all()) and bool((whole[:work_off] == head).all())   # nothing outside the stated bytes of work
        assert np.array_equal(DE.bits(d_rows[:n].cpu().numpy()), DE.bits(R))
        return cell.cpu().numpy(), corner.cpu().numpy(), point.cpu().numpy(), offsets.cpu().numpy(), summary.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_count(got, d, n, what=""):
    cell, corner, point, offsets, summary = got
    H, nc = 3 * n, int(d.summary[4])
    assert np.array_equal(summary[:8], d.summary) and (summary[8:] == POISON).all(), "%s: summary %s, not %s" % (what, summary[:8].tolist(), d.summary.tolist())
    assert np.array_equal(cell[:H], d.cell), "%s: cell differs first at %d" % (what, int(np.argmax(cell[:H] != d.cell)))
    assert (cell[H:] == POISON).all(), what
    assert np.array_equal(corner[:nc], d.cell_corner) and (corner[nc:] == POISON).all(), what           # D3: nothing behind n_cells
    bad = (DE.bits(point[:nc]) != DE.bits(d.cell_point)).any(1) if nc else np.zeros(0, bool)
    assert not bad.any(), "%s: %d of %d points differ, first cell %d: %s, not %s" % (what, int(bad.sum()), nc, int(np.argmax(bad)),
                                                                                   point[int(np.argmax(bad))], d.cell_point[int(np.argmax(bad))])
    assert (point[nc:] == POISON_F).all(), what
    assert np.array_equal(offsets[:n + 1], d.offsets), "%s: offsets differ first at %d" % (what, int(np.argmax(offsets[:n + 1] != d.offsets)))
    assert (offsets[n + 1:] == POISON).all(), what


def _full_points(d, n):
    """cell_point at the size the fill takes, 3 n points, with values behind n_cells that no output may show"""
    return np.concatenate([d.cell_point, np.full((3 * n - d.cell_point.shape[0], 3), -POISON_F, F)])


def _fill(lib, sg, R, cell, points, offsets, capacity, dev, shift=0, ids=True, stream=None, sync=True, out_shift=None):
    """ezrt_decimate_rows_device over poisoned buffers: tri36 starts `shift` floats and out `out_shift` floats (default: the same) into
    512-byte aligned allocations, and out and src have ROOM rows behind `capacity`.  Returns (out [capacity + ROOM, 36], src)."""
    n = R.shape[0]
    oshift = shift if out_shift is None else out_shift
    d_in = torch.full((shift + n * 36 + 36,), 3.0, dtype=torch.float32, device=dev)
    d_in[shift:shift + n * 36] = _g(R, dev, F).reshape(-1)
    d_out = torch.full((oshift + (capacity + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    src = torch.full((capacity + ROOM,), POISON, dtype=torch.int32, device=dev)
    d_cell, d_pts, d_off = _g(cell, dev, np.int32), _g(points, dev, F), _g(offsets, dev, np.int64)
    assert d_in.data_ptr() % 512 == 0 and d_out.data_ptr() % 512 == 0 and d_cell.numel() == 3 * n and d_pts.numel() == 9 * n and d_off.numel() == n + 1
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_decimate_rows_device(sg._h, P(d_in.data_ptr() + 4 * shift), n, P(d_cell.data_ptr()), P(d_pts.data_ptr()), P(d_off.data_ptr()),
                                        capacity, P(d_out.data_ptr() + 4 * oshift), P(src.data_ptr()) if ids else None,
                                        P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    def after():
        assert bool((d_out[:oshift] == POISON_F).all()) and np.array_equal(DE.bits(d_in[shift:shift + n * 36].cpu().numpy().reshape(-1, 36)), DE.bits(R))
        return d_out[oshift:].cpu().numpy().reshape(-1, 36), src.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_fill(got, rows, placed, capacity, ids=True, what=""):
    """`rows`: DE.row_of, D8 of every source row; `placed`: the (output row, source row) pairs of DE.candidates.  An output row with one
    candidate holds it; one with several (offsets that no count call left may send two source rows to one place, and which of them
    writes a word last is open) holds in every word the word of one of them; every other row holds the poison."""
    out, src = got
    assert out.shape[0] == capacity + ROOM
    by_row = {}
    for r, t in placed:
        by_row.setdefault(r, []).append(t)
    assert all(0 <= r < capacity for r in by_row)
    at = np.array(sorted(by_row), np.int64)
    single = np.array([len(by_row[r]) == 1 for r in at], bool)
    one = at[single]
    t1 = np.array([by_row[r][0] for r in one], np.int64)
    bad = (DE.bits(out[one]) != DE.bits(rows[t1])) & ~(np.isnan(out[one]) & np.isnan(rows[t1]))
    assert not bad.any(), "%s: %d rows differ, first output row %d" % (what, int(bad.any(1).sum()), int(one[np.argmax(bad.any(1))]))
    if ids:
        assert np.array_equal(src[one], t1), what
    for r in at[~single]:
        cand = rows[by_row[r]]
        assert ((DE.bits(cand) == DE.bits(out[r])[None]) | (np.isnan(cand) & np.isnan(out[r])[None])).any(0).all(), (what, r)
        assert not ids or src[r] in by_row[r], (what, r)
    rest = np.ones(capacity + ROOM, bool)
    rest[at] = False
    assert (out[rest] == POISON_F).all(), "%s: a row that belongs to no source row was written" % what
    assert (src[rest] == POISON).all() if ids else (src == POISON).all(), what


def _both(lib, sg, dev, key, R, g, flags, what):
    """count and fill of one case against the restatement"""
    n = R.shape[0]
    d = _want(key, R, g, flags)
    _same_count(_count(lib, sg, R, g, flags, dev), d, n, what)
    T = int(d.offsets[n])
    pts = _full_points(d, n)
    got = _fill(lib, sg, R, d.cell, pts, d.offsets, T, dev)
    _same_fill(got, DE.row_of(R, d.cell, pts), [(r, int(t)) for r, t in enumerate(d.src)], T, True, what)
    assert DE.same_rows(got[0][:T], d.out), what
    return d


@pytest.mark.parametrize("flags", (0, DE.DEDUP))
@pytest.mark.parametrize("n", DS.SIZES)
def test_decimation_on_the_bits(hip, sg, dev, n, flags):
    R = DS.sized(n)
    for div in DS.GRIDS:
        _both(hip.lib, sg, dev, ("sized", n, div), R, DS.grid(R, div), flags, "%d rows, div %d, flags %d" % (n, div, flags))


@pytest.mark.parametrize("name,div", (("sphere", 4), ("sphere", 8), ("sphere", 16), ("bunny", 8), ("bunny", 4096), ("sphere2", 16)))
def test_the_shipped_meshes(hip, sg, dev, name, div):
    R = DS.shipped(name)
    d = _both(hip.lib, sg, dev, (name, div), R, DS.grid(R, div), DE.DEDUP, "%s, div %d" % (name, div))
    for row in DS.TABLE:
        if row[:2] == (name, div):
            assert d.summary.tolist()[:5] == [row[2], row[4], row[5], 0, row[3]]
    if (name, div) in (("sphere", 16), ("bunny", 4096)):
        assert d.summary[4] * 2 > np.unique(DE.keys(R[:, :9]).reshape(-1, 3), axis=0).shape[0]   # near one corner's value per cell


def test_every_corner_in_one_cell(hip, sg, dev):
    R, g = DS.one_cell()
    d = _both(hip.lib, sg, dev, "one cell", R, g, DE.DEDUP, "61440 corners in one cell")
    assert d.summary.tolist() == [0, 20480, 0, 0, 1, 0, 1, 1]


@pytest.mark.parametrize("name", DS.EDGE_NAMES)
def test_the_edge_cases(hip, sg, dev, name):
    R, g = DS.edge(name)
    for flags in (0, DE.DEDUP):
        _both(hip.lib, sg, dev, ("edge", name), R, g, flags, "%s, flags %d" % (name, flags))


def test_what_work_holds_means_nothing_and_two_streams(hip, sg, dev):
    n = 2049
    R = DS.sized(n)
    g = DS.grid(R, 256)
    d = _want(("sized", n, 256), R, g, DE.DEDUP)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(DS.SEED + 11))):
        _same_count(_count(hip.lib, sg, R, g, DE.DEDUP, dev, work_fill=fill), d, n, "work=%s" % what)
    for off in (1, 3):                                                         # work is 8-byte aligned, and need not be more
        _same_count(_count(hip.lib, sg, R, g, DE.DEDUP, dev, work_fill=-1, work_off=off), d, n, "work %d bytes into its allocation" % (8 * off))
    R2 = DS.shipped("bunny")
    g2 = DS.grid(R2, 16)
    d2 = _want(("bunny", 16), R2, g2, 0)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    a1 = _count(hip.lib, sg, R, g, DE.DEDUP, dev, work_fill=-1, stream=s1, sync=False)
    a2 = _count(hip.lib, sg, R2, g2, 0, dev, work_fill=0, stream=s2, sync=False)
    T, T2 = int(d.summary[0]), int(d2.summary[0])
    p1, p2 = _full_points(d, n), _full_points(d2, R2.shape[0])
    f1 = _fill(hip.lib, sg, R, d.cell, p1, d.offsets, T, dev, stream=s1, sync=False)
    f2 = _fill(hip.lib, sg, R2, d2.cell, p2, d2.offsets, T2, dev, shift=1, stream=s2, sync=False)
    torch.cuda.synchronize()
    _same_count(a1(), d, n, "on a side stream")
    _same_count(a2(), d2, R2.shape[0], "on another side stream")
    _same_fill(f1(), DE.row_of(R, d.cell, p1), [(r, int(t)) for r, t in enumerate(d.src)], T, True, "on a side stream")
    _same_fill(f2(), DE.row_of(R2, d2.cell, p2), [(r, int(t)) for r, t in enumerate(d2.src)], T2, True, "on another side stream")


@pytest.mark.parametrize("n,div", ((257, 256), (2049, 256), (2049, 4096)))
def test_both_routes_give_the_same_bits(hip, sg, dev, n, div):
    """one row in, tri36 and out are still 16-byte aligned and take the staged route; 4 bytes in they take the per-lane route, and so
    does a call with only one of the two off the 16 bytes"""
    R = DS.sized(n)
    d = _want(("sized", n, div), R, DS.grid(R, div), DE.DEDUP)
    T = int(d.summary[0])
    assert T > n // 2
    pts = _full_points(d, n)
    rows, placed = DE.row_of(R, d.cell, pts), [(r, int(t)) for r, t in enumerate(d.src)]
    for shift, ids in ((36, True), (1, True), (37, False), (2, True), (3, True)):
        _same_fill(_fill(hip.lib, sg, R, d.cell, pts, d.offsets, T, dev, shift=shift, ids=ids), rows, placed, T, ids, "%d rows, %d floats in" % (n, shift))
    for shift, oshift in ((0, 1), (3, 0), (36, 2), (1, 72)):                   # tri36 aligned and out not, and the other way round
        _same_fill(_fill(hip.lib, sg, R, d.cell, pts, d.offsets, T, dev, shift=shift, out_shift=oshift), rows, placed, T, True,
                   "%d rows, tri36 %d and out %d floats in" % (n, shift, oshift))


@pytest.mark.parametrize("shift", (0, 1))
def test_capacity_offsets_and_cells_that_no_count_left(hip, sg, dev, shift):
    """D10: whatever offsets and cell hold, a row is written whole or not at all and nothing outside [0, capacity) is touched"""
    n = 2049
    R = DS.sized(n)
    d = _want(("sized", n, 4096), R, DS.grid(R, 4096), DE.DEDUP)
    T = int(d.summary[0])
    assert T > n // 2
    pts = _full_points(d, n)
    rng = np.random.default_rng(DS.SEED + 31)
    i64 = np.int64
    some = d.offsets.copy()
    k = rng.integers(0, n + 1, n // 20)
    some[k] = rng.choice(i64([-2 ** 63, 2 ** 63 - 1, -1, T, T + 1, 0, 1]), k.size)
    cases = [("capacity T - 1", d.offsets, T - 1), ("capacity T / 2", d.offsets, T // 2), ("capacity 1", d.offsets, 1), ("capacity 0", d.offsets, 0),
             ("negative", d.offsets - T - 5, T), ("descending", d.offsets[::-1].copy(), T), ("shifted by one", d.offsets + 1, T),
             ("shifted by one, room for it", d.offsets + 1, T + 1), ("random", rng.integers(-5, T + 5, n + 1).astype(i64), T),
             ("random bits", rng.integers(-2 ** 63, 2 ** 63 - 1, n + 1, dtype=i64), T), ("5 % overwritten", some, T),
             ("all zero", np.zeros(n + 1, i64), T), ("all INT64_MAX", np.full(n + 1, 2 ** 63 - 1, i64), T), ("every row", np.arange(n + 1, dtype=i64), n)]
    rows = DE.row_of(R, d.cell, pts)
    for name, off, cap in cases:
        placed = DE.candidates(n, d.cell, off, cap)
        if name in ("capacity T / 2", "shifted by one, room for it", "5 % overwritten", "every row"):
            assert placed
        if name in ("negative", "capacity 0", "all INT64_MAX", "shifted by one", "descending"):
            assert len(placed) < T
        _same_fill(_fill(hip.lib, sg, R, d.cell, pts, off, cap, dev, shift=shift), rows, placed, cap, True, name)
    # cells that no count left: out of range on either side, equal entries, random words, and any cell below 3 n, used or not
    H = 3 * n
    i32 = np.int32
    for name, cell in (("out of range", np.where(rng.random(H) < 0.1, rng.choice(i32([-1, -2 ** 31, H, H + 1, 2 ** 31 - 1]), H), d.cell).astype(i32)),
                       ("equal entries", np.where((np.arange(H) % 3 == 1) & (rng.random(H) < 0.3), np.roll(d.cell, 1), d.cell).astype(i32)),
                       ("random words", rng.integers(-2 ** 31, 2 ** 31 - 1, H, dtype=np.int64).astype(i32)),
                       ("any cell below 3 n", rng.integers(0, H, H).astype(i32))):
        placed = DE.candidates(n, cell, d.offsets, T)
        assert len(placed) < T or name == "any cell below 3 n"
        _same_fill(_fill(hip.lib, sg, R, cell, pts, d.offsets, T, dev, shift=shift), DE.row_of(R, cell, pts), placed, T, True, name)


def test_a_chain_decimate_topology_subdivide_decimate(hip, sg, dev):
    R = DS.shipped("sphere")
    g = DS.grid(R, 8)
    d = _want(("sphere", 8), R, g, DE.DEDUP)
    got = query.decimate_rows(sg, _g(R, dev, F), float(g[3]), origin=[float(x) for x in g[:3]])
    torch.cuda.synchronize()
    assert DE.same_rows(got.rows.cpu().numpy(), d.out) and got.rows.shape[0] == 294
    coarse = hip.scene_create(got.rows.cpu().numpy(), BS.proxy_nodes(got.rows.shape[0]))
    topo = query.mesh_topology(coarse)
    assert topo.closed and DE.closed(d.out)
    sub = query.subdivide_rows(sg, got.rows)                                   # midpoint mode: four rows per row
    fine = query.decimate_rows(sg, sub.rows, 2.0 ** -12, origin=[float(x) for x in g[:3]])
    torch.cuda.synchronize()
    assert fine.summary.tolist()[:4] == [4 * 294, 0, 0, 0] and int(fine.summary[5]) == int(fine.summary[4]) == 149 + 294 * 3 // 2
    assert np.array_equal(DE.bits(fine.rows[:, :9].cpu().numpy()), DE.keys(sub.rows[:, :9].cpu().numpy()))   # on the bits, -0 as +0
    assert np.array_equal(DE.bits(fine.rows[:, 18:].cpu().numpy()), DE.bits(sub.rows[:, 18:].cpu().numpy()))
    assert np.array_equal(fine.src.cpu().numpy(), np.arange(4 * 294))


def test_the_wrapper(hip, sg, dev):
    for i, (name, div) in enumerate((("sphere", 4), ("bunny", 16), ("sphere", 16), ("bunny", 8))):
        R = DS.shipped(name)
        g = DS.grid(R, div)
        kw = ({}, {"stream": torch.cuda.Stream(dev)}, {"src": False}, {"dedup": False})[i]
        d = _want((name, div), R, g, 0 if "dedup" in kw else DE.DEDUP)
        if "stream" in kw:
            kw["stream"].wait_stream(torch.cuda.current_stream(dev))
        got = query.decimate_rows(sg, _g(R, dev, F), float(g[3]), origin=tuple(float(x) for x in g[:3]), **kw)
        torch.cuda.synchronize()
        n, nc = R.shape[0], int(d.summary[4])
        assert isinstance(got, query.DecimatedRows) and got.n_rows == n and got.rows.dtype == torch.float32
        assert tuple(got.rows.shape) == (int(d.summary[0]), 36) and np.array_equal(got.summary.cpu().numpy(), d.summary), (name, div)
        assert DE.same_rows(got.rows.cpu().numpy(), d.out), (name, div)
        assert got.cell.dtype == torch.int32 and tuple(got.cell.shape) == (n, 3) and np.array_equal(got.cell.cpu().numpy().reshape(-1), d.cell)
        assert tuple(got.cell_point.shape) == (nc, 3) and np.array_equal(DE.bits(got.cell_point.cpu().numpy()), DE.bits(d.cell_point))
        if kw.get("src", True):
            assert got.src.dtype == torch.int32 and np.array_equal(got.src.cpu().numpy(), d.src)
        else:
            assert got.src is None
    R = DS.shipped("sphere")
    dead = query.decimate_rows(sg, _g(R, dev, F), 0.0)
    assert dead.summary.tolist() == [0, 0, 0, 320, 0, 0, 1, 0] and tuple(dead.rows.shape) == (0, 36) and bool((dead.cell == -1).all())
    empty = query.decimate_rows(sg, torch.zeros((0, 36), dtype=torch.float32, device=dev), 1.0)
    assert tuple(empty.rows.shape) == (0, 36) and empty.summary.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and empty.n_rows == 0 and empty.src.numel() == 0
    assert tuple(empty.cell.shape) == (0, 3) and tuple(empty.cell_point.shape) == (0, 3)


def test_untouched_state(hip, bunny_small, dev):
    from ezrt_amd import scene as S
    from ezrt_amd import scenes, trace
    scn = bunny_small.upload(hip)
    tri = np.ascontiguousarray(bunny_small.tri, np.float32).reshape(-1, 36)
    rows = torch.from_numpy(tri).to(dev)                                       # (the inputs first: nothing but the call between the two reads)
    g = DS.grid(tri, 16)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    scn.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (scn.counters(), scn.last_render_ms())
    assert before[0]["rays"] > 0
    got = query.decimate_rows(scn, rows, float(g[3]), origin=[float(x) for x in g[:3]])
    torch.cuda.synchronize()
    assert 0 < got.rows.shape[0] < rows.shape[0] and (scn.counters(), scn.last_render_ms()) == before


def test_errors(hip, sg, oracle, bunny_small, dev):
    lib = hip.lib
    n = 300
    R = DS.shipped("sphere")[:n]
    grid = DS.grid(R, 8)
    d = DE.decimate(R, grid)
    T = int(d.offsets[n])
    assert 0 < T < n
    wb = lib.ezrt_decimate_work_bytes(n)
    full = lambda k, dt: torch.full((k,), 5, dtype=dt, device=dev)
    bufs = dict(tri36=_g(R, dev, F), grid4=_g(grid, dev, F), cell=full(3 * n, torch.int32), cell_corner=full(3 * n, torch.int32),
                cell_point=full(9 * n, torch.float32), offsets=full(n + 1, torch.int64), summary=full(8, torch.int64),
                work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    host = np.zeros(max(36 * (n + T), wb // 8 + 64), np.int64)
    hp = P(host.ctypes.data)
    torch.cuda.synchronize()
    f = lib.ezrt_decimate_count_device
    dp = lambda x: P(x.data_ptr())

    def fa(**kw):
        g = lambda k: kw[k] if k in kw else dp(bufs[k])
        return [kw.get("s", sg._h), g("tri36"), kw.get("n_rows", n), g("grid4"), kw.get("flags", 1), g("cell"), g("cell_corner"), g("cell_point"),
                g("offsets"), g("summary"), g("work"), kw.get("work_bytes", wb), None]
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + list(bufs):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in bufs:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    for flags in (2, 3, -1, 1 << 30):
        assert f(*fa(flags=flags)) == EZRT_ERR_INVALID and b"EZRT_DECIMATE_DEDUP" in lib.ezrt_last_error(), flags
    assert f(*fa(n_rows=-1)) == EZRT_ERR_INVALID and f(*fa(n_rows=(2 ** 31 - 1) // 3 + 1, work_bytes=2 ** 44)) == EZRT_ERR_INVALID
    assert b"INT32_MAX / 3" in lib.ezrt_last_error()
    assert f(*fa(n_rows=0)) == 0                                               # launches nothing
    torch.cuda.synchronize()
    for k in ("cell", "cell_corner", "cell_point", "offsets", "summary"):
        assert bool((bufs[k] == 5).all()), k
    assert not host.any()
    # the fill
    g = lib.ezrt_decimate_rows_device
    fb = dict(tri36=bufs["tri36"], cell=_g(d.cell, dev, np.int32), cell_point=_g(_full_points(d, n), dev, F), offsets=_g(d.offsets, dev, np.int64),
              out=torch.full((T, 36), 5.0, dtype=torch.float32, device=dev), src=full(T, torch.int32))

    def ga(**kw):
        h = lambda k: kw[k] if k in kw else dp(fb[k])
        return [kw.get("s", sg._h), h("tri36"), kw.get("n_rows", n), h("cell"), h("cell_point"), h("offsets"), kw.get("capacity", T), h("out"), h("src"), None]
    for k in ("s", "tri36", "cell", "cell_point", "offsets", "out"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in fb:
        assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert g(*ga(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(capacity=2 ** 62)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(n_rows=-1)) == EZRT_ERR_INVALID and g(*ga(n_rows=(2 ** 31 - 1) // 3 + 1)) == EZRT_ERR_INVALID
    # out overlapping tri36: the same rows, rows that begin inside tri36, rows that end inside it
    both = torch.full((2 * n + T, 36), 5.0, dtype=torch.float32, device=dev)
    both[n:2 * n] = bufs["tri36"]
    torch.cuda.synchronize()
    at = lambda row: P(both.data_ptr() + 144 * row)
    for out_row, cap in ((n, T), (2 * n - 1, 1), (n - 1, 2), (n - T + 1, T), (n, 1)):
        assert g(*ga(tri36=at(n), out=at(out_row), capacity=cap)) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error(), (out_row, cap)
    assert g(*ga(tri36=at(n), out=at(2 * n), capacity=T, src=None)) == 0      # behind it: no overlap
    assert g(*ga(tri36=at(n), out=at(n - 1), capacity=1, src=None)) == 0      # before it
    assert g(*ga(n_rows=0)) == 0 and g(*ga(capacity=0, out=None)) == 0
    torch.cuda.synchronize()
    assert bool((fb["out"] == 5.0).all()) and bool((fb["src"] == 5).all()) and not host.any()
    assert DE.same_rows(both[2 * n:].cpu().numpy(), d.out) and DE.same_rows(both[n - 1:n].cpu().numpy(), d.out[:1])
    # the rejected calls left no HIP error behind: the next call works
    _same_count(_count(lib, sg, R, grid, 1, dev), d, n, "after the rejected calls")
    assert g(*ga(src=None)) == 0
    torch.cuda.synchronize()
    assert DE.same_rows(fb["out"].cpu().numpy(), d.out) and bool((fb["src"] == 5).all())
    # the wrapper
    rows = bufs["tri36"]
    with pytest.raises(TypeError):
        query.decimate_rows(bunny_small.upload(oracle), rows, 1.0)
    with pytest.raises(TypeError):
        query.decimate_rows(sg, rows.cpu(), 1.0)
    with pytest.raises(TypeError):
        query.decimate_rows(sg, rows.to(torch.float64), 1.0)
    with pytest.raises(ValueError):
        query.decimate_rows(sg, rows[:, :35], 1.0)
    with pytest.raises(ValueError):
        query.decimate_rows(sg, rows.reshape(2, -1, 36), 1.0)
    with pytest.raises(ValueError):
        query.decimate_rows(sg, rows, 1.0, origin=(0, 0))
    with pytest.raises(ValueError):
        query.decimate_rows(sg, rows, 1.0, dedup=1)

"""Isosurface extraction on device tensors (include/ezrt_isosurface.h, ezrt_amd/query.py: isosurface_rows, grid_points).

Every output of both calls -- offsets, summary; out, cell -- is compared EXACTLY with tests/iso_expected.py, the header's rules restated
in numpy and held to their properties by tests/test_iso_expected.py.  There is no tolerance anywhere (a NaN normal is a NaN).

* the smallest grids that can go wrong -- one cell, less than a wave, exactly two blocks, blocks ending mid-row, an x-row longer than a
  wave, one cell per x-row, no cells -- over poisoned buffers with room behind them; a grid of more than 2048 blocks with a sparse
  surface (the scan's second tile; most blocks are skipped);
* the field with all 256 cell cases; dense noise whose blocks emit several staging rounds; values at the level, -0 against a level
  of +0, NaN and infinite values; each way for a grid not to be live;
* `work` pre-filled with zeros, with 0xFF and with noise; two calls on two streams;
* the staged and the per-lane route of the fill (out offset by one row, and by 4 bytes) give the same bits; capacity below T and
  offsets that no count call left: blocks are whole or absent, nothing outside [0, capacity) is touched;
* two chains: a 65^3 sphere field, a scene of the rows, closed and oriented, V - E + F = 2, the volume on the bits; the signed
  distance of the shipped cube on grid_points, the offset surface, closed and oriented, equal to the restatement;
* the wrapper, the untouched counters, the error contract.  Nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ezrt_amd import _abi, query

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_scenes as BS  # noqa: E402
import inside_scenes as INS  # noqa: E402
import iso_expected as IE  # noqa: E402
import iso_scenes as IS  # noqa: E402
import orient_expected as OE  # noqa: E402
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


def _want(key, V, g):
    """the restatement's Iso, computed once and shared"""
    if key not in _cache:
        _cache[key] = IE.iso(V, g, IS.MATERIAL)
    return _cache[key]


def _g(x, dev, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev)                        # (a copy: the fields are handed out read-only)


def _dims(V):
    nz, ny, nx = V.shape
    return nx, ny, nz


def _count(lib, sg, V, grid, dev, work_fill=FILL, stream=None, sync=True, work_off=0):
    """ezrt_iso_count_device over poisoned buffers with ROOM entries behind their stated size; `work` begins work_off int64 into a
    512-byte aligned allocation"""
    nx, ny, nz = _dims(V)
    nb = IE.n_blocks_of(V.shape)
    d_val = _g(np.concatenate([V.reshape(-1), np.full(8, np.nan, F)]), dev, F)  # guard values behind the grid: NaN, so a cell that read one emits nothing
    d_grid = _g(grid, dev, F)
    offsets = torch.full((nb + 1 + ROOM,), POISON, dtype=torch.int64, device=dev)
    summary = torch.full((8 + ROOM,), POISON, dtype=torch.int64, device=dev)
    wb = lib.ezrt_iso_work_bytes(nx, ny, nz)
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
    got = lib.ezrt_iso_count_device(sg._h, P(d_val.data_ptr()), nx, ny, nz, P(d_grid.data_ptr()), P(offsets.data_ptr()), P(summary.data_ptr()),
                                    P(work.data_ptr()), wb, P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    alive = (d_val, d_grid, offsets, summary, whole)                           # until the stream is done: a tensor freed here is handed out again at once

    def after():
        assert len(alive) == 5
        assert bool((work[wb // 8:] == tail).all()) and bool((whole[:work_off] == head).all())   # nothing outside the stated bytes of work
        assert np.array_equal(IE.bits(d_val[:V.size].cpu().numpy()), IE.bits(V.reshape(-1)))
        return offsets.cpu().numpy(), summary.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_count(got, I, what=""):
    offsets, summary = got
    nb = I.offsets.size - 1
    assert np.array_equal(summary[:8], I.summary) and (summary[8:] == POISON).all(), "%s: summary %s, not %s" % (what, summary[:8].tolist(), I.summary.tolist())
    assert np.array_equal(offsets[:nb + 1], I.offsets), "%s: offsets differ first at %d" % (what, int(np.argmax(offsets[:nb + 1] != I.offsets)))
    assert (offsets[nb + 1:] == POISON).all(), what


def _fill(lib, sg, V, grid, offsets, capacity, dev, shift=0, ids=True, stream=None, sync=True):
    """ezrt_iso_rows_device over poisoned buffers: out starts `shift` floats into a 512-byte aligned allocation, and out and cell have
    ROOM rows behind `capacity`.  Returns (out [capacity + ROOM, 36], cell)."""
    nx, ny, nz = _dims(V)
    d_val = _g(np.concatenate([V.reshape(-1), np.full(8, np.nan, F)]), dev, F)
    d_grid, d_mat, d_off = _g(grid, dev, F), _g(IS.MATERIAL, dev, F), _g(offsets, dev, np.int64)
    d_out = torch.full((shift + (capacity + ROOM) * 36,), POISON_F, dtype=torch.float32, device=dev)
    cell = torch.full((capacity + ROOM,), POISON, dtype=torch.int32, device=dev)
    assert d_out.data_ptr() % 512 == 0 and d_off.numel() == IE.n_blocks_of(V.shape) + 1
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    else:
        torch.cuda.synchronize()
    got = lib.ezrt_iso_rows_device(sg._h, P(d_val.data_ptr()), nx, ny, nz, P(d_grid.data_ptr()), P(d_mat.data_ptr()), P(d_off.data_ptr()), capacity,
                                   P(d_out.data_ptr() + 4 * shift), P(cell.data_ptr()) if ids else None,
                                   P(stream.cuda_stream) if stream is not None else None)
    assert got == 0, lib.ezrt_last_error()

    alive = (d_val, d_grid, d_mat, d_off, d_out, cell)                         # until the stream is done: a tensor freed here is handed out again at once

    def after():
        assert len(alive) == 6
        assert bool((d_out[:shift] == POISON_F).all()) and np.array_equal(IE.bits(d_val[:V.size].cpu().numpy()), IE.bits(V.reshape(-1)))
        return d_out[shift:].cpu().numpy().reshape(-1, 36), cell.cpu().numpy()
    if not sync:
        return after
    torch.cuda.synchronize()
    return after()


def _same_fill(got, I, placed, capacity, ids=True, what=""):
    """`placed`: the (output row, row of I.out) pairs of IE.candidates.  An output row with one candidate holds it; one with several
    (offsets that no count call left may send two blocks to one place, and which of them writes a word last is open) holds in every
    word the word of one of them; every other row holds the poison."""
    out, cell = got
    assert out.shape[0] == capacity + ROOM
    by_row = {}
    for r, t in placed:
        by_row.setdefault(r, []).append(t)
    assert all(0 <= r < capacity for r in by_row)
    at = np.array(sorted(by_row), np.int64)
    single = np.array([len(by_row[r]) == 1 for r in at], bool)
    one = at[single]
    t1 = np.array([by_row[r][0] for r in one], np.int64)
    bad = (IE.bits(out[one]) != IE.bits(I.out[t1])) & ~(np.isnan(out[one]) & np.isnan(I.out[t1]))
    assert not bad.any(), "%s: %d rows differ, first output row %d: %s, not %s" % (
        what, int(bad.any(1).sum()), int(one[np.argmax(bad.any(1))]), out[one][np.argmax(bad.any(1))][:18], I.out[t1][np.argmax(bad.any(1))][:18])
    if ids:
        assert np.array_equal(cell[one], I.cell[t1]), what
    for r in at[~single]:
        cand = I.out[by_row[r]]
        assert ((IE.bits(cand) == IE.bits(out[r])[None]) | (np.isnan(cand) & np.isnan(out[r])[None])).any(0).all(), (what, r)
        assert not ids or cell[r] in I.cell[by_row[r]], (what, r)
    rest = np.ones(capacity + ROOM, bool)
    rest[at] = False
    assert (out[rest] == POISON_F).all(), "%s: a row that belongs to no block was written" % what
    assert (cell[rest] == POISON).all() if ids else (cell == POISON).all(), what


def _straight(I):
    T = I.out.shape[0]
    return [(r, r) for r in range(T)]


def _both(lib, sg, dev, key, V, g, what):
    """count and fill of one case against the restatement"""
    I = _want(key, V, g)
    _same_count(_count(lib, sg, V, g, dev), I, what)
    T = int(I.offsets[-1])
    got = _fill(lib, sg, V, g, I.offsets, T, dev)
    _same_fill(got, I, _straight(I), T, True, what)
    assert IE.same_rows(got[0][:T], I.out), what
    return I


@pytest.mark.parametrize("dims", IS.DIMS)
def test_the_smallest_grids_on_the_bits(hip, sg, dev, dims):
    nx, ny, nz = dims
    for seed, padded in ((0, False), (1, True)):
        V, g = IS.noise(dims, padded and min(dims) > 2, seed)
        assert V.shape == (nz, ny, nx)
        I = _both(hip.lib, sg, dev, ("noise", dims, seed), V, g, "%s, seed %d" % (dims, seed))
        assert I.summary[5] == (nx - 1) * (ny - 1) * (nz - 1) and I.summary[0] > 0
    assert {(2, 2, 2): 1, (5, 4, 3): 1, (17, 9, 5): 2, (19, 7, 6): 3, (67, 5, 3): 3, (2, 9, 40): 2}[dims] == IE.n_blocks_of((nz, ny, nx))
    if dims == (17, 9, 5):
        assert I.summary[5] == 512
    if dims == (19, 7, 6):
        assert I.summary[5] == 540


def test_no_cells(hip, sg, dev):
    lib = hip.lib
    buf = torch.full((64,), 5.0, dtype=torch.float32, device=dev)
    i8 = torch.full((16,), 5, dtype=torch.int64, device=dev)
    work = torch.full((4,), 5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for nx, ny, nz in IS.NO_CELLS:
        assert lib.ezrt_iso_work_bytes(nx, ny, nz) == 8
        assert lib.ezrt_iso_count_device(sg._h, P(buf.data_ptr()), nx, ny, nz, P(buf.data_ptr()), P(i8.data_ptr()), P(i8.data_ptr() + 64), P(work.data_ptr()), 8,
                                         None) == 0, lib.ezrt_last_error()
        assert lib.ezrt_iso_rows_device(sg._h, P(buf.data_ptr()), nx, ny, nz, P(buf.data_ptr()), P(buf.data_ptr()), P(i8.data_ptr()), 1,
                                        P(buf.data_ptr() + 128), None, None) == 0, lib.ezrt_last_error()
        got = query.isosurface_rows(sg, torch.zeros((nz, ny, nx), dtype=torch.float32, device=dev), 0.5)
        assert tuple(got.rows.shape) == (0, 36) and got.cell.numel() == 0 and got.summary.tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and got.shape == (nz, ny, nx)
    dead = query.isosurface_rows(sg, torch.zeros((1, 5, 5), dtype=torch.float32, device=dev), 0.5, spacing=0.0)
    assert dead.summary.tolist() == [0] * 8
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all()) and bool((i8 == 5).all()) and bool((work == 5).all())


def test_a_sparse_surface_in_more_than_2048_blocks(hip, sg, dev):
    V, g = IS.sparse_large()
    I = _both(hip.lib, sg, dev, "sparse_large", V, g, "sparse, 2130 blocks")
    nb = I.offsets.size - 1
    assert nb == 2130 > 2048 and hip.lib.ezrt_iso_work_bytes(*_dims(V)) == 24
    emits = np.diff(I.offsets) > 0
    assert 0 < I.summary[4] == emits.sum() < nb // 4 and emits[2048:].any() and emits[:2048].any()   # rows behind the second tile's sum
    n, nv, ne, nf, ok = IE.topology(I.out)
    assert ok and nv - ne + nf == 4                                            # two spheres


def test_all_256_cell_cases(hip, sg, dev):
    V, g = IS.patterns()
    I = _both(hip.lib, sg, dev, "patterns", V, g, "patterns")
    assert np.unique(IE.classify(V, g)[1]).size == 256 and I.summary[0] > 1000


def test_dense_noise_several_staging_rounds(hip, sg, dev):
    V, g = IS.noise()
    I = _both(hip.lib, sg, dev, "noise", V, g, "dense noise")
    per_block = np.diff(I.offsets)
    assert per_block.max() > 4 * 256 and I.counts.max() >= 10                  # a block emits more rows than four staging rounds hold
    ends = (I.offsets[1:] - I.offsets[:-1]) % 256
    assert (ends != 0).any()                                                   # and its last round is not full


@pytest.mark.parametrize("name", ("special", "at_level", "sphere", "torus"))
def test_special_values_and_closed_surfaces(hip, sg, dev, name):
    V, g = getattr(IS, name)()
    I = _both(hip.lib, sg, dev, name, V, g, name)
    if name == "special":
        assert I.summary[3] > 0 and np.isnan(V).any() and np.isinf(V).any() and (np.signbit(V) & (V == 0)).any() and ((V == 0) & ~np.signbit(V)).any()
    if name == "at_level":
        assert np.isnan(I.out[:, 9:18]).any()                                  # degenerate rows are emitted, with NaN normals


def test_grids_that_are_not_live(hip, sg, dev):
    V, _ = IS.special()
    for name, g in IS.not_live():
        I = _want(("dead", name), V, g)
        assert I.summary[6] == 0 and I.summary[0] == 0 and I.summary[3] > 0
        _same_count(_count(hip.lib, sg, V, g, dev), I, name)
        live = _want("special", V, IS.special()[1])
        got = _fill(hip.lib, sg, V, g, live.offsets, int(live.offsets[-1]), dev)   # offsets of a live grid: the count is recomputed, nothing fits it
        _same_fill(got, I, [], int(live.offsets[-1]), True, name)


def test_what_work_holds_means_nothing_and_two_streams(hip, sg, dev):
    V, g = IS.sparse_large()
    I = _want("sparse_large", V, g)
    for what, fill in (("zeros", 0), ("0xFF", -1), ("noise", np.random.default_rng(IS.SEED + 11))):
        _same_count(_count(hip.lib, sg, V, g, dev, work_fill=fill), I, "work=%s" % what)
    for off in (1, 3):                                                         # work is 8-byte aligned, and need not be more
        _same_count(_count(hip.lib, sg, V, g, dev, work_fill=-1, work_off=off), I, "work %d bytes into its allocation" % (8 * off))
    V2, g2 = IS.noise()
    I2 = _want("noise", V2, g2)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)                    # two calls in flight, two work buffers
    a1 = _count(hip.lib, sg, V, g, dev, work_fill=-1, stream=s1, sync=False)
    a2 = _count(hip.lib, sg, V2, g2, dev, work_fill=0, stream=s2, sync=False)
    T, T2 = int(I.summary[0]), int(I2.summary[0])
    f1 = _fill(hip.lib, sg, V, g, I.offsets, T, dev, stream=s1, sync=False)
    f2 = _fill(hip.lib, sg, V2, g2, I2.offsets, T2, dev, shift=1, stream=s2, sync=False)
    torch.cuda.synchronize()
    _same_count(a1(), I, "on a side stream")
    _same_count(a2(), I2, "on another side stream")
    _same_fill(f1(), I, _straight(I), T, True, "on a side stream")
    _same_fill(f2(), I2, _straight(I2), T2, True, "on another side stream")


@pytest.mark.parametrize("name", ("noise", "patterns", "at_level"))
def test_both_routes_give_the_same_bits(hip, sg, dev, name):
    """one row in, out is still 16-byte aligned and takes the staged route; 4, 8 or 12 bytes in it takes the per-lane route"""
    V, g = getattr(IS, name)()
    I = _want(name, V, g)
    T = int(I.summary[0])
    for shift, ids in ((36, True), (1, True), (37, False), (2, True), (3, True), (4, False)):
        _same_fill(_fill(hip.lib, sg, V, g, I.offsets, T, dev, shift=shift, ids=ids), I, _straight(I), T, ids, "%s, %d floats in" % (name, shift))


@pytest.mark.parametrize("shift", (0, 1))
def test_capacity_and_offsets_that_no_count_left(hip, sg, dev, shift):
    """G9: whatever offsets holds, a block is written whole or not at all and nothing outside [0, capacity) is touched"""
    i64 = np.int64
    for name in ("noise", "sphere", "patterns"):
        V, g = getattr(IS, name)()
        I = _want(name, V, g)
        T = int(I.summary[0])
        nb = I.offsets.size - 1
        rng = np.random.default_rng(IS.SEED + 31)
        some = I.offsets.copy()
        k = rng.integers(0, nb + 1, max(nb // 4, 2))
        some[k] = rng.choice(i64([-2 ** 63, 2 ** 63 - 1, -1, T, T + 1, 0, 1]), k.size)
        first = int(np.diff(I.offsets).max())
        cases = [("capacity T - 1", I.offsets, T - 1), ("capacity T / 2", I.offsets, T // 2), ("capacity 1", I.offsets, 1), ("capacity 0", I.offsets, 0),
                 ("negative", I.offsets - T - 5, T), ("descending", I.offsets[::-1].copy(), T), ("shifted by one", I.offsets + 1, T),
                 ("shifted by one, room for it", I.offsets + 1, T + 1), ("random", rng.integers(-5, T + 5, nb + 1).astype(i64), T),
                 ("random bits", rng.integers(-2 ** 63, 2 ** 63 - 1, nb + 1, dtype=i64), T), ("some overwritten", some, T),
                 ("all zero", np.zeros(nb + 1, i64), T), ("all INT64_MAX", np.full(nb + 1, 2 ** 63 - 1, i64), T),
                 ("all INT64_MIN", np.full(nb + 1, -2 ** 63, i64), T), ("alternating extremes", np.where(np.arange(nb + 1) % 2, 2 ** 63 - 1, -2 ** 63).astype(i64), T),
                 ("wrong difference", I.offsets + np.arange(nb + 1), T + nb), ("room for the largest block only", I.offsets, first)]
        for what, off, cap in cases:
            placed = IE.candidates(I, off, cap)
            if what in ("capacity T / 2", "shifted by one, room for it"):
                assert placed
            if what in ("negative", "capacity 0", "all INT64_MAX", "all INT64_MIN", "shifted by one", "descending", "wrong difference", "capacity T - 1"):
                assert len(placed) < T
            _same_fill(_fill(hip.lib, sg, V, g, off, cap, dev, shift=shift), I, placed, cap, True, "%s: %s" % (name, what))


def _scene_of(hip, rows):
    R = np.ascontiguousarray(rows, F)
    return hip.scene_create(R, BS.proxy_nodes(R.shape[0]))


def test_a_chain_sphere_field_to_a_closed_oriented_mesh(hip, sg, dev):
    V, g = IS.sphere(65)
    I = _want("sphere65", V, g)
    got = query.isosurface_rows(sg, _g(V, dev, F), float(g[6]), origin=[float(x) for x in g[:3]], spacing=[float(x) for x in g[3:6]],
                                material=[float(x) for x in IS.MATERIAL])
    torch.cuda.synchronize()
    assert IE.same_rows(got.rows.cpu().numpy(), I.out) and np.array_equal(got.cell.cpu().numpy(), I.cell)
    assert np.array_equal(got.summary.cpu().numpy(), I.summary) and got.rows.shape[0] > 50000
    mesh = _scene_of(hip, got.rows.cpu().numpy())
    topo = query.mesh_topology(mesh)
    weld = query.mesh_weld(mesh)
    assert topo.closed and topo.oriented
    assert query.euler_characteristic(weld, topo) == 2
    o = query.mesh_orient(mesh, topo)
    assert o.n_patch == 1 and int(o.flip.sum()) == 0 and o.pflags.tolist() == [0]
    P9 = OE.vertices(I.out)
    S = OE.scale(P9, np.ones(P9.shape[0], bool))
    want = np.float64(sum(OE.q_of(P9, S))) * 2.0 ** S / 6
    vol = query.patch_volume(o).tolist()
    assert o.scale == S and vol == [float(want)] and vol[0] > 0
    assert vol[0] == pytest.approx(IE.volume(I.out), rel=1e-6)


def test_a_chain_offset_surface_of_the_shipped_cube(hip, sg, dev):
    from ezrt_amd import scenes
    v, f = scenes.mesh("quad")                                                 # the shipped cube: 12 triangles, [-0.5, 0.5]^3
    cube = hip.scene_create(*INS.build(INS.tri36(np.ascontiguousarray(v[f], F))))
    shape, origin, spacing, r = (21, 23, 25), (-1.0, -1.1, -1.0), (2.0 / 24, 2.2 / 22, 0.1), 0.2
    pts = query.grid_points(shape, origin, spacing, dev)
    g = IE.grid8(origin, spacing, r)
    assert np.array_equal(IE.bits(pts.cpu().numpy()), IE.bits(IE.positions(shape, g)))   # G2 on the bits
    sd = query.signed_distance(cube, pts)
    values = sd.dist.reshape(shape)
    got = query.isosurface_rows(cube, values, r, origin, spacing)
    torch.cuda.synchronize()
    Vh = values.cpu().numpy()
    assert (Vh < 0).any() and np.isfinite(Vh).all()
    I = IE.iso(Vh, g)                                                          # the restatement fed with the same values read back
    assert IE.same_rows(got.rows.cpu().numpy(), I.out) and np.array_equal(got.cell.cpu().numpy(), I.cell) and got.rows.shape[0] > 1000
    assert np.array_equal(got.summary.cpu().numpy(), I.summary) and not bool((got.rows[:, 18:] != 0).any())
    mesh = _scene_of(hip, got.rows.cpu().numpy())
    topo = query.mesh_topology(mesh)
    assert topo.closed and topo.oriented
    o = query.mesh_orient(mesh, topo)
    vol = float(query.patch_volume(o)[0])
    exact = 1 + 6 * r + 3 * np.pi * r * r + 4.0 / 3.0 * np.pi * r ** 3         # the Minkowski sum of the unit cube and a ball
    assert o.n_patch == 1 and int(o.flip.sum()) == 0 and 0.9 * exact < vol < exact   # (the tets cut the rounded edges from inside)


def test_the_wrapper(hip, sg, dev):
    for i, name in enumerate(("sphere", "torus", "noise", "special")):
        V, g = getattr(IS, name)()
        kw = ({}, {"stream": torch.cuda.Stream(dev)}, {"cell": False}, {"stream": torch.cuda.Stream(dev).cuda_stream})[i]
        I = _want(name, V, g)
        if isinstance(kw.get("stream"), torch.cuda.Stream):
            kw["stream"].wait_stream(torch.cuda.current_stream(dev))
        else:
            torch.cuda.synchronize()
        h = [float(x) for x in g[3:6]]
        got = query.isosurface_rows(sg, _g(V, dev, F), float(g[6]), origin=tuple(float(x) for x in g[:3]), spacing=h[0] if h[0] == h[1] == h[2] else h,
                                    material=[float(x) for x in IS.MATERIAL], **kw)
        torch.cuda.synchronize()
        assert isinstance(got, query.IsoRows) and got.shape == V.shape and got.rows.dtype == torch.float32
        assert tuple(got.rows.shape) == (int(I.summary[0]), 36) and np.array_equal(got.summary.cpu().numpy(), I.summary), name
        assert IE.same_rows(got.rows.cpu().numpy(), I.out), name
        if kw.get("cell", True):
            assert got.cell.dtype == torch.int32 and np.array_equal(got.cell.cpu().numpy(), I.cell)
        else:
            assert got.cell is None
    V, g = IS.sphere()
    none = query.isosurface_rows(sg, _g(V, dev, F), 100.0)
    assert tuple(none.rows.shape) == (0, 36) and none.summary.tolist() == [0, 0, 4096, 0, 0, 4096, 1, 0]
    bare = query.isosurface_rows(sg, _g(V, dev, F), 0.0)                       # material=None: 18 zeros, on the bits
    assert bare.rows.shape[0] == 3164 and not bool((bare.rows[:, 18:].view(torch.int32) != 0).any())


def test_untouched_state(hip, bunny_small, dev):
    from ezrt_amd import scene as S
    from ezrt_amd import scenes, trace
    scn = bunny_small.upload(hip)
    V, g = IS.sphere()
    values = _g(V, dev, F)                                                     # (the inputs first: nothing but the call between the two reads)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(64, 64, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=1, tile=(16, 16))
    frame = torch.zeros((64, 64, 4), dtype=torch.float32, device=dev)
    scn.render_device(prm, frame.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    before = (scn.counters(), scn.last_render_ms())
    assert before[0]["rays"] > 0
    got = query.isosurface_rows(scn, values, 0.0)
    torch.cuda.synchronize()
    assert got.rows.shape[0] == 3164 and (scn.counters(), scn.last_render_ms()) == before


def test_errors(hip, sg, oracle, bunny_small, dev):
    lib = hip.lib
    V, grid = IS.sphere()
    I = _want("sphere", V, grid)
    nx, ny, nz = _dims(V)
    T, nb = int(I.offsets[-1]), I.offsets.size - 1
    wb = lib.ezrt_iso_work_bytes(nx, ny, nz)
    full = lambda k, dt: torch.full((k,), 5, dtype=dt, device=dev)
    bufs = dict(values=_g(V.reshape(-1), dev, F), grid8=_g(grid, dev, F), offsets=full(nb + 1, torch.int64), summary=full(8, torch.int64),
                work=torch.zeros(wb // 8 + 1, dtype=torch.int64, device=dev))
    host = np.zeros(max(36 * T, V.size, 64), np.int64)
    hp = P(host.ctypes.data)
    torch.cuda.synchronize()
    f = lib.ezrt_iso_count_device
    dp = lambda x: P(x.data_ptr())

    def fa(**kw):
        g = lambda k: kw[k] if k in kw else dp(bufs[k])
        return [kw.get("s", sg._h), g("values"), kw.get("nx", nx), kw.get("ny", ny), kw.get("nz", nz), g("grid8"), g("offsets"), g("summary"), g("work"),
                kw.get("work_bytes", wb), None]
    assert f(*fa(work_bytes=wb - 1)) == EZRT_ERR_INVALID and b"work_bytes" in lib.ezrt_last_error()
    assert f(*fa(work_bytes=0)) == EZRT_ERR_INVALID
    assert f(*fa(work=P(bufs["work"].data_ptr() + 4))) == EZRT_ERR_INVALID and b"aligned" in lib.ezrt_last_error()
    for k in ["s"] + list(bufs):
        assert f(*fa(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in bufs:                                                             # host memory is rejected, never read or written
        assert f(*fa(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    for k in ("nx", "ny", "nz"):
        assert f(*fa(**{k: 0})) == EZRT_ERR_INVALID and b"dimension" in lib.ezrt_last_error() and f(*fa(**{k: -5})) == EZRT_ERR_INVALID
        assert f(*fa(**{k: 2 ** 31 - 1, "work_bytes": 2 ** 44})) == EZRT_ERR_INVALID and b"INT32_MAX" in lib.ezrt_last_error()
    assert f(*fa(nz=1)) == 0                                                   # no cells: launches nothing
    torch.cuda.synchronize()
    for k in ("offsets", "summary"):
        assert bool((bufs[k] == 5).all()), k
    assert not host.any()
    # the fill
    g = lib.ezrt_iso_rows_device
    fb = dict(values=bufs["values"], grid8=bufs["grid8"], material18=_g(IS.MATERIAL, dev, F), offsets=_g(I.offsets, dev, np.int64),
              out=torch.full((T, 36), 5.0, dtype=torch.float32, device=dev), cell=full(T, torch.int32))

    def ga(**kw):
        h = lambda k: kw[k] if k in kw else dp(fb[k])
        return [kw.get("s", sg._h), h("values"), kw.get("nx", nx), kw.get("ny", ny), kw.get("nz", nz), h("grid8"), h("material18"), h("offsets"),
                kw.get("capacity", T), h("out"), h("cell"), None]
    for k in ("s", "values", "grid8", "material18", "offsets", "out"):
        assert g(*ga(**{k: None})) == EZRT_ERR_INVALID and b"NULL" in lib.ezrt_last_error(), k
    for k in fb:
        assert g(*ga(**{k: hp})) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error(), k
    assert g(*ga(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(capacity=2 ** 62)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
    assert g(*ga(nx=0)) == EZRT_ERR_INVALID and g(*ga(ny=2 ** 31 - 1)) == EZRT_ERR_INVALID
    # out overlapping values: the same bytes, rows that begin inside values, rows that end inside it
    nv = V.size
    both = torch.full((36 * T + nv + 36 * T,), 5.0, dtype=torch.float32, device=dev)
    both[36 * T:36 * T + nv] = bufs["values"]
    torch.cuda.synchronize()
    at = lambda fl: P(both.data_ptr() + 4 * fl)
    for out_at, cap in ((36 * T, T), (36 * T + nv - 1, 1), (36 * T - 35, 1), (1, T), (36 * T + 4, 1)):
        assert g(*ga(values=at(36 * T), out=at(out_at), capacity=cap)) == EZRT_ERR_INVALID and b"overlaps" in lib.ezrt_last_error(), (out_at, cap)
    assert g(*ga(values=at(36 * T), out=at(36 * T + nv), capacity=T, cell=None)) == 0    # behind it: no overlap (and 4 bytes off 16: per lane)
    assert g(*ga(values=at(36 * T), out=at(0), capacity=T, cell=None)) == 0             # before it
    assert g(*ga(nz=1)) == 0 and g(*ga(capacity=0, out=None)) == 0
    torch.cuda.synchronize()
    assert bool((fb["out"] == 5.0).all()) and bool((fb["cell"] == 5).all()) and not host.any()
    assert IE.same_rows(both[36 * T + nv:].cpu().numpy().reshape(-1, 36), I.out) and IE.same_rows(both[:36 * T].cpu().numpy().reshape(-1, 36), I.out)
    # the rejected calls left no HIP error behind: the next call works
    _same_count(_count(lib, sg, V, grid, dev), I, "after the rejected calls")
    assert g(*ga(cell=None)) == 0
    torch.cuda.synchronize()
    assert IE.same_rows(fb["out"].cpu().numpy(), I.out) and bool((fb["cell"] == 5).all())
    # the wrapper
    values = _g(V, dev, F)
    with pytest.raises(TypeError):
        query.isosurface_rows(bunny_small.upload(oracle), values, 0.0)
    with pytest.raises(TypeError):
        query.isosurface_rows(sg, values.cpu(), 0.0)
    with pytest.raises(TypeError):
        query.isosurface_rows(sg, values.to(torch.float64), 0.0)
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values.reshape(-1), 0.0)
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values.transpose(0, 2), 0.0)
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values, 0.0, origin=(0, 0))
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values, 0.0, spacing=(1, 2))
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values, 0.0, material=[0.0] * 17)
    with pytest.raises(ValueError):
        query.isosurface_rows(sg, values, 0.0, cell=1)

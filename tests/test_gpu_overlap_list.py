"""Overlap lists on device tensors (include/ezrt_overlap_list.h, ezrt_amd/query.py: box_overlap_list, obb_overlap_list,
tri_overlap_list, self_overlap_list, capsule_overlap_list): every triangle a query touches, in CSR form.

Every answer is a set of integers and is compared exactly.  The expected rows come from the numpy restatements the max_k tests use
(overlaps() of tests/box_overlap_expected.py, obb_overlap_expected.py and tri_overlap_expected.py, within() of segment_expected.py,
crosses() of self_overlap_expected.py): the boolean query x triangle matrix, a row is np.nonzero of its line.

* on the bits: offsets, ids and n_found of the five queries on the voxel solid, the Bunny scene, adversarial geometry and a scene that
  does not prune (the sweep route) -- four of them through test_lists_on_the_bits, the self-overlap through
  test_self_lists_on_the_bits --, with the query sets of the max_k tests -- all ~2 000 boxes and triangles, every second oriented box
  (~1 030) and every fifth capsule (~400: their restatements are the slow ones) -- and the first 64 of every row against the max_k = 64
  call on the device;
* row lengths at every seam of ezrt_overlap_list_limits on the constructed line of tests/overlap_list_scenes.py, in one batch and in
  a shuffled one, under every kind of tree; every tree shape of tests/tree_shapes.py;
* batches of 1 .. 129 queries and a [2, 3, 4] shape; capacities over poisoned rows; hand-made offsets between guard words;
* the self-overlap lists on the same scenes and on the defect scene, with ids = None and an id subset, and their symmetry; walk against
  sweep; a refit (also BETWEEN count and fill); stream order; a render call
  beside the query and untouched counters; the error contract."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from ezrt_amd import _abi, query, refit
from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allhits_scenes as A  # noqa: E402
import box_overlap_expected as BE  # noqa: E402
import box_overlap_scenes as BS  # noqa: E402
import inside_scenes as IS  # noqa: E402
import obb_overlap_expected as OE  # noqa: E402
import obb_overlap_scenes as OS  # noqa: E402
import overlap_list_scenes as LS  # noqa: E402
import segment_expected as SX  # noqa: E402
import segment_scenes as SS  # noqa: E402
import self_overlap_expected as SE  # noqa: E402
import self_overlap_scenes as SO  # noqa: E402
import tree_shapes as T  # noqa: E402
import tri_overlap_expected as TE  # noqa: E402
import tri_overlap_scenes as TS  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
SCENES = ("voxel_solid", "bunny", "nasty", "not_nested")
P = C.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def limits():
    insert_max, tile_max = _abi.overlap_list_limits()
    assert 0 <= insert_max <= 64 < tile_max
    return insert_max, tile_max


def _gpu(x, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


# kind -> (the queries of the max_k tests as a tuple of arrays, thinned; the restatement's matrix; the list call; the max_k = 64 call)
KINDS = {
    "box": (lambda tri, nodes, seed: BS.boxes_for(tri, nodes, 700 + seed), 1, lambda q, tri: BE.overlaps(q[0], q[1], tri),
            query.box_overlap_list, query.box_overlap),
    "obb": (lambda tri, nodes, seed: OS.boxes_for(tri, nodes, 2200 + seed)[:2], 2, lambda q, tri: OE.overlaps(q[0], q[1], tri),
            query.obb_overlap_list, query.obb_overlap),
    "tri": (lambda tri, nodes, seed: (TS.tris_for(tri, nodes, 900 + seed),), 1, lambda q, tri: TE.overlaps(q[0], tri),
            query.tri_overlap_list, query.tri_overlap),
    "capsule": (lambda tri, nodes, seed: SS.queries_for(tri, 2100 + seed)[::2], 5, lambda q, tri: SX.within(q[0], q[1], tri),
                query.capsule_overlap_list, query.capsule_overlap),
}
_cache = {}


def _scene(name, hip, bunny_small):
    """(tri, nodes, the device scene); not_nested is the Bunny scene's triangles under nodes that do not prune"""
    if ("scene", name) not in _cache:
        if name == "voxel_solid":
            v = IS.voxel_solid()
            tri, nodes = v["tri"], v["nodes"]
        else:
            tri, nodes, _ = A.scene(name, bunny_small)
        _cache[("scene", name)] = (tri, nodes, hip.scene_create(tri, nodes))
    return _cache[("scene", name)]


def _case(kind, name, hip, bunny_small):
    """(queries, the restatement's matrix, the device scene), computed once and shared; not_nested shares the Bunny scene's queries
    and matrix: the triangles are the same"""
    tri, nodes, sg = _scene(name, hip, bunny_small)
    base = "bunny" if name == "not_nested" else name
    if (kind, base) not in _cache:
        make, stride, over = KINDS[kind][:3]
        btri, bnodes, _ = _scene(base, hip, bunny_small)
        q = tuple(np.ascontiguousarray(x[::stride]) for x in make(btri, bnodes, SCENES.index(base)))
        _cache[(kind, base)] = (q, np.asarray(over(q, btri), bool))
    q, over = _cache[(kind, base)]
    return q, over, sg


def _lists(fn, sg, q, dev, check=True, **kw):
    """(offsets, ids, n_found) as numpy, after the checks of the shapes and types"""
    r = fn(sg, *(_gpu(x, dev) for x in q), check=check, **kw)
    torch.cuda.synchronize()
    n = int(np.prod(q[0].shape[:-1]))
    assert isinstance(r, query.OverlapList) and r.offsets.dtype == torch.int64 and r.tri.dtype == torch.int32
    assert tuple(r.offsets.shape) == (n + 1,) and r.tri.dim() == 1
    if not check:
        assert r.n_found is None
        return r.offsets.cpu().numpy(), r.tri.cpu().numpy(), None
    assert r.n_found.dtype == torch.int32 and tuple(r.n_found.shape) == (n,)
    return r.offsets.cpu().numpy(), r.tri.cpu().numpy(), r.n_found.cpu().numpy()


def _same(got, over, what=""):
    offsets, ids = LS.rows_of(over)
    assert np.array_equal(got[0], offsets), "%s: offsets differ, first at query %d" % (what, int(np.argmax(got[0] != offsets)))
    assert got[1].shape == ids.shape and np.array_equal(got[1], ids), "%s: ids differ" % what
    if got[2] is not None:
        assert np.array_equal(got[2], np.diff(offsets)), "%s: n_found differs" % what


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lists_on_the_bits(hip, bunny_small, dev, limits, kind, name):
    q, over, sg = _case(kind, name, hip, bunny_small)
    assert (sg.prune_info()["mode"] == -1) == (name == "not_nested")   # the sweep route runs on the scene that does not prune
    got = _lists(KINDS[kind][3], sg, q, dev)
    _same(got, over, "%s %s" % (kind, name))
    # the first 64 of every row are the max_k = 64 call's row on the device, the length its count
    r = KINDS[kind][4](sg, *(_gpu(x, dev) for x in q), 64, count=True)
    torch.cuda.synchronize()
    rows64, count = r.tri.cpu().numpy(), r.n_overlap.cpu().numpy()
    assert np.array_equal(count, np.diff(got[0]))
    for i in range(count.shape[0]):
        k = min(64, int(count[i]))
        assert np.array_equal(rows64[i, :k], got[1][got[0][i]:got[0][i] + k]) and (rows64[i, k:] == -1).all(), i
    # the comparison is not of nothing
    n_q = count.shape[0]
    assert n_q >= (1900 if kind in ("box", "tri") else 1000 if kind == "obb" else 380)
    assert (count == 0).any() and (count > 0).sum() > n_q // 3 and count.max() > 64
    if kind == "box" and name in ("bunny", "not_nested"):
        assert count.max() == over.shape[1] > limits[1]                # the box that holds the scene: a row past tile_max


@pytest.mark.parametrize("kind", LS.KINDS)
def test_row_lengths_at_every_seam(hip, dev, limits, kind):
    insert_max, tile_max = limits
    M = tile_max + 300
    tri, nodes = LS.line_scene(kind, M)
    sg = hip.scene_create(tri, nodes)
    assert (sg.prune_info()["mode"] == -1) == (kind == "leaf_misses")
    if kind == "uncovered":
        assert T.check_valid(tri, nodes)["uncovered"].size == LS.N_APPENDED + 2   # reached only by the sweep behind the walk
    lengths = LS.seam_lengths(insert_max, tile_max, M)
    assert {0, 1, 64, 65, insert_max, insert_max + 1, tile_max, tile_max + 1, M} <= set(lengths)
    pos = LS.position(tri)
    rng = np.random.default_rng(5)
    for order in (np.arange(len(lengths)), rng.permutation(len(lengths)), rng.permutation(np.repeat(np.arange(len(lengths)), 2))):
        L = np.asarray(lengths)[order]
        q = LS.boxes(L)
        over = BE.overlaps(q[0], q[1], tri)
        assert np.array_equal(over, pos[None, :] < L[:, None]) and np.array_equal(over.sum(1), L)   # rows of exactly L
        _same(_lists(query.box_overlap_list, sg, q, dev), over, "%s %r" % (kind, L))
    ids = _lists(query.box_overlap_list, sg, LS.boxes([M]), dev)[1]
    assert np.array_equal(ids, np.arange(M))
    if kind == "runs5_shuffled":                                       # (the builders sort the array along x; these nodes do not)
        assert not np.array_equal(np.argsort(pos, kind="stable"), np.arange(M))   # ids are not in the order of the positions


@pytest.mark.parametrize("name", T.HOST_SHAPES + T.LBVH_SHAPES)
def test_every_tree_shape(hip, dev, name):
    tri, nodes, expect = T.shape(name)
    Q = T.shape_queries(name)
    sg = hip.scene_create(tri, nodes)
    lo, hi = np.concatenate([Q["lo"], T.vertices(tri).reshape(-1, 3).min(0)[None]]), np.concatenate([Q["hi"], T.vertices(tri).reshape(-1, 3).max(0)[None]])
    over = BE.overlaps(lo, hi, tri)
    _same(_lists(query.box_overlap_list, sg, (lo, hi), dev), over, name)
    assert over[-1].all() and (tri.shape[0] <= 8 or over.sum(1).max() > 64)
    _same(_lists(query.tri_overlap_list, sg, (Q["tris"],), dev), TE.overlaps(Q["tris"], tri), name)
    cross = SE.crosses(tri)
    _same(_self(sg, None, dev), cross, name)


def _self(sg, ids, dev, **kw):
    r = query.self_overlap_list(sg, None if ids is None else _gpu(ids, dev, np.int32), check=True, **kw)
    torch.cuda.synchronize()
    return r.offsets.cpu().numpy(), r.tri.cpu().numpy(), r.n_found.cpu().numpy()


def test_batch_sizes_and_shapes(hip, bunny_small, dev):
    q, over, sg = _case("box", "nasty", hip, bunny_small)
    for n in (1, 63, 64, 65, 129):
        sel = np.arange(n) * 7 % over.shape[0]
        _same(_lists(query.box_overlap_list, sg, (q[0][sel], q[1][sel]), dev), over[sel], "n=%d" % n)
    sel = np.arange(24) * 11 % over.shape[0]
    lead = (q[0][sel].reshape(2, 3, 4, 3), q[1][sel].reshape(2, 3, 4, 3))
    r = query.box_overlap_list(sg, _gpu(lead[0], dev), _gpu(lead[1], dev), check=True)
    torch.cuda.synchronize()
    assert tuple(r.offsets.shape) == (25,) and tuple(r.n_found.shape) == (24,)
    _same((r.offsets.cpu().numpy(), r.tri.cpu().numpy(), r.n_found.cpu().numpy()), over[sel], "[2, 3, 4]")
    c, u = _case("obb", "nasty", hip, bunny_small)[0]
    ro = query.obb_overlap_list(sg, _gpu(c[:24].reshape(2, 3, 4, 3), dev), _gpu(u[:24].reshape(2, 3, 4, 3, 3), dev))
    torch.cuda.synchronize()
    _same((ro.offsets.cpu().numpy(), ro.tri.cpu().numpy(), None), _case("obb", "nasty", hip, bunny_small)[1][:24], "obb [2, 3, 4]")
    e = query.box_overlap_list(sg, torch.empty((0, 3), device=dev), torch.empty((0, 3), device=dev), check=True)
    assert tuple(e.offsets.shape) == (1,) and int(e.offsets[0]) == 0 and tuple(e.tri.shape) == (0,) and tuple(e.n_found.shape) == (0,)
    e = query.tri_overlap_list(sg, torch.empty((0, 9), device=dev), capacity=7)
    assert tuple(e.tri.shape) == (7,) and bool((e.tri == -1).all()) and e.n_found is None


def _raw_box(lib, sg, lo_t, hi_t, offsets_t, cap, tri_ptr, nf_t):
    assert lib.ezrt_query_box_overlap_list_device(sg._h, P(lo_t.data_ptr()), P(hi_t.data_ptr()), lo_t.shape[0], P(offsets_t.data_ptr()), cap,
                                                  tri_ptr, P(nf_t.data_ptr()) if nf_t is not None else None, None) == 0
    torch.cuda.synchronize()


def test_capacity(hip, bunny_small, dev):
    """a row is written whole or not at all; the rows that end past the capacity stay poisoned, every other row is complete"""
    q, over, sg = _case("box", "nasty", hip, bunny_small)
    lib = hip.lib
    sel = np.append(np.arange(299) * 5 % over.shape[0], int(np.argmax(over.sum(1))))   # the longest row last: total - 1 cuts it off
    over = over[sel]
    lo_t, hi_t = _gpu(q[0][sel], dev), _gpu(q[1][sel], dev)
    n = 300
    nov = torch.full((n,), -7, dtype=torch.int32, device=dev)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    assert lib.ezrt_query_box_overlap_device(sg._h, P(lo_t.data_ptr()), P(hi_t.data_ptr()), n, 0, None, P(nov.data_ptr()), None) == 0
    assert lib.ezrt_overlap_offsets_device(sg._h, P(nov.data_ptr()), n, P(off.data_ptr()), None) == 0
    torch.cuda.synchronize()
    offsets, ids = LS.rows_of(over)
    assert np.array_equal(off.cpu().numpy(), offsets) and np.array_equal(nov.cpu().numpy(), np.diff(offsets))
    total = int(offsets[-1])
    assert total > 300 and np.diff(offsets)[-1] > 64
    for cap in (0, total - 1, total // 2, total, total + 5):
        buf = torch.full((max(cap, total) + 8,), -9, dtype=torch.int32, device=dev)
        nf = torch.full((n,), -7, dtype=torch.int32, device=dev)
        _raw_box(lib, sg, lo_t, hi_t, off, cap, P(buf.data_ptr()), nf)
        got = buf.cpu().numpy()
        want = np.full(got.shape, -9, np.int32)
        fits = offsets[1:] <= cap
        for i in np.nonzero(fits)[0]:
            want[offsets[i]:offsets[i + 1]] = ids[offsets[i]:offsets[i + 1]]
        assert np.array_equal(got, want), cap
        assert np.array_equal(nf.cpu().numpy(), np.diff(offsets)), cap   # n_found is the truth for skipped rows too
        assert fits.all() == (cap >= total) and (cap == 0 or fits.any())
    # the wrapper: a given capacity returns that many entries, the unwritten ones -1, and never more
    for cap in (0, total - 1, total + 5):
        o, t, f = _lists(query.box_overlap_list, sg, (q[0][sel], q[1][sel]), dev, capacity=cap)
        want = np.full(cap, -1, np.int32)
        for i in np.nonzero(offsets[1:] <= cap)[0]:
            want[offsets[i]:offsets[i + 1]] = ids[offsets[i]:offsets[i + 1]]
        assert np.array_equal(o, offsets) and np.array_equal(t, want) and np.array_equal(f, np.diff(offsets))


@pytest.mark.parametrize("kind", ("sah8", "leaf_misses"))
def test_bad_offsets_write_nothing_outside_valid_rows(hip, dev, limits, kind):
    """hand-made offsets: a negative start, a row shorter and a row longer than the truth, a negative length, a row past the capacity.
    Only rows that are valid and fit may be written, between guard words; n_found reports the truth"""
    insert_max, tile_max = limits
    M = tile_max + 300
    tri, nodes = LS.line_scene(kind, M)
    sg = hip.scene_create(tri, nodes)
    true = [5, 70, 20, 300, 2 * insert_max + 9, 3, 40]
    q = LS.boxes(true)
    over = BE.overlaps(q[0], q[1], tri)
    lo_t, hi_t = _gpu(q[0], dev), _gpu(q[1], dev)
    e = 395 + 2 * insert_max + 4                                        # row 4 ends here: 5 shorter than the truth
    cap, G = e + 30, 64
    hand = np.array([-3, 5, 75, 90, 395, e, e - 2, cap + 7], np.int64)
    #  row 0 (-3, 5)     a negative start: no row
    #  row 1 (5, 75)     the truth (70): complete
    #  row 2 (75, 90)    shorter than the truth (20): contents unspecified, inside the row
    #  row 3 (90, 395)   longer than the truth (300): contents unspecified, inside the row
    #  row 4 (395, e)    shorter than the truth, longer than insert_max: appended, and sorted on the walk
    #  row 5 (e, e - 2)  a negative length: no row
    #  row 6 (e - 2, cap + 7)  past the capacity: skipped whole
    buf = torch.full((G + cap + G,), -9, dtype=torch.int32, device=dev)
    nf = torch.full((len(true),), -7, dtype=torch.int32, device=dev)
    _raw_box(hip.lib, sg, lo_t, hi_t, _gpu(hand, dev, np.int64), cap, P(buf.data_ptr() + 4 * G), nf)
    got = buf.cpu().numpy()
    assert np.array_equal(nf.cpu().numpy(), true)
    assert (got[:G + 5] == -9).all() and (got[G + e:] == -9).all()      # the guards, [0, 5) and everything from e on
    ids1 = np.nonzero(over[1])[0]
    assert np.array_equal(got[G + 5:G + 75], ids1)                      # the one row whose length is the truth
    for a, b, i in ((75, 90, 2), (395, e, 4)):                          # short rows hold ids of their own query and nothing else
        assert np.isin(got[G + a:G + b], np.nonzero(over[i])[0]).all(), i
    assert np.isin(got[G + 90:G + 395], np.concatenate([np.nonzero(over[3])[0], [-9]])).all()
    # the same rows past the capacity: nothing at all is written
    buf.fill_(-9)
    _raw_box(hip.lib, sg, lo_t, hi_t, _gpu(hand + 10 ** 12, dev, np.int64), cap, P(buf.data_ptr() + 4 * G), nf)
    assert bool((buf == -9).all()) and np.array_equal(nf.cpu().numpy(), true)
    buf.fill_(-9)
    _raw_box(hip.lib, sg, lo_t, hi_t, _gpu(np.array([1, 2 ** 62, -2 ** 62, 2 ** 63 - 1, -2 ** 63, -1, -5, -4], np.int64), dev, np.int64), cap,
             P(buf.data_ptr() + 4 * G), nf)
    assert bool((buf == -9).all()) and np.array_equal(nf.cpu().numpy(), true)


def test_walk_equals_sweep(hip, bunny_small, dev):
    for kind in sorted(KINDS):
        q, over, sg = _case(kind, "bunny", hip, bunny_small)
        swept = _case(kind, "not_nested", hip, bunny_small)[2]
        assert sg.prune_info()["mode"] != -1 and swept.prune_info()["mode"] == -1
        sel = slice(0, 300)
        a = _lists(KINDS[kind][3], sg, tuple(x[sel] for x in q), dev)
        b = _lists(KINDS[kind][3], swept, tuple(x[sel] for x in q), dev)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), kind
        assert a[0][-1] > 300


SELF_SCENES = SCENES + ("defects", "defects_swept")


def _self_case(name, hip, bunny_small):
    """(tri, crosses() of ALL its triangles, the device scene), computed once and shared; the two defect scenes (walk and sweep)
    share one matrix, as do the Bunny scene and not_nested"""
    if name.startswith("defects"):
        d = SO.defect_scene()
        if ("scene", name) not in _cache:
            arrays = (d["tri"], d["nodes"]) if name == "defects" else A.not_nested(types.SimpleNamespace(**d))
            _cache[("scene", name)] = (arrays[0], arrays[1], hip.scene_create(*arrays))
        base = "defects"
    else:
        base = "bunny" if name == "not_nested" else name
    tri, nodes, sg = _scene(name, hip, bunny_small)
    if ("self", base) not in _cache:
        _cache[("self", base)] = SE.crosses(tri)
    return tri, _cache[("self", base)], sg


@pytest.mark.parametrize("name", SELF_SCENES)
def test_self_lists_on_the_bits(hip, bunny_small, dev, name):
    """the fifth query, as test_lists_on_the_bits: every triangle of the scene as a query (ids = None: 288, 5 300, 2 812 and 585 rows,
    the restatement over all pairs) and an id subset with ids outside the scene, against crosses() and the max_k = 64 call"""
    tri, cross, sg = _self_case(name, hip, bunny_small)
    m = tri.shape[0]
    assert (sg.prune_info()["mode"] == -1) == (name in ("not_nested", "defects_swept"))
    busiest = int(np.argmax(cross.sum(1)))
    sub = np.array([5, -1, m, 2 ** 31 - 1, 5, busiest, 0, m - 1, -2 ** 31] + list(range(0, m, 3)), np.int32)
    live = (sub >= 0) & (sub < m)
    for ids, want in ((None, cross), (sub, np.where(live[:, None], cross[np.clip(sub, 0, m - 1)], False))):
        got = _self(sg, ids, dev)
        _same(got, want, "self %s %s" % (name, "all" if ids is None else "subset"))
        r = query.self_overlap(sg, None if ids is None else _gpu(ids, dev, np.int32), 64, count=True)
        torch.cuda.synchronize()
        rows64, count = r.tri.cpu().numpy(), r.n_overlap.cpu().numpy()
        assert np.array_equal(count, np.diff(got[0]))
        for i in np.nonzero(count)[0]:
            k = min(64, int(count[i]))
            assert np.array_equal(rows64[i, :k], got[1][got[0][i]:got[0][i] + k]), i
        assert (rows64[count == 0] == -1).all()
    assert cross[np.clip(sub, 0, m - 1)][live].any() == cross.any()   # the subset meets the crossings where there are any
    # the comparison is not of nothing where the mesh crosses itself; the clean meshes have empty rows by the restatement
    rows = cross.sum(1)
    if name.startswith("defects"):
        assert rows.max() > 64 and (rows == 0).any() and cross.sum() > 1000
    elif name == "nasty":
        assert rows.max() >= 2 and cross.sum() > 0
    else:
        assert not cross.any()


def test_self_overlap_lists_are_symmetric(hip, bunny_small, dev):
    d = SO.defect_scene()
    tri, nodes = d["tri"], d["nodes"]
    cross = SE.crosses(tri)
    m = tri.shape[0]
    for sg in (hip.scene_create(tri, nodes), hip.scene_create(*A.not_nested(types.SimpleNamespace(**d)))):
        got = _self(sg, None, dev)
        _same(got, cross, "defects")
        o, t, _ = got
        pairs = set(zip(np.repeat(np.arange(m), np.diff(o)).tolist(), t.tolist()))
        assert len(pairs) == t.size and all((b, a) in pairs for a, b in pairs) and all(a != b for a, b in pairs)
        assert np.diff(o).max() > 64 and (np.diff(o) == 0).any() and t.size == cross.sum() > 1000
        ids = np.array([5, -1, m, 2 ** 31 - 1, 5, int(np.argmax(cross.sum(1))), 0, m - 1] + list(range(0, m, 3)), np.int32)
        live = (ids >= 0) & (ids < m)
        want = np.where(live[:, None], cross[np.clip(ids, 0, m - 1)], False)
        _same(_self(sg, ids, dev), want, "ids")
        assert not want[[1, 2, 3]].any() and want[5].sum() > 64
    # clean meshes have empty rows everywhere (also the sweep)
    for name in ("voxel_solid", "not_nested"):
        tri, nodes, sg = _scene(name, hip, bunny_small)
        o, t, f = _self(sg, None, dev)
        assert not o.any() and t.size == 0 and not f.any() and o.shape == (tri.shape[0] + 1,)
    tri, nodes, sg = _scene("nasty", hip, bunny_small)
    _same(_self(sg, None, dev), SE.crosses(tri), "nasty")


def test_after_a_refit_and_between_the_passes(hip, dev):
    v = IS.voxel_solid()
    tri, nodes = v["tri"], v["nodes"]
    lo, hi = (x[:400] for x in BS.boxes_for(tri, nodes, 77))
    moved = tri.copy()
    for k in range(3):
        moved[:, 3 * k:3 * k + 3] = moved[:, 3 * k:3 * k + 3] * np.float32(2) + np.float32([3, -5, 11])
    mlo, mhi = lo * np.float32(2) + np.float32([3, -5, 11]), hi * np.float32(2) + np.float32([3, -5, 11])
    sg = hip.scene_create(tri, nodes)
    lib = hip.lib
    before, after = BE.overlaps(mlo, mhi, tri), BE.overlaps(mlo, mhi, moved)
    _same(_lists(query.box_overlap_list, sg, (mlo, mhi), dev), before, "before the refit")
    # count and offsets on the old geometry, the fill on the new: n_found tells, and a row whose n_found is its length is right
    lo_t, hi_t = _gpu(mlo, dev), _gpu(mhi, dev)
    n = 400
    nov, off = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    assert lib.ezrt_query_box_overlap_device(sg._h, P(lo_t.data_ptr()), P(hi_t.data_ptr()), n, 0, None, P(nov.data_ptr()), None) == 0
    assert lib.ezrt_overlap_offsets_device(sg._h, P(nov.data_ptr()), n, P(off.data_ptr()), None) == 0
    refit.refit(sg, moved)
    old = off.cpu().numpy()
    buf = torch.full((int(old[-1]) + 8,), -9, dtype=torch.int32, device=dev)
    nf = torch.full((n,), -7, dtype=torch.int32, device=dev)
    _raw_box(lib, sg, lo_t, hi_t, off, int(old[-1]), P(buf.data_ptr()), nf)
    found, got = nf.cpu().numpy(), buf.cpu().numpy()
    assert np.array_equal(found, after.sum(1)) and (found != np.diff(old)).sum() > 100 and (got[int(old[-1]):] == -9).all()
    for i in np.nonzero((found == np.diff(old)) & (found > 0))[0]:
        assert np.array_equal(got[old[i]:old[i + 1]], np.nonzero(after[i])[0]), i
    _same(_lists(query.box_overlap_list, sg, (mlo, mhi), dev), after, "after the refit")
    assert after.sum() > 1000 and not np.array_equal(before, after)


def test_stream_order(hip, bunny_small, dev):
    q, over, sg = _case("box", "nasty", hip, bunny_small)
    src = tuple(_gpu(x[:500], dev) for x in q)
    late = tuple(torch.zeros_like(x) for x in src)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        for a, b in zip(late, src):
            a.copy_(b)                                                 # the boxes are written on `side`, behind the sleep
    total = int(over[:500].sum())
    a = query.box_overlap_list(sg, *late, capacity=total, check=True, stream=side)   # issued from the default stream's context
    b = query.box_overlap_list(sg, *late, stream=side.cuda_stream)     # a raw handle; synchronises `side` itself for the total
    side.synchronize()
    _same((a.offsets.cpu().numpy(), a.tri.cpu().numpy(), a.n_found.cpu().numpy()), over[:500], "on a side stream")
    _same((b.offsets.cpu().numpy(), b.tri.cpu().numpy(), None), over[:500], "on a raw stream handle")


def test_beside_a_render_call_and_untouched_state(hip, bunny_small, dev):
    q, over, _ = _case("box", "bunny", hip, bunny_small)
    sg = bunny_small.upload(hip)
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    prm = trace.make_params(128, 128, eye, cam, cfg["integrator"], cfg["max_bounce"], spp=2, tile=(16, 16))
    qt = tuple(_gpu(x, dev) for x in q)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    sg.render_device(prm, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    assert before[0]["rays"] > 0
    query.box_overlap_list(sg, *qt, check=True)
    query.self_overlap_list(sg, capacity=10)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before
    frame = torch.zeros((128, 128, 4), dtype=torch.float32, device=dev)
    a.wait_stream(torch.cuda.current_stream(dev))
    b.wait_stream(torch.cuda.current_stream(dev))
    sg.render_device(prm, frame.data_ptr(), a.cuda_stream)
    got = query.box_overlap_list(sg, *qt, capacity=int(over.sum()), check=True, stream=b)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), alone.cpu().numpy().view(np.uint32))
    _same(tuple(x.cpu().numpy() for x in got), over, "beside a render call")


def test_errors(hip, oracle, bunny_small, dev):
    tri, nodes, sg = _scene("voxel_solid", hip, bunny_small)
    lib = hip.lib
    n = 10
    lo, hi = (x[:n] for x in BS.boxes_for(tri, nodes, 3))
    offsets, ids = LS.rows_of(BE.overlaps(lo, hi, tri))
    total = int(offsets[-1])
    d = lambda t: P(t.data_ptr())  # noqa: E731
    hp = lambda a: P(a.ctypes.data)  # noqa: E731
    lo_t, hi_t, off = _gpu(lo, dev), _gpu(hi, dev), _gpu(offsets, dev, np.int64)
    c_t, u_t = _gpu(np.zeros((n, 3)), dev), _gpu(np.tile(np.eye(3), (n, 1, 1)), dev)
    t9, s6, rad = _gpu(np.zeros((n, 9)), dev), _gpu(np.zeros((n, 6)), dev), _gpu(np.zeros(n), dev)
    idt = torch.arange(n, dtype=torch.int32, device=dev)
    nov = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros(total + 8, dtype=torch.int32, device=dev)
    nf = torch.zeros(n, dtype=torch.int32, device=dev)
    host_f, host_i32, host_i64 = np.zeros(n * 9, np.float32), np.zeros(total + n, np.int32), np.zeros(n + 1, np.int64)
    tail = lambda **kw: [kw.get("n", n), kw.get("offsets", d(off)), kw.get("capacity", total), kw.get("tri", d(out)), kw.get("n_found", d(nf)), None]  # noqa: E731
    calls = {
        "box": (lib.ezrt_query_box_overlap_list_device, lambda **kw: [kw.get("s", sg._h), kw.get("in0", d(lo_t)), kw.get("in1", d(hi_t))] + tail(**kw), 2),
        "obb": (lib.ezrt_query_obb_overlap_list_device, lambda **kw: [kw.get("s", sg._h), kw.get("in0", d(c_t)), kw.get("in1", d(u_t))] + tail(**kw), 2),
        "tri": (lib.ezrt_query_tri_overlap_list_device, lambda **kw: [kw.get("s", sg._h), kw.get("in0", d(t9))] + tail(**kw), 1),
        "self": (lib.ezrt_query_self_overlap_list_device, lambda **kw: [kw.get("s", sg._h), kw.get("in0", d(idt))] + tail(**kw), 0),
        "capsule": (lib.ezrt_query_capsule_overlap_list_device, lambda **kw: [kw.get("s", sg._h), kw.get("in0", d(s6)), kw.get("in1", d(rad))] + tail(**kw), 2),
    }
    torch.cuda.synchronize()
    for key, (f, args, n_required) in calls.items():
        assert f(*args()) == 0 and f(*args(n_found=None)) == 0 and f(*args(capacity=0, tri=None)) == 0, key
        for k in ("s", "offsets", "tri") + ("in0", "in1")[:n_required]:
            assert f(*args(**{k: None})) == EZRT_ERR_INVALID, (key, k)
        assert f(*args(n=-1)) == EZRT_ERR_INVALID and f(*args(capacity=-1)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error()
        for big in (2 ** 62, 2 ** 62 + total, 2 ** 61, 2 ** 63 - 1):              # 4 * capacity would wrap, or pass PTRDIFF_MAX
            assert f(*args(capacity=big)) == EZRT_ERR_INVALID and b"capacity" in lib.ezrt_last_error(), (key, big)
        # host memory is rejected, never read or written
        assert f(*args(in0=hp(host_f))) == EZRT_ERR_INVALID and b"device memory" in lib.ezrt_last_error()
        assert f(*args(offsets=hp(host_i64))) == EZRT_ERR_INVALID and f(*args(tri=hp(host_i32))) == EZRT_ERR_INVALID
        assert f(*args(n_found=hp(host_i32))) == EZRT_ERR_INVALID
        out.fill_(5), nf.fill_(5)
        assert f(*args(n=0)) == 0
        torch.cuda.synchronize()
        assert bool((out == 5).all()) and bool((nf == 5).all())         # n == 0 launches nothing
    assert calls["self"][0](*calls["self"][1](in0=None)) == 0          # ids may be NULL: query i is triangle i ...
    assert calls["self"][0](*calls["self"][1](in0=None, n=tri.shape[0] + 1)) == EZRT_ERR_INVALID   # ... of the scene
    g = lib.ezrt_overlap_offsets_device
    assert g(sg._h, d(nov), n, d(off), None) == 0
    for bad in ((None, d(nov), n, d(off)), (sg._h, None, n, d(off)), (sg._h, d(nov), n, None), (sg._h, d(nov), -1, d(off)),
                (sg._h, hp(host_i32), n, d(off)), (sg._h, d(nov), n, hp(host_i64))):
        assert g(*bad, None) == EZRT_ERR_INVALID, bad
    off.fill_(5)
    assert g(sg._h, d(nov), 0, d(off), None) == 0
    torch.cuda.synchronize()
    assert bool((off == 5).all()) and not host_f.any() and not host_i32.any() and not host_i64.any()
    lib.ezrt_overlap_list_limits(None, None)                           # either pointer may be NULL
    # the rejected calls left no HIP error behind: the next call works
    _same(_lists(query.box_overlap_list, sg, (lo, hi), dev), BE.overlaps(lo, hi, tri), "after the rejected calls")
    # the wrappers
    for bad in (-1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="capacity"):
            query.box_overlap_list(sg, lo_t, hi_t, capacity=bad)
    with pytest.raises(TypeError):
        query.box_overlap_list(sg, torch.from_numpy(lo), torch.from_numpy(hi))
    with pytest.raises(TypeError):
        query.tri_overlap_list(bunny_small.upload(oracle), t9)
    with pytest.raises(ValueError):
        query.box_overlap_list(sg, lo_t, hi_t[:5])
    with pytest.raises(ValueError):
        query.capsule_overlap_list(sg, s6, rad[:5])
    with pytest.raises(TypeError):
        query.self_overlap_list(sg, idt.to(torch.int64))

"""tests/plane_loops_expected.py -- the numpy-and-dictionary restatement of include/ezrt_plane_loops.h (L1 .. L6) that the GPU test
compares with exactly -- held against the properties the header states, on tests/plane_scenes.py's inputs for the four CPU scenes and
on hand-made ones.  Needs no GPU and no library.

* order is a permutation of exactly the non-degenerate rows of the chained planes; consecutive rows of a loop match q1 to q0 on the
  bits; a closed loop's last q1 is its head's q0; an open one's ends are ends; heads ascend; the CSR arrays are consistent.
* The counts of every scene (printed): all loops of the closed voxel solid are closed, `open_solid` has open chains, `nasty` has keys
  of multiplicity above 1.
* A flipped copy reverses every loop; a permutation of the voxel solid's triangles keeps the set of cyclic point sequences; the
  section z = 1.5 of the voxel solid encloses +8.0 exactly.
* Two cubes touching along an edge, cut across it: a key with two IN and two OUT rows pairs by ascending row.
* L2: planes that are not chained (a capacity below the total, garbage offsets) have no loops and keep their rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inside_scenes as IS  # noqa: E402
import plane_expected as PE  # noqa: E402
import plane_loops_expected as LE  # noqa: E402
import plane_scenes as PS  # noqa: E402

F = np.float32
_cache = {}


def _case(name, bunny_small):
    """(tri, planes, (offsets, ids, seg, crossed), loops), computed once and shared"""
    if name not in _cache:
        tri, nodes, planes, kind = PS.inputs(name, bunny_small)
        sec = PE.section(planes, tri)
        _cache[name] = (tri, planes, sec, LE.loops(sec[0], sec[2], tri.shape[0]))
    return _cache[name]


def _check_structure(offsets, seg, lp, n_tri, capacity=None):
    """the properties that hold for every section"""
    b = LE.bits(seg)
    cap = b.shape[0] if capacity is None else capacity
    ok = LE.chained(offsets, cap, n_tri)
    deg = LE.degenerate(seg)
    want = np.concatenate([np.arange(offsets[i], offsets[i + 1]) for i in range(offsets.size - 1) if ok[i]] + [np.zeros(0, np.int64)])
    want = want[~deg[want]]
    assert np.array_equal(np.sort(lp.order), want)                            # a permutation of exactly these rows
    L = lp.closed.size
    assert lp.plane_loops[0] == 0 and lp.plane_loops[-1] == L and (np.diff(lp.plane_loops) >= 0).all()
    assert lp.loop_offsets[0] == 0 and lp.loop_offsets[-1] == want.size and (np.diff(lp.loop_offsets) >= 1).all()
    has_pred = np.zeros(cap, bool)
    has_pred[lp.next[lp.next >= 0]] = True
    assert (np.bincount(lp.next[lp.next >= 0], minlength=cap) <= 1).all()      # at most one predecessor
    assert (lp.next[want] >= -1).all() and (lp.next[deg[:cap] & (lp.next != -9)] == -1).all()
    for i in range(offsets.size - 1):
        l0, l1 = int(lp.plane_loops[i]), int(lp.plane_loops[i + 1])
        if not ok[i]:
            assert l0 == l1
            continue
        heads = lp.order[lp.loop_offsets[l0:l1]]
        assert (np.diff(heads) > 0).all()                                      # heads ascend
        for l in range(l0, l1):
            rows = lp.order[lp.loop_offsets[l]:lp.loop_offsets[l + 1]]
            assert ((rows >= offsets[i]) & (rows < offsets[i + 1])).all()
            assert np.array_equal(b[rows[:-1], 1], b[rows[1:], 0])            # q1 -> the next q0, on the bits
            assert np.array_equal(lp.next[rows[:-1]], rows[1:])
            if lp.closed[l]:
                assert np.array_equal(b[rows[-1], 1], b[rows[0], 0]) and lp.next[rows[-1]] == rows[0] and rows[0] == rows.min()
            else:
                assert lp.next[rows[-1]] == -1 and not has_pred[rows[0]]


def _counts(offsets, seg, lp):
    single = int((np.diff(lp.loop_offsets) == 1).sum())
    return dict(rows=int(offsets[-1]), degenerate=int(LE.degenerate(seg)[:offsets[-1]].sum()), closed=int(lp.closed.sum()),
                open=int((lp.closed == 0).sum()), multi=LE.multiplicity(offsets, seg), single=single,
                longest=int(np.diff(lp.loop_offsets).max()), largest_plane=int(np.diff(offsets).max()))


@pytest.mark.parametrize("name", PS.CPU_NAMES)
def test_structure_and_counts(bunny_small, name):
    tri, planes, sec, lp = _case(name, bunny_small)
    _check_structure(sec[0], sec[2], lp, tri.shape[0])
    c = _counts(sec[0], sec[2], lp)
    print(name, c)
    if name == "voxel_solid":                                                  # closed, consistently wound, no key twice
        assert (c["rows"], c["degenerate"], c["closed"], c["open"], c["multi"]) == (3292, 576, 112, 0, 0)
    if name == "open_solid":                                                   # open chains
        assert c["open"] > 0 and (c["rows"], c["degenerate"], c["closed"], c["open"], c["single"]) == (2532, 460, 11, 366, 47)
    if name == "nasty":                                                        # the pairing rule at work
        assert c["multi"] > 0 and (c["rows"], c["degenerate"], c["closed"], c["open"], c["multi"], c["single"]) == (17422, 21, 0, 15490, 618, 15427)
    if name == "bunny":                                                        # planes longer than a small tile
        assert (c["rows"], c["degenerate"], c["closed"], c["open"], c["longest"], c["largest_plane"]) == (16570, 109, 218, 39, 287, 341)


@pytest.mark.parametrize("name", PS.CPU_NAMES)
def test_a_flipped_copy_reverses_the_loops(bunny_small, name):
    tri, planes, sec, lp = _case(name, bunny_small)
    off, ids, seg, _ = PE.section(planes, PE.flipped(tri))
    assert np.array_equal(off, sec[0]) and np.array_equal(LE.bits(seg), LE.bits(sec[2])[:, ::-1])
    fl = LE.loops(off, seg, tri.shape[0])
    _check_structure(off, seg, fl, tri.shape[0])
    ok = fl.next >= 0                                                          # a flip swaps IN(k) and OUT(k) of every key, so the j-th of
                                                                               # one still meets the j-th of the other: next is INVERTED
                                                                               # whatever the multiplicity (`nasty` has 618 repeated keys)
    pairs = lambda frm, to: sorted(zip(frm.tolist(), to.tolist()))
    assert pairs(fl.next[ok], np.nonzero(ok)[0]) == pairs(np.nonzero(lp.next >= 0)[0], lp.next[lp.next >= 0])   # next, reversed
    assert np.array_equal(fl.plane_loops, lp.plane_loops) and np.array_equal(np.sort(fl.closed), np.sort(lp.closed))
    mine = sorted(tuple(lp.order[lp.loop_offsets[l]:lp.loop_offsets[l + 1]]) for l in range(lp.closed.size))
    rev = []
    for l in range(fl.closed.size):
        rows = [int(r) for r in fl.order[fl.loop_offsets[l]:fl.loop_offsets[l + 1]]]
        rows = rows[:1] + rows[:0:-1] if fl.closed[l] else rows[::-1]          # a cycle keeps its head (the lowest row)
        rev.append(tuple(rows))
    assert sorted(rev) == mine


def test_a_permutation_of_the_triangles_keeps_the_cycles(bunny_small):
    tri, planes, sec, lp = _case("voxel_solid", bunny_small)
    perm = np.random.default_rng(7).permutation(tri.shape[0])
    off, ids, seg, _ = PE.section(planes, tri[perm])
    other = LE.loops(off, seg, tri.shape[0])
    _check_structure(off, seg, other, tri.shape[0])
    assert np.array_equal(off, sec[0]) and not np.array_equal(other.order, lp.order)
    assert LE.canonical_cycles(other, seg) == LE.canonical_cycles(lp, sec[2]) and len(LE.canonical_cycles(lp, sec[2])) == 112


def test_the_area_of_a_section_of_the_voxel_solid():
    tri = IS.voxel_solid()["tri"]
    z = F([[0, 0, 1, 1.5], [0, 0, -1, -1.5]])
    off, ids, seg, _ = PE.section(z, tri)
    lp = LE.loops(off, seg, tri.shape[0])
    length, area = LE.measures(lp, seg, z)
    assert list(off) == [0, 32, 64] and lp.closed.all() and lp.order.size == 64
    assert area[lp.plane_loops[0]:lp.plane_loops[1]].sum() == 8.0 == area[lp.plane_loops[1]:lp.plane_loops[2]].sum()   # half-integers: exact
    assert (length > 0).all() and length[lp.plane_loops[0]:lp.plane_loops[1]].sum() == length[lp.plane_loops[1]:].sum()


def test_a_key_of_multiplicity_two_pairs_by_ascending_row():
    tri = LE.two_cubes()
    plane = F([[0, 0, 1, 0.5]])
    off, ids, seg, _ = PE.section(plane, tri)
    lp = LE.loops(off, seg, tri.shape[0])
    _check_structure(off, seg, lp, tri.shape[0])
    b = LE.bits(seg)
    key = F([1, 1, 0.5]).view(np.uint32)
    out = np.nonzero((b[:, 0] == key).all(1))[0]
    inn = np.nonzero((b[:, 1] == key).all(1))[0]
    assert out.size == 2 and inn.size == 2 and LE.multiplicity(off, seg) == 1
    assert lp.next[inn[0]] == out[0] and lp.next[inn[1]] == out[1]             # ascending row to ascending row
    assert off[-1] == 16 and lp.closed.all() and lp.order.size == 16
    length, area = LE.measures(lp, seg, plane)
    assert area.sum() == 2.0 and length.sum() == 8.0
    # the other order of the same triangles pairs the other way where the rows' order says so -- and still by ascending row
    off2, ids2, seg2, _ = PE.section(plane, tri[::-1])
    lp2 = LE.loops(off2, seg2, tri.shape[0])
    b2 = LE.bits(seg2)
    out2, inn2 = np.nonzero((b2[:, 0] == key).all(1))[0], np.nonzero((b2[:, 1] == key).all(1))[0]
    assert lp2.next[inn2[0]] == out2[0] and lp2.next[inn2[1]] == out2[1] and lp2.closed.all()


def test_planes_that_are_not_chained(bunny_small):
    tri, planes, sec, lp = _case("open_solid", bunny_small)
    off, seg, m = sec[0], sec[2], tri.shape[0]
    total = int(off[-1])
    last = int(np.nonzero(np.diff(off) > 0)[0][-1])
    short = LE.loops(off, seg, m, capacity=total - 1)                          # a section that did not fit: the last non-empty plane
    _check_structure(off, seg, short, m, capacity=total - 1)
    assert np.array_equal(short.plane_loops[:last + 1], lp.plane_loops[:last + 1]) and (short.plane_loops[last + 1:] == lp.plane_loops[last]).all()
    assert np.array_equal(short.next[:off[last]], lp.next[:off[last]]) and (short.next[off[last]:] == -9).all()
    assert np.array_equal(short.order, lp.order[:short.order.size]) and short.order.size < lp.order.size
    bad = LE.hostile_offsets(off, total, m)
    got = LE.loops(bad, seg, m)
    _check_structure(bad, seg, got, m)
    ok = LE.chained(bad, total, m)
    assert list(np.nonzero(~ok)[0]) == [4, 5, 12, 13, 29, 30, 49, 50] and got.order.size > 0
    for i in np.nonzero(ok)[0]:                                                # the others are unchanged
        assert np.array_equal(got.next[off[i]:off[i + 1]], lp.next[off[i]:off[i + 1]]) and np.diff(got.plane_loops)[i] == np.diff(lp.plane_loops)[i]
    gone = np.concatenate([np.arange(off[i], off[i + 1]) for i in (4, 5, 12, 13, 29, 30, 49, 50)])
    assert gone.size > 100 and (got.next[gone] == -9).all()

"""The numpy restatement of the plane clipping (tests/clip_expected.py; include/ezrt_clip.h, rules K1 to K8) held to what the header
says follows from the rules -- on the CPU, without the library.  tests/test_gpu_clip.py compares the device with the restatement on
the bits; this file is what makes the restatement worth comparing with.

Scenes and planes: tests/clip_scenes.py -- cube_pow2, the voxel solid, torus(32), the small Bunny, "nasty", `dead`, `signed_zero`; the
planes of plane_scenes.planes_for (through centroids, axis planes exactly through vertices with both signs, misses, not live) and
planes through three vertices of a triangle computed in fp32."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_expected as BE  # noqa: E402
import clip_expected as CE  # noqa: E402
import clip_scenes as CS  # noqa: E402
import orient_expected as OE  # noqa: E402
import orient_scenes as OS  # noqa: E402
import plane_expected as PE  # noqa: E402
import plane_loops_expected as PLE  # noqa: E402
import plane_scenes as PS  # noqa: E402
import topology_expected as TE  # noqa: E402

F = np.float32
_clips = {}


def _all(name, bunny_small):
    """(rows, planes, kinds, [Clip per plane]), computed once and shared"""
    if name not in _clips:
        R = CS.rows(name, bunny_small)
        p, kind = CS.planes(name, bunny_small)
        _clips[name] = (R, p, kind, [CE.clip(R, q) for q in p])
    return _clips[name]


def _keys(a, b):
    """the multiset of directed edges a -> b (float32 [r, 3] each) as 24-byte keys"""
    k = np.concatenate([CE.bits(a).reshape(-1, 3), CE.bits(b).reshape(-1, 3)], 1)
    return collections.Counter(x.tobytes() for x in np.ascontiguousarray(k))


@pytest.mark.parametrize("name", CS.NAMES)
def test_the_arrays_agree_with_one_another(bunny_small, name):
    R, planes, kind, clips = _all(name, bunny_small)
    n = R.shape[0]
    fin = np.isfinite(R[:, :9]).all(1)
    assert set(kind.tolist()) == {0, 1, 2, 3, 4}
    for p, kd, c in zip(planes, kind, clips):
        T = int(c.offsets[n])
        assert c.offsets[0] == 0 and (np.diff(c.offsets) == c.count).all() and c.count.min() >= 0 and c.count.max() <= 2
        assert c.summary.tolist() == [T, (c.kind == CE.WHOLE).sum(), (c.kind >= CE.ONE_UP).sum(), (fin & (c.count == 0)).sum(), (~fin).sum(),
                                      (c.cut_edge >= 0).sum(), int(kd != PS.KIND_DEAD), 0]
        assert c.out.shape == (T, 36) and (np.diff(c.src) >= 0).all() and (np.bincount(c.src, minlength=n) == c.count).all()
        assert CE.same_rows(c.out[:, 18:], R[c.src, 18:])                      # K5: the source row's material
        whole = c.kind[c.src] == CE.WHOLE
        assert np.array_equal(CE.bits(c.out[whole]), CE.bits(R[c.src[whole]])) and (c.cut_edge[whole] == -1).all()
        if kd == PS.KIND_DEAD:                                                 # K1: a plane that is not live keeps nothing
            assert T == 0 and c.summary[6] == 0 and c.summary[3] + c.summary[4] == n
        if kd == PS.KIND_MISS:
            assert c.summary[2] == 0 and T in (0, int(fin.sum()))
        # K8 on the count call's own offsets: every piece, each to its own row
        assert CE.candidates(c, c.offsets, T) == [(r, r) for r in range(T)]
        assert CE.candidates(c, c.offsets, T - 1) == [(r, r) for r in range(int(c.offsets[c.src[-1]]) if T else 0)]
        # P4's clamp: no piece leaves the box of its source row
        got, box = c.out[:, :9].reshape(-1, 3, 3), R[c.src, :9].reshape(-1, 3, 3)
        assert (got >= box.min(1, keepdims=True)).all() and (got <= box.max(1, keepdims=True)).all()


@pytest.mark.parametrize("name", CS.NAMES)
def test_cut_edges_are_the_section(bunny_small, name):
    """K6: the cut edge of an output row is P5's segment of its source row, q0 -> q1 on the bits -- and a row has one exactly when it
    emits cut pieces"""
    R, planes, kind, clips = _all(name, bunny_small)
    offsets, tri, seg, _ = PE.section(planes, R)
    for i, c in enumerate(clips):
        ids, sg = tri[offsets[i]:offsets[i + 1]], seg[offsets[i]:offsets[i + 1]]
        cs = CE.cut_segments(c)
        rows = c.src[c.cut_edge >= 0]
        assert np.array_equal(rows, np.nonzero(c.kind >= CE.ONE_UP)[0])          # one per cut row, in order
        assert np.isin(rows, ids).all()
        assert np.array_equal(CE.bits(cs), CE.bits(sg[np.searchsorted(ids, rows)]))
        # a crossed row without a cut edge touches the plane from below, with a vertex or with an edge
        rest = ids[~np.isin(ids, rows)]
        assert (c.count[rest] == 0).all()


@pytest.mark.parametrize("name", CS.CLOSED)
def test_closed_mesh_boundary_is_the_section(bunny_small, name):
    """on a closed, consistently wound manifold: no FLIPPED and no NONMANIFOLD edge among the clipped rows, and their BOUNDARY half-edges
    are the section's rows of non-zero length, on the bits and in direction"""
    R, planes, kind, clips = _all(name, bunny_small)
    t0 = TE.topology(R, components=False)
    assert TE.closed(t0) and TE.oriented(t0)
    offsets, tri, seg, _ = PE.section(planes, R)
    cases = ridges = 0
    for i, c in enumerate(clips):
        t = TE.topology(c.out, components=False)
        assert t.summary[4] == 0 and t.summary[5] == 0, (name, planes[i])
        h = np.nonzero(t.edge_class == TE.BOUNDARY)[0]
        P = c.out[:, :9].reshape(-1, 3)
        got = _keys(P[h], P[3 * (h // 3) + (h % 3 + 1) % 3])
        sg = seg[offsets[i]:offsets[i + 1]]
        sg = sg[(CE.bits(sg[:, 0]) != CE.bits(sg[:, 1])).any(1)]
        # (an edge IN the plane whose two triangles both lie below it is in the section twice, once each way, and bounds nothing
        # above the plane: such pairs cancel -- the torus's lowest ring under the plane through it)
        want = _keys(sg[:, 0], sg[:, 1]) - _keys(sg[:, 1], sg[:, 0])
        ridges += sum(_keys(sg[:, 0], sg[:, 1]).values()) - sum(want.values())
        assert got == want, (name, planes[i])
        cases += len(got) > 0
    assert cases >= 8 and (ridges > 0) == (name == "torus32")


@pytest.mark.parametrize("name", CS.NAMES)
def test_rotating_a_row_changes_no_cut_piece(bunny_small, name):
    R, planes, kind, clips = _all(name, bunny_small)
    k = np.random.default_rng(CS.SEED + 7).integers(0, 3, R.shape[0])
    R2 = CS.rotate_rows(R, k)
    for p, c in list(zip(planes, clips))[::2]:
        c2 = CE.clip(R2, p)
        assert np.array_equal(c2.offsets, c.offsets) and np.array_equal(c2.summary, c.summary) and np.array_equal(c2.src, c.src)
        assert np.array_equal(c2.cut_edge, c.cut_edge) and np.array_equal(c2.kind, c.kind)
        cut = c.kind[c.src] != CE.WHOLE
        assert CE.same_rows(c2.out[cut], c.out[cut])
        assert CE.same_rows(c2.out[~cut], R2[c.src[~cut]])


def _outline(rows):
    """the directed edges of the triangles `rows` [m, 36] that no other of them holds the other way round: their common outline"""
    V = rows[:, :9].reshape(-1, 3, 3)
    e = collections.Counter()
    for v in V:
        for j in range(3):
            a, b = CE.bits(v[j]).tobytes(), CE.bits(v[(j + 1) % 3]).tobytes()
            if a == b:
                continue
            if e[(b, a)] > 0:
                e[(b, a)] -= 1
            else:
                e[(a, b)] += 1
    return +e


@pytest.mark.parametrize("name", CS.NAMES)
def test_reversing_the_winding_reverses_every_piece(bunny_small, name):
    R, planes, kind, clips = _all(name, bunny_small)
    R2 = OS.reverse_rows(R, np.ones(R.shape[0], bool))
    swap = np.r_[0:3, 6:9, 3:6, 9:12, 15:18, 12:15, 18:36]
    for p, c in list(zip(planes, clips))[1::2]:
        c2 = CE.clip(R2, p)
        assert np.array_equal(c2.offsets, c.offsets) and np.array_equal(c2.summary, c.summary)
        one = c.count[c.src] == 1                                              # a single piece is the same triangle the other way round
        a, b = c.out[one], c2.out[one]
        rev = [b[:, swap], CS.rotate_rows(b, 1)[:, swap], CS.rotate_rows(b, 2)[:, swap]]
        same = [~((CE.bits(x) != CE.bits(a)) & ~(np.isnan(x) & np.isnan(a))).any(1) for x in rev]
        assert (same[0] | same[1] | same[2]).all()
        for k in np.nonzero(c.count == 2)[0][:200]:                            # two pieces: the same quadrilateral, the other way round
            o = int(c.offsets[k])
            want = collections.Counter({(y, x): m for (x, y), m in _outline(c.out[o:o + 2]).items()})
            assert _outline(c2.out[o:o + 2]) == want


@pytest.mark.parametrize("name", CS.NAMES)
def test_a_plane_and_its_negation_emit_every_vertex(bunny_small, name):
    R, planes, kind, clips = _all(name, bunny_small)
    V = R[:, :9].reshape(-1, 3, 3)
    fin = np.isfinite(V).all(axis=(1, 2))
    for p, kd, c in list(zip(planes, kind, clips))[::3]:
        if kd == PS.KIND_DEAD:
            continue
        cn = CE.clip(R, -p)
        s = PE.sides(p[None], V)[0]
        assert np.array_equal(PE.sides(-p[None], V)[0][fin], -s[fin])
        for cc, mask in ((c, s > 0), (cn, s < 0)):
            have = set()
            for r, k in zip(cc.out[:, :9].reshape(-1, 3, 3), cc.src):
                have.update((int(k), CE.bits(v).tobytes()) for v in r)
            k, j = np.nonzero(mask & fin[:, None])
            assert all((int(a), CE.bits(V[a, b]).tobytes()) in have for a, b in zip(k, j))
        assert c.summary[0] + cn.summary[0] >= fin.sum() - ((s == 0).any(1) & fin).sum()


def _chain(R, plane):
    """clip, topology, boundary, cap, topology, orientation -- on the restatements"""
    c = CE.clip(R, F(plane))
    t = TE.topology(c.out, components=False)
    b = BE.boundary(c.out, t.twin, t.edge_class)
    full = BE.capped(c.out, b)
    t2 = TE.topology(full)
    o = OE.orient(full, t2.twin, t2.edge_class, True)
    return c, t, b, full, t2, o


@pytest.mark.parametrize("plane,volume", (((0, 0, 1, 1), 48.0), ((0, 0, -1, -1), 16.0)))
def test_the_chain_on_the_cube(plane, volume):
    c, t, b, full, t2, o = _chain(CS.rows("cube_pow2"), plane)
    assert not TE.closed(t) and b.summary[1] == 1 and b.summary[2] == 1 and b.summary[4] == 0
    assert TE.closed(t2) and TE.oriented(t2) and t2.summary[6] == 1
    assert o.summary[1] == 1 and not o.flip.any() and not (o.pflags & (OE.OPEN | OE.NONORIENTABLE | OE.INWARD)).any()
    assert OE.patch_volume(o).tolist() == [volume]
    cap = full[c.out.shape[0]:]                                                # the cap faces -(a, b, c): outward
    nrm = np.cross(cap[:, 3:6] - cap[:, 0:3], cap[:, 6:9] - cap[:, 0:3])
    d = nrm @ np.asarray(plane[:3], np.float64)                                # (the loop has points in a line: some fan triangles are flat)
    assert cap.shape[0] >= 2 and (d <= 0).all() and (d < 0).sum() >= 2


@pytest.mark.parametrize("plane,loops", (((0.3, 0.2, 1, 0.1), None), ((0, 0, 1, 0), 2)))
def test_the_chain_on_the_torus(plane, loops):
    c, t, b, full, t2, o = _chain(CS.rows("torus32"), plane)
    assert c.summary[2] > 0 and not TE.closed(t) and b.summary[1] == b.summary[2] >= 1 and b.summary[4] == 0
    if loops is not None:
        assert b.summary[1] == loops                                           # an annulus
    # the boundary loops of the clipped rows are the plane loops of the same plane, as cyclic sequences of points on the bits
    R = CS.rows("torus32")
    off, _, seg, _ = PE.section(F(plane)[None], R)
    lp = PLE.loops(off, seg, R.shape[0])
    assert lp.closed.all() and lp.closed.size == b.summary[1]
    assert CE.canonical_cycles(c.out[:, :9].reshape(-1, 3)[b.order], b.loop_offsets) == PLE.canonical_cycles(lp, seg)
    assert TE.closed(t2) and TE.oriented(t2) and t2.summary[6] == 1
    assert o.summary[1] == 1 and not o.flip.any() and not (o.pflags & (OE.OPEN | OE.NONORIENTABLE | OE.INWARD)).any()

"""The rule of the plane loops (include/ezrt_plane_loops.h: L1 .. L6) restated with numpy and dictionaries on a section as
tests/plane_expected.py's `section` (or the device) returns it -- a helper, no test.  Integers and bit patterns only: there is no
floating-point operation in the rule."""
import collections

import numpy as np

Loops = collections.namedtuple("Loops", "next order plane_loops loop_offsets closed")


def bits(seg):
    """uint32 [rows, 2, 3]: the bit patterns of the end points"""
    return np.ascontiguousarray(seg, np.float32).reshape(-1, 2, 3).view(np.uint32)


def chained(offsets, capacity, n_tri):
    """L2: bool [n]"""
    o = np.asarray(offsets, np.int64)
    lo, hi = o[:-1], o[1:]
    return (lo >= 0) & (lo <= hi) & (hi <= capacity) & (hi - lo <= n_tri)


def degenerate(seg):
    """L3: bool [rows]"""
    b = bits(seg)
    return (b[:, 0] == b[:, 1]).all(1)


def loops(offsets, seg, n_tri, capacity=None):
    """L1 .. L6: Loops(next int64 [capacity] (rows the call does not touch hold -9), order int64 [chained rows], plane_loops int64
    [n + 1], loop_offsets int64 [L + 1], closed uint8 [L]) of the section (offsets [n + 1], seg [capacity or more rows, 2, 3])"""
    o = np.asarray(offsets, np.int64)
    b = bits(seg)
    cap = b.shape[0] if capacity is None else capacity
    ok = chained(o, cap, n_tri)
    nxt = np.full(cap, -9, np.int64)
    order, plane_loops, lengths, closed = [], [0], [], []
    for i in range(o.size - 1):
        if not ok[i]:
            plane_loops.append(plane_loops[-1])
            continue
        r0, r1 = int(o[i]), int(o[i + 1])
        nxt[r0:r1] = -1
        rows = [r for r in range(r0, r1) if not (b[r, 0] == b[r, 1]).all()]           # L3 (ascending)
        out, inn = collections.defaultdict(list), collections.defaultdict(list)       # L4
        for r in rows:
            out[b[r, 0].tobytes()].append(r)
            inn[b[r, 1].tobytes()].append(r)
        pred = {}
        for k, ins in inn.items():
            for a, c in zip(ins, out.get(k, ())):
                nxt[a] = c
                pred[c] = a
        seen = set()                                                                  # L5, L6
        heads = [r for r in rows if r not in pred]                                    # paths, in ascending head row
        found = []
        for h in heads:
            chain = [h]
            while nxt[chain[-1]] >= 0:
                chain.append(int(nxt[chain[-1]]))
            seen.update(chain)
            found.append((h, chain, 0))
        for r in rows:                                                                # what is left lies on cycles: the first row met
            if r in seen:                                                             # of each is its lowest
                continue
            chain = [r]
            while nxt[chain[-1]] != r:
                chain.append(int(nxt[chain[-1]]))
            seen.update(chain)
            found.append((r, chain, 1))
        found.sort(key=lambda f: f[0])
        for h, chain, c in found:
            order.extend(chain)
            lengths.append(len(chain))
            closed.append(c)
        plane_loops.append(plane_loops[-1] + len(found))
    loop_offsets = np.zeros(len(lengths) + 1, np.int64)
    loop_offsets[1:] = np.cumsum(np.asarray(lengths, np.int64))
    return Loops(nxt, np.asarray(order, np.int64), np.asarray(plane_loops, np.int64), loop_offsets, np.asarray(closed, np.uint8))


def polylines(lp, seg):
    """per loop (closed, points float32 [len, 3]): the q0 of its rows in order (an open loop's last q1 is not appended)"""
    s = np.ascontiguousarray(seg, np.float32).reshape(-1, 2, 3)
    return [(int(lp.closed[l]), s[lp.order[lp.loop_offsets[l]:lp.loop_offsets[l + 1]], 0]) for l in range(lp.closed.size)]


def canonical_cycles(lp, seg):
    """the sorted list of the closed loops' cyclic point sequences, each rotated to start at its least point (bytes of the bit
    patterns): equal for two sections that differ in the order of their rows, where no key repeats"""
    out = []
    for c, pts in polylines(lp, seg):
        if not c:
            continue
        keys = [p.tobytes() for p in pts]
        k = keys.index(min(keys))
        out.append(tuple(keys[k:] + keys[:k]))
    return sorted(out)


def multiplicity(offsets, seg):
    """the number of (plane, key) pairs that more than one non-degenerate row holds as q0, or more than one as q1"""
    o = np.asarray(offsets, np.int64)
    b = bits(seg)
    many = 0
    for i in range(o.size - 1):
        c0, c1 = collections.Counter(), collections.Counter()
        for r in range(int(o[i]), int(o[i + 1])):
            if not (b[r, 0] == b[r, 1]).all():
                c0[b[r, 0].tobytes()] += 1
                c1[b[r, 1].tobytes()] += 1
        many += len({k for k, v in c0.items() if v > 1} | {k for k, v in c1.items() if v > 1})
    return many


def measures(lp, seg, planes):
    """(length, area) float64 [L]: sum |q1 - q0| and 1/2 sum n^ . (q0 x q1) over each loop's rows, in numpy"""
    s = np.ascontiguousarray(seg, np.float32).reshape(-1, 2, 3).astype(np.float64)
    p = np.asarray(planes, np.float64).reshape(-1, 4)
    L = lp.closed.size
    length, area = np.zeros(L), np.zeros(L)
    for i in range(p.shape[0]):
        nrm = p[i, :3] / np.sqrt((p[i, :3] * p[i, :3]).sum())
        for l in range(int(lp.plane_loops[i]), int(lp.plane_loops[i + 1])):
            rows = lp.order[lp.loop_offsets[l]:lp.loop_offsets[l + 1]]
            q0, q1 = s[rows, 0], s[rows, 1]
            length[l] = np.sqrt(((q1 - q0) ** 2).sum(1)).sum()
            area[l] = 0.5 * (np.cross(q0, q1) @ nrm).sum()
    return length, area


def _cube(lo, hi):
    """the 12 outward counter-clockwise triangles of the box [lo, hi] as rows of 36 floats (vertices only)"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (3, 0, 4, 7)]
    T = np.zeros((12, 36), np.float32)
    for q, (a, b, cc, d) in enumerate(quads):
        T[2 * q, :9] = np.concatenate([c[a], c[b], c[cc]])
        T[2 * q + 1, :9] = np.concatenate([c[a], c[cc], c[d]])
    return T


def two_cubes():
    """two unit cubes that touch along the edge x = 1, y = 1"""
    return np.concatenate([_cube((0, 0, 0), (1, 1, 1)), _cube((1, 1, 0), (2, 2, 1))])


def hostile_offsets(off, capacity, n_tri):
    """a copy of a section's offsets (at least 60 planes) with entries that no count call writes: negative, beyond the capacity,
    descending, a span above n_tri.  Every edit shrinks or unchains the two planes it borders, so the planes that stay chained keep
    their own rows and no two of them overlap."""
    bad = np.array(off, np.int64)
    a, p, b, d = 5, 12, 30, 50
    assert bad.size > 60 and off[p] + n_tri + 1 <= capacity and off[p + 2] <= off[p] + n_tri
    bad[a] = -5                              # plane a - 1 descends to a negative end, plane a starts below 0
    bad[p + 1] = off[p] + n_tri + 1          # plane p spans more than n_tri rows inside the capacity; plane p + 1 descends
    bad[b] = capacity + 7                    # plane b - 1 ends beyond the capacity, plane b descends from there
    bad[d] = -2 ** 62                        # plane d - 1 descends, plane d has a span far above n_tri from a negative start
    return bad

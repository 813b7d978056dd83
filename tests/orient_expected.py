"""The mesh orientation of include/ezrt_orient.h (rules O1 to O8) restated on the host -- a helper, no test.  numpy only.

orient(tri, twin, edge_class, outward) takes the scene's triangle rows ([n, 36] or [n, 9] or [n, 3, 3] float32) and the two arrays of a
topology (or any garbage of that size: O2 reads nothing out of bounds) and returns every array of the device call; rewind(rows, flip)
is ezrt_rewind_device on a copy.  Links are found by O2, patches by a breadth-first walk with parity from the lowest id of each
patch, O4 by a check of every link afterwards, O6 with numpy float64 in exactly the written order and Python integers for the sums.
tests/test_orient_expected.py holds it to the properties the header states."""
import collections

import numpy as np

OPEN, NONORIENTABLE, REWOUND, INWARD = 1, 2, 4, 8
Orient = collections.namedtuple("Orient", "flip patch_root patch proot psize pflags vol6 summary takes link q scale")


def vertices(tri):
    """float32 [n, 3, 3]"""
    T = np.ascontiguousarray(tri, np.float32)
    if T.ndim == 2 and T.shape[1] == 36:
        T = T[:, :9]
    return np.ascontiguousarray(T.reshape(-1, 3, 3))


def links(twin, edge_class):
    """O1 and O2: (takes bool [n], link int64 [3 n]: the half-edge g that h is a link to, or -1)"""
    tw = np.asarray(twin).reshape(-1).astype(np.int64)
    cl = np.asarray(edge_class).reshape(-1).astype(np.int64)
    H = tw.shape[0]
    n = H // 3
    takes = ((cl.reshape(n, 3) >= 1) & (cl.reshape(n, 3) <= 4)).all(1)
    h = np.arange(H)
    ok = np.repeat(takes, 3) & ((cl == 2) | (cl == 3)) & (tw >= 0) & (tw < H)
    g = np.where(ok, tw, 0)                                                    # read only where the tests so far hold
    ok &= (g // 3 != h // 3) & takes[g // 3] & (cl[g] == cl) & (tw[g] == h)
    return takes, np.where(ok, g, -1)


def scale(V, takes):
    """O6: S = 3 E - 30, E the frexp exponent of the largest finite |coordinate| of the triangles that take part"""
    B = V[takes].view(np.uint32) & np.uint32(0x7FFFFFFF)
    B = B[(B & 0x7F800000) != 0x7F800000]
    A = float(B.max().view(np.float32)) if B.size else 0.0                   # compared on the bits: the order of finite |x| is theirs
    E = int(np.frexp(np.float64(A))[1]) if A != 0.0 else 0
    return 3 * E - 30


def q_of(V, S):
    """O6: q(t) of every triangle, a list of Python ints"""
    with np.errstate(all="ignore"):
        D = V.astype(np.float64)
        a, b, c = D[:, 0], D[:, 1], D[:, 2]
        ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
        bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        d = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)
        r = np.rint(np.ldexp(d, -S))                                           # round to nearest even
    return [int(x) if np.isfinite(y) else 0 for x, y in zip(r, d)]


def orient(tri, twin, edge_class, outward):
    V = vertices(tri)
    n = V.shape[0]
    takes, link = links(twin, edge_class)
    assert takes.shape[0] == n
    cl = np.asarray(edge_class).reshape(-1)
    S = scale(V, takes)
    q = q_of(V, S)
    adj = [[] for _ in range(n)]                                               # (neighbour, sigma) per link
    for h in np.nonzero(link >= 0)[0]:
        adj[h // 3].append((int(link[h]) // 3, 1 if cl[h] == 3 else 0))
    patch_root = np.full(n, -1, np.int32)
    patch = np.full(n, -1, np.int32)
    f0 = np.zeros(n, np.uint8)
    flip = np.zeros(n, np.uint8)
    proot, psize, pflags, vol6 = [], [], [], []
    for r in range(n):                                                         # ascending: r is the lowest id of its patch
        if not takes[r] or patch_root[r] >= 0:
            continue
        p = len(proot)
        patch_root[r], patch[r] = r, p
        members, queue = [r], collections.deque([r])
        while queue:
            a = queue.popleft()
            for b, s in adj[a]:
                if patch_root[b] < 0:
                    patch_root[b], patch[b], f0[b] = r, p, f0[a] ^ s
                    members.append(b)
                    queue.append(b)
        orientable = all(f0[a] ^ f0[b] == s for a in members for b, s in adj[a])   # O4, every link
        closed = all(link[3 * a + e] >= 0 for a in members for e in range(3))     # O5
        if not orientable:
            for a in members:
                f0[a] = 0
        v0 = sum(-q[a] if f0[a] else q[a] for a in members)
        inward = orientable and closed and v0 < 0
        act = bool(outward) and inward                                         # O7
        for a in members:
            flip[a] = f0[a] ^ (1 if act else 0)
        rewound = any(flip[a] for a in members)
        proot.append(r)
        psize.append(len(members))
        pflags.append((0 if closed else OPEN) | (0 if orientable else NONORIENTABLE) | (REWOUND if rewound else 0) | (INWARD if inward else 0))
        vol6.append(-v0 if act else v0)
    pf = np.array(pflags, np.uint8)
    summary = np.array([int(takes.sum()), len(proot), int(((pf & NONORIENTABLE) == 0).sum()), int(((pf & OPEN) == 0).sum()), int(flip.sum()),
                        int(((pf & INWARD) != 0).sum()), S, 0], np.int64)
    assert all(-2 ** 63 <= v < 2 ** 63 for v in vol6)
    return Orient(flip, patch_root, patch, np.array(proot, np.int32), np.array(psize, np.int32), pf, np.array(vol6, np.int64), summary, takes,
                  link, q, S)


def rewind(rows, flip):
    """ezrt_rewind_device on a copy of rows [n, 36] (or [n, 3, 3]: the vertices alone)"""
    R = np.array(rows, np.float32)
    f = np.asarray(flip).astype(bool)
    if R.ndim == 3:
        R[f] = R[f][:, [0, 2, 1]]
        return R
    for lo in (3, 12):
        a, b = R[f, lo:lo + 3].copy(), R[f, lo + 3:lo + 6].copy()
        R[f, lo:lo + 3], R[f, lo + 3:lo + 6] = b, a
    return R


def patch_volume(o):
    """float64 [P]: vol6 * 2 ** S / 6"""
    return o.vol6.astype(np.float64) * 2.0 ** o.scale / 6

"""The boxes of the oriented-box tests on the device (tests/test_gpu_obb_overlap.py, tools/obb_overlap_host_check.py; a helper, no
test): about 2 000 boxes per scene, drawn with a fixed seed from the kinds that can go wrong -- axis-aligned boxes whose planes
coincide with the planes of the tree's slots and of the triangles' own bounding boxes, the same turned by 90 degrees (exact in fp32),
thin boxes along diagonals (the hull passes much, the face directions must prune), sheared boxes, small boxes at the surface, a box
that holds everything, boxes that are not live."""
import numpy as np

F = np.float32
NODE, TRI, TURNED, THIN, SHEARED, LOCAL, WHOLE, DEAD = range(8)
THIN_ASPECT = 20.0         # a thin box is at least this many times longer than thick


def _aligned(lo, hi, small):
    """(centre, axes) of the axis-aligned boxes [lo, hi]; an extent of zero becomes 2 * small (a box without volume is not live)"""
    c = ((lo + hi) * F(0.5)).astype(F)
    h = ((hi - lo) * F(0.5)).astype(F)
    h = np.where(h > 0, h, small).astype(F)
    u = np.zeros((c.shape[0], 3, 3), F)
    for j in range(3):
        u[:, j, j] = h[:, j]
    return c, u


def _rotations(rng, n):
    """float64 [n, 3, 3]: random rotations (rows orthonormal)"""
    q = np.linalg.qr(rng.normal(0, 1, (n, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def _surface(rng, P, n, spread):
    t = rng.integers(0, P.shape[0], n)
    w = rng.dirichlet((1, 1, 1), n).astype(F)
    return ((P[t] * w[:, :, None]).sum(1) + rng.normal(0, spread, (n, 3))).astype(F)


def boxes_for(tri, nodes, seed, n=2000):
    """(centre float32 [n', 3], axes float32 [n', 3, 3], kind int [n']) for the scene's triangle array [m, 36] and the caller's tree
    [*, 12] (box at floats 6-11)"""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(tri, F).reshape(-1, 36)[:, :9].reshape(-1, 3, 3)
    N = np.ascontiguousarray(nodes, F).reshape(-1, 12)[1:]
    m = P.shape[0]
    blo, bhi = np.percentile(P.reshape(-1, 3), [2, 98], axis=0)
    size = float(np.max(bhi - blo))
    small = F(2.0 ** np.floor(np.log2(0.01 * size)))
    k = n // 7
    parts = []
    # node boxes of the caller's tree and triangle bounding boxes as axis-aligned boxes: box planes coincide with slot planes
    sel = rng.integers(0, N.shape[0], k)
    parts.append(_aligned(N[sel, 6:9], N[sel, 9:12], small) + (NODE,))
    t = rng.integers(0, m, k)
    parts.append(_aligned(P[t].min(1), P[t].max(1), small) + (TRI,))
    # the same kinds turned by 90 degrees about a coordinate axis through their centre: a signed permutation of the components
    sel, t = rng.integers(0, N.shape[0], k - k // 2), rng.integers(0, m, k // 2)
    c, u = _aligned(np.concatenate([N[sel, 6:9], P[t].min(1)]), np.concatenate([N[sel, 9:12], P[t].max(1)]), small)
    ax = rng.integers(0, 3, k)
    a, b = (ax + 1) % 3, (ax + 2) % 3
    r = np.arange(k)
    turned = u.copy()
    turned[r, :, a], turned[r, :, b] = -u[r, :, b], u[r, :, a]
    parts.append((c, turned, TURNED))
    # thin boxes along random diagonals through points of the surface
    R = _rotations(rng, 2 * k)
    length = size * 10.0 ** rng.uniform(-1.3, -0.4, (2 * k, 1))
    R[:, 0] *= length
    R[:, 1] *= length / rng.uniform(THIN_ASPECT, 3 * THIN_ASPECT, (2 * k, 1))
    R[:, 2] *= length / rng.uniform(THIN_ASPECT, 3 * THIN_ASPECT, (2 * k, 1))
    parts.append((_surface(rng, P, 2 * k, 0.002 * size), R[:, rng.permutation(3)].astype(F), THIN))
    # sheared boxes: a rotated box whose axes lean into one another
    R = _rotations(rng, k) * (size * 10.0 ** rng.uniform(-2.5, -0.8, (k, 3, 1)))
    lean = np.eye(3) + rng.uniform(-0.9, 0.9, (k, 3, 3)) * (1 - np.eye(3))
    parts.append((_surface(rng, P, k, 0.01 * size), np.einsum("nij,njc->nic", lean, R).astype(F), SHEARED))
    # rotated boxes a leaf's size around points of the surface, a few larger
    R = _rotations(rng, k) * (size * 10.0 ** rng.uniform(-3, -0.8, (k, 1, 1)) * rng.uniform(0.3, 1.0, (k, 3, 1)))
    R[:8] *= 6.0
    parts.append((_surface(rng, P, k, 0.01 * size), R.astype(F), LOCAL))
    # one box that holds the whole scene, with room to spare
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    c, u = _aligned(lo[None], hi[None], small)
    parts.append((c, (u * F(1.25)).astype(F), WHOLE))
    # boxes that are not live, of every kind above: a zero axis, two parallel axes, three coplanar axes, a NaN, an infinity
    j = 70
    c = np.concatenate([p[0] for p in parts])
    u = np.concatenate([p[1] for p in parts])
    pick = rng.permutation(c.shape[0])[:j]
    pick[:7] = [0, k, 2 * k, 3 * k, 5 * k, 6 * k, 7 * k]               # one of each kind for sure
    c, u = c[pick].copy(), u[pick].copy()
    r, ax, what = np.arange(j), rng.integers(0, 3, j), (np.arange(j) + 3) % 7
    s = what == 0
    u[r[s], ax[s]] = 0
    s = what == 1
    u[r[s], ax[s]] = u[r[s], (ax[s] + 1) % 3] * F(-0.5)
    s = what == 2
    u[r[s], ax[s]] = u[r[s], (ax[s] + 1) % 3] + u[r[s], (ax[s] + 2) % 3] * F(2)
    s = what == 3
    u[r[s], ax[s], (ax[s] + 1) % 3] = np.nan
    s = what == 4
    u[r[s], ax[s], ax[s]] = np.inf
    s = what == 5
    c[r[s], ax[s]] = np.nan
    s = what == 6
    c[r[s], ax[s]] = -np.inf
    parts.append((c, u, DEAD))
    centre = np.concatenate([p[0] for p in parts]).astype(F)
    axes = np.concatenate([p[1] for p in parts]).astype(F)
    kind = np.concatenate([np.full(p[0].shape[0], p[2]) for p in parts])
    order = rng.permutation(centre.shape[0])
    return np.ascontiguousarray(centre[order]), np.ascontiguousarray(axes[order]), kind[order]


def hulls(centre, axes):
    """(lo, hi) float32 [n, 3]: the axis-aligned boxes a caller of box_overlap would ask for instead, rounded outward"""
    c, h = centre.astype(np.float64), np.abs(axes.astype(np.float64)).sum(1)
    lo, hi = (c - h).astype(F), (c + h).astype(F)
    with np.errstate(invalid="ignore"):
        lo = np.where(lo.astype(np.float64) > c - h, np.nextafter(lo, F(-np.inf)), lo)
        hi = np.where(hi.astype(np.float64) < c + h, np.nextafter(hi, F(np.inf)), hi)
    return lo, hi


def visited(centre, axes, nodes, both):
    """int [n]: the number of triangles below the leaves that a depth-first walk of the caller's tree reaches for each box, descending
    a node when its box passes the hull gate (both = False) or both gates (both = True) of tests/obb_overlap_expected.py; and
    bool [n]: whether some node that the walk met passed the hull gate and failed the face gate"""
    import obb_overlap_expected as OE
    N = np.ascontiguousarray(nodes, F).reshape(-1, 12)
    B = OE.Boxes(centre, axes)
    n = B.c.shape[0]
    count, bitten = np.zeros(n, np.int64), np.zeros(n, bool)
    stack = [(1, np.nonzero(B.live)[0])]
    while stack:
        i, boxes = stack.pop()
        if boxes.size == 0:
            continue
        Bi = B.take(boxes)
        lo, hi = np.tile(N[i, 6:9], (boxes.size, 1)), np.tile(N[i, 9:12], (boxes.size, 1))
        if i > 1:                                                      # (the root's own box is never tested)
            hull = OE.hull_passes(Bi, lo, hi)
            face = OE.face_passes(Bi, lo, hi)
            bitten[boxes[hull & ~face]] = True
            boxes = boxes[hull & face] if both else boxes[hull]
        if N[i, 3] > 0:
            count[boxes] += int(N[i, 3])
        else:
            stack.append((int(N[i, 0]), boxes))
            stack.append((int(N[i, 1]), boxes))
    return count, bitten

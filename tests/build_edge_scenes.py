"""The edge inputs of the builder tests (tests/test_build_edge_scenes.py on the CPU, tests/test_gpu_build_edges.py on the device)
-- a helper, no test.  numpy only: no GPU, no library.

Every generator returns triangles in the reference layout [n, 36] (p1 p2 p3, three normals, then the material) with `arange(n)` in
the emissive column, so that repeated triangles stay distinguishable after a builder has reordered them.  `rnd(n, seed, scale, off)`
is the cluster generator of tests/test_gpu_lbvh.py (`_random_tris`: centres uniform in [-2, 2], vertices within 0.3 of them), scaled
and shifted in float64 before the cast to float32.

  dup_chain          copies of ONE triangle: every SAH cost is S (r - l + 1), the first minimum wins, the split lands at l -- one
                     triangle peeled per level, depth n - leaf_n + 1
  line               point-triangles on the x axis at shuffled positions: every box has two zero extents, S == 0, every cost +0:
                     the same chain
  flat               z = 0.25 everywhere: one zero extent
  signed0            the half-integer grid with every zero replaced at random by -0.0 or +0.0
  big                rnd(400): the INF = 114514 cost cap holds at the top levels only
  beyond_inf         rnd(1e5): coordinates beyond 114514, the start value of the prefix boxes -- every node is capped
  beyond_sentinel    rnd(1e7, 2.5e9): every coordinate beyond 1145141919, the start value of new_node
  tiny               rnd(1e-20): area products are subnormal
  subnormal          rnd(1e-39): coordinates and centroids are subnormal, every cost underflows to 0
  inf                +inf in one coordinate of every 37th triangle, -inf in one of every 41st (offset 5): never both signs in one
                     triangle, which would make a NaN centroid
  overflow_centroid  rnd(1e38): finite vertices whose centroid sums overflow to +-inf
  near_flt_max       40 triangles with every x in [3.401e38, 3.402e38] (FLT_MAX = 3.4028235e38)            -- linear BVH only
  nan_vertex         one NaN coordinate in one vertex of three triangles                                   -- linear BVH only
  size_<n>, ties_<n> rnd() at the sizes where the device sorts and scans change shape; ties_<n> is `_random_tris(ties=True)`"""
import numpy as np

SEED = 2700
N = 300
CHAIN_N = 4200     # depth 4193 at leaf_n = 8: beyond the 4096 levels the device SAH builder once stopped at
SIZES = (2, 3, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4097)
TIES = (256, 257, 1025)
NAN_AT = ((7, 0), (120, 4), (255, 8))      # (triangle, coordinate of its nine) that holds a NaN in `nan_vertex`


def _tri36(P):
    P = np.asarray(P, np.float32)
    n = P.shape[0]
    T = np.zeros((n, 36), np.float32)
    T[:, :9] = P.reshape(n, 9)
    T[:, 9:18] = np.tile([0, 1, 0], 3)
    T[:, 18:21] = np.arange(n, dtype=np.float32)[:, None]      # tell repeated triangles apart
    return T


def _points(n, seed, scale=1.0, off=0.0):
    """[n, 3 vertices, 3] float64"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2, 2, (n, 1, 3))
    return (c + rng.uniform(-0.3, 0.3, (n, 3, 3))) * scale + off


def rnd(n=N, seed=SEED, scale=1.0, off=0.0):
    return _tri36(_points(n, seed, scale, off))


def ties(n, seed=SEED):
    """a coarse grid and repeated triangles: many equal centroid keys and equal costs"""
    P = (np.round(_points(n, seed) * 2) / 2).astype(np.float32)
    P[n // 2:] = P[: n - n // 2]
    return _tri36(P)


def dup_chain(n=CHAIN_N):
    one = np.float32([[0.25, -0.5, 1.0], [1.5, 0.75, -0.25], [-0.75, 1.25, 0.5]])
    return _tri36(np.repeat(one[None], n, axis=0))


def line(n=150):
    x = np.random.default_rng(SEED + 1).permutation(n).astype(np.float32) * np.float32(0.25) - np.float32(3.0)
    P = np.zeros((n, 3, 3), np.float32)
    P[:, :, 0] = x[:, None]
    return _tri36(P)


def flat():
    P = _points(N, SEED + 2)
    P[:, :, 2] = 0.25
    return _tri36(P)


def signed0():
    P = (np.round(_points(N, SEED + 3) * 2) / 2).astype(np.float32)
    zero = P == 0
    sign = np.random.default_rng(SEED + 4).integers(0, 2, P.shape).astype(bool)
    P[zero & sign] = np.float32(-0.0)
    P[zero & ~sign] = np.float32(0.0)
    return _tri36(P)


def big():
    return rnd(N, SEED + 5, 400.0)


def beyond_inf():
    return rnd(N, SEED + 6, 1e5)


def beyond_sentinel():
    return rnd(N, SEED + 7, 1e7, 2.5e9)


def tiny():
    return rnd(N, SEED + 8, 1e-20)


def subnormal():
    return rnd(N, SEED + 9, 1e-39)


def inf():
    T = rnd(N, SEED + 10)
    for i in range(0, N, 37):
        T[i, i % 9] = np.inf
    for i in range(5, N, 41):
        T[i, (i + 4) % 9] = -np.inf
    return T


def overflow_centroid():
    return rnd(N, SEED + 11, 1e38)


def near_flt_max():
    P = _points(40, SEED + 12)
    P[:, :, 0] = np.random.default_rng(SEED + 13).uniform(3.401e38, 3.402e38, (40, 3))
    return _tri36(P)


def nan_vertex():
    T = rnd(N, SEED + 14)
    for t, c in NAN_AT:
        T[t, c] = np.nan
    return T


CASES = {"dup_chain": dup_chain, "line": line, "flat": flat, "signed0": signed0, "big": big, "beyond_inf": beyond_inf,
         "beyond_sentinel": beyond_sentinel, "tiny": tiny, "subnormal": subnormal, "inf": inf,
         "overflow_centroid": overflow_centroid, "near_flt_max": near_flt_max, "nan_vertex": nan_vertex}
for _n in SIZES:
    CASES["size_%d" % _n] = (lambda n=_n: rnd(n, SEED + 100 + n))
for _n in TIES:
    CASES["ties_%d" % _n] = (lambda n=_n: ties(n, SEED + 200 + n))

SIZE_NAMES = tuple("size_%d" % n for n in SIZES) + tuple("ties_%d" % n for n in TIES)
LBVH_ONLY = ("near_flt_max", "nan_vertex")      # no parity builder contract: see include/ezrt_build.h
ALL_NAMES = tuple(CASES)
PARITY_NAMES = tuple(k for k in CASES if k not in LBVH_ONLY)
HITTABLE = ("flat", "signed0", "big", "beyond_inf", "tiny") + SIZE_NAMES      # rays can hit these: three-way comparison
UNHITTABLE = ("tiny",)      # hitTriangle's normalize underflows on them: tests/test_build_edge_scenes.py shows it
_cache = {}


def rays_at(tri36, n, seed):
    """[n, 6] finite rays aimed at the box of the case's own finite coordinates: origins in the box inflated by half (a flat box
    by half its largest extent; kept inside float32), targets inside the box"""
    rng = np.random.default_rng(seed)
    V = np.asarray(tri36, np.float32)[:, :9].reshape(-1, 3).astype(np.float64)
    V[~np.isfinite(V)] = np.nan
    lo, hi = np.nanmin(V, axis=0), np.nanmax(V, axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    o = np.clip(mid + rng.uniform(-1.5, 1.5, (n, 3)) * np.maximum(half, 0.5 * half.max()), -3e38, 3e38)
    d = mid + rng.uniform(-1, 1, (n, 3)) * half - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


def case(name):
    """tri36 of a case; built once, handed out read-only"""
    if name not in _cache:
        T = np.ascontiguousarray(CASES[name](), np.float32)
        T.setflags(write=False)
        _cache[name] = T
    return _cache[name]


def centroids(tri36):
    """the builders' sort keys, ((p1 + p2) + p3) / 3 in float32"""
    P = np.asarray(tri36, np.float32)[:, :9].reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        return (((P[:, 0] + P[:, 1]) + P[:, 2]) / np.float32(3.0)).astype(np.float32)

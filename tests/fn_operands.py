"""Operands of the function-level pins, shared by tests/test_ref_fsh_pin.py (executed shader == oracle, CPU) and
tests/test_gpu_fn_parity.py (oracle == device, GPU), so that both statements are about identical inputs.

Two families per function: the RANDOM sets (10^5 rows, the seeds and generators test_ref_fsh_pin.py has always used) and
an EDGE set, written out below row by row with a label per row: every branch and every degenerate operand the functions
can meet.  Op numbers and layouts are include/ezrt.h's (ezrt_debug_fn).
"""
import numpy as np

N_FN = 100_000
TINY_N = np.float32(1.17549435e-38)      # the smallest normal fp32
TINY_S = np.float32(1e-42)               # a subnormal
TINY_S1 = np.float32(1.4e-45)            # the smallest subnormal
# material floats: 0-2 emissive, 3-5 baseColor, 6 subsurface, 7 metallic, 8 specular, 9 specularTint, 10 roughness,
# 11 anisotropic, 12 sheen, 13 sheenTint, 14 clearcoat, 15 clearcoatGloss, 16 IOR, 17 transmission
SCALARS = {6: "subsurface", 7: "metallic", 8: "specular", 9: "specularTint", 10: "roughness", 11: "anisotropic",
           12: "sheen", 13: "sheenTint", 14: "clearcoat", 15: "clearcoatGloss"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Bit equality; a NaN equals a NaN (include/ezrt.h: sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def mismatches(a, b):
    """Row numbers where a and b differ on the bits (NaN == NaN)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    bad = ~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))
    return np.flatnonzero(bad.reshape(bad.shape[0], -1).any(1))


def nonfinite_rows(a):
    a = np.asarray(a, np.float32)
    return ~np.isfinite(a.reshape(a.shape[0], -1)).all(1)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _materials(rng, n):
    """Random Disney parameters, with the edge values the reference's branches test mixed in (metallic 1, roughness 0,
    clearcoatGloss 0 / 1 -> GTR1's a >= 1 branch is unreachable but a = 0.1 / 0.001 are, black base colour -> Cdlum = 0)."""
    m = rng.uniform(0.0, 1.0, (n, 18)).astype(np.float32)
    m[:, 0:3] = 0.0
    edge = rng.integers(0, 8, n)
    m[edge == 0, 7] = 1.0          # metallic
    m[edge == 1, 10] = 0.0         # roughness
    m[edge == 2, 15] = 1.0         # clearcoatGloss
    m[edge == 3, 15] = 0.0
    m[edge == 4, 3:6] = 0.0        # baseColor black: Ctint = vec3(1)
    m[edge == 5, 14] = 0.0         # clearcoat
    return m


def _vnl(rng, n):
    """V N L triples: N random, V and L mostly in N's hemisphere, a share below it (the early returns)."""
    N = _unit(rng, n)
    V, L = _unit(rng, n), _unit(rng, n)
    flip_v = (np.einsum("ij,ij->i", V, N) < 0) & (rng.uniform(size=n) < 0.85)
    flip_l = (np.einsum("ij,ij->i", L, N) < 0) & (rng.uniform(size=n) < 0.85)
    V[flip_v] = -V[flip_v]
    L[flip_l] = -L[flip_l]
    return np.concatenate([V, N, L], 1).astype(np.float32)


# ---- the random sets, one function per test of test_ref_fsh_pin.py (its seed, its order of draws) ----------------------
def evaluate_iso_random():
    rng = np.random.default_rng(1)
    return _vnl(rng, N_FN), _materials(rng, N_FN)


def evaluate_uniform_random():
    rng = np.random.default_rng(2)
    return _vnl(rng, N_FN), _materials(rng, N_FN)


def sample_brdf_random():
    """-> (a of op 3, materials, V N L of the same draw: op 4's operands are (V, N, sampled L) and these)."""
    rng = np.random.default_rng(3)
    m = _materials(rng, N_FN)
    xi = rng.uniform(0, 1, (N_FN, 3)).astype(np.float32)
    xi[:64, 2] = np.float32(1.0)       # rand() can return exactly 1.0: the clearcoat branch's upper edge
    xi[64:128, 1] = np.float32(1.0)
    vn = _vnl(rng, N_FN)
    return np.concatenate([xi, vn[:, 0:6]], 1), m, vn


def hemisphere_random():
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.uniform(0, 1, (N_FN, 2)).astype(np.float32), _unit(rng, N_FN)], 1)
    a[:16, 0] = np.float32(1.0)
    a[16:32, 2:5] = np.float32([1, 0, 0])      # |N.x| > 0.999: the other helper axis
    return a


def env_random():
    """-> (L of ops 5, 7, 10; xi of op 6)"""
    rng = np.random.default_rng(5)
    L = _unit(rng, N_FN)
    L[:8] = np.float32([[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 1e-20], [-1, 0, -1e-20]])
    L *= rng.uniform(0.5, 2.0, (N_FN, 1)).astype(np.float32)     # hdrColor normalises
    xi = rng.uniform(0, 1, (N_FN, 2)).astype(np.float32)
    xi[:4] = np.float32([[0, 0], [1, 1], [0, 1], [1, 0]])
    return L, xi


# ---- the edge sets ------------------------------------------------------------------------------------------------------
def edge_materials():
    """-> ([n, 18], labels).  Each of the ten scalar parameters at 0, 1, -0.0, the smallest normal and a subnormal with the
    others random; base colour black, one channel only, above 1; and plain random rows."""
    rng = np.random.default_rng(101)
    rows, labels = [], []

    def base():
        m = rng.uniform(0.05, 0.95, 18).astype(np.float32)
        m[0:3] = 0.0
        return m
    for k, name in SCALARS.items():
        for v, vn in ((0.0, "0"), (1.0, "1"), (-0.0, "-0"), (TINY_N, "minnormal"), (TINY_S, "subnormal")):
            m = base()
            m[k] = np.float32(v)
            rows.append(m)
            labels.append("%s=%s" % (name, vn))
    for c, cn in (((0, 0, 0), "black"), ((-0.0, -0.0, -0.0), "black-0"), ((0.7, 0, 0), "r-only"), ((0, 0.7, 0), "g-only"),
                  ((0, 0, 0.7), "b-only"), ((2.0, 3.0, 1.5), "above1"), ((TINY_S, TINY_S, TINY_S), "subnormal")):
        m = base()
        m[3:6] = np.float32(c)
        rows.append(m)
        labels.append("baseColor=" + cn)
    m = base()                       # everything the branches test at once
    m[7], m[10], m[14], m[15] = 1.0, 0.0, 0.0, 1.0
    rows.append(m)
    labels.append("metallic=1,roughness=0,clearcoat=0,gloss=1")
    m = base()
    m[7], m[12], m[13] = 1.0, 1.0, 1.0
    rows.append(m)
    labels.append("metallic=1,sheen=1,sheenTint=1")
    for i in range(6):
        rows.append(base())
        labels.append("random%d" % i)
    return np.stack(rows).astype(np.float32), labels


def _nrm(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def edge_vnl():
    """-> ([n, 9] V N L, labels).  N.V and N.L exactly 0 and +- the smallest values that survive normalize (1 + t^2 rounds
    to 1: the vector is its own normalisation), L == V, L == -V (a zero half vector when both graze), N on every axis and on
    either side of getTangent's |N.x| > 0.999 switch, and plain random rows."""
    up = np.float32([0, 1, 0])
    Vg, Lg = np.float32([0, 0.6, 0.8]), np.float32([0.6, 0.8, 0])
    rows, labels = [], []

    def add(label, V, N, L):
        rows.append(np.concatenate([np.float32(V), np.float32(N), np.float32(L)]))
        labels.append(label)
    add("NV=0", [1, 0, 0], up, Lg)
    add("NL=0", Vg, up, [0, 0, 1])
    add("NV=0,NL=0", [1, 0, 0], up, [0, 0, 1])
    for t, tn in ((TINY_S1, "minsub"), (TINY_N, "minnormal")):
        add("NV=+" + tn, [1, t, 0], up, Lg)
        add("NV=-" + tn, [1, -t, 0], up, Lg)
        add("NL=+" + tn, Vg, up, [0, t, 1])
        add("NL=-" + tn, Vg, up, [0, -t, 1])
    add("NV=-0", [1, -0.0, 0], up, Lg)
    add("L==V", Vg, up, Vg)
    add("L==V==N", up, up, up)
    add("L==-V", Vg, up, -Vg)
    add("L==-V,grazing", [1, 0, 0], up, [-1, 0, 0])
    for ax in range(3):
        for sg in (1.0, -1.0):
            N = np.zeros(3, np.float32)
            N[ax] = sg
            o1, o2 = np.zeros(3), np.zeros(3)
            o1[(ax + 1) % 3], o2[(ax + 2) % 3] = 0.5, -0.3
            add("N=%s%s" % ("+" if sg > 0 else "-", "xyz"[ax]), _nrm(N + o1), N, _nrm(N + o2))
    x0 = np.float32(0.999)
    for nx, nn in ((x0, "0.999"), (np.nextafter(x0, np.float32(1)), "0.999+ulp"), (np.nextafter(x0, np.float32(0)), "0.999-ulp"),
                   (-x0, "-0.999"), (-np.nextafter(x0, np.float32(1)), "-0.999-ulp")):
        N = np.float32([nx, np.sqrt(1.0 - float(nx) ** 2), 0])
        add("N.x=" + nn, _nrm(N + np.float32([0, 0, 0.5])), N, _nrm(N + np.float32([0, 0.3, -0.2])))
    rng = np.random.default_rng(102)
    for i, r in enumerate(_vnl(rng, 8)):
        rows.append(r)
        labels.append("random%d" % i)
    return np.stack(rows).astype(np.float32), labels


def edge_xi3():
    """-> ([n, 3], labels): every corner of {0, 1}^3, each component alone at 0 and at 1, and random rows."""
    rng = np.random.default_rng(103)
    rows, labels = [], []
    for c in range(8):
        x = np.float32([(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1])
        rows.append(x)
        labels.append("xi=(%d,%d,%d)" % tuple(x))
    for k in range(3):
        for v in (0.0, 1.0):
            x = rng.uniform(0.05, 0.95, 3).astype(np.float32)
            x[k] = v
            rows.append(x)
            labels.append("xi%d=%d" % (k + 1, v))
    for i in range(6):
        rows.append(rng.uniform(0, 1, 3).astype(np.float32))
        labels.append("random%d" % i)
    return np.stack(rows), labels


def _cross(*sets):
    """Full cross product of (array, labels) sets -> (list of arrays row-aligned, labels joined with ' | ')."""
    sizes = [len(s[1]) for s in sets]
    idx = np.indices(sizes).reshape(len(sets), -1)
    arrays = [np.ascontiguousarray(s[0][i]) for s, i in zip(sets, idx)]
    labels = [" | ".join(s[1][j] for s, j in zip(sets, col)) for col in idx.T]
    return arrays, labels


def edge_evaluate():
    """ops 1, 2, 4: every edge geometry with every edge material -> (a [n, 9], b [n, 18], labels)."""
    (a, b), labels = _cross(edge_vnl(), edge_materials())
    return a, b, labels


def edge_sample_brdf():
    """op 3: every edge xi with the (V, N) of every edge geometry and every edge material -> (a [n, 9], b, labels)."""
    g, gl = edge_vnl()
    (x, vn, b), labels = _cross(edge_xi3(), (g[:, 0:6], gl), edge_materials())
    return np.concatenate([x, vn], 1), b, labels


def edge_hemisphere():
    """op 9: xi corners / single components / random with every edge N -> (a [n, 5], labels)."""
    g, gl = edge_vnl()
    x, xl = edge_xi3()
    (xx, N), labels = _cross((x[:, 0:2], xl), (g[:, 3:6], gl))
    return np.concatenate([xx, N], 1), labels


def edge_env_dirs():
    """ops 5, 7, 10 -> (L [n, 3], labels): both poles, the +-x seam with z = +-1e-20 and +-0, the axes, unnormalised by
    0.5, 2 and 1e10, and the zero vector (normalize gives NaN: the lookups then read texel 0)."""
    base = [("+y", [0, 1, 0]), ("-y", [0, -1, 0]), ("+x", [1, 0, 0]), ("-x", [-1, 0, 0]), ("+z", [0, 0, 1]), ("-z", [0, 0, -1]),
            ("-x,z=+1e-20", [-1, 0, 1e-20]), ("-x,z=-1e-20", [-1, 0, -1e-20]), ("-x,z=-0", [-1, 0, -0.0]),
            ("+x,z=+1e-20", [1, 0, 1e-20]), ("+x,z=-1e-20", [1, 0, -1e-20]),
            ("near+y", [1e-4, 1, 1e-4]), ("near-y", [-1e-4, -1, 1e-4]), ("diag", [0.5, 0.5, -0.7])]
    rows, labels = [], []
    for name, v in base:
        for s in (1.0, 0.5, 2.0, 1e10):
            rows.append(np.float32(v) * np.float32(s))
            labels.append("%s x%g" % (name, s))
    rows.append(np.float32([0, 0, 0]))
    labels.append("zero")
    return np.stack(rows).astype(np.float32), labels


def edge_env_xi(cache):
    """op 6 -> (xi [n, 2], labels): the four corners, each component alone at 0 / 1, texel centres and texel corners (the
    lookup's x.5 and x.0 columns), and the centres of cache texels whose stored x is exactly 0.5 where the cache has such
    (phi = 0: the seam of SampleHdr's own parametrisation)."""
    rng = np.random.default_rng(104)
    rows, labels = [], []
    for c in ((0, 0), (1, 1), (0, 1), (1, 0)):
        rows.append(np.float32(c))
        labels.append("xi=(%d,%d)" % c)
    for k in range(2):
        for v in (0.0, 1.0):
            x = rng.uniform(0.05, 0.95, 2).astype(np.float32)
            x[k] = v
            rows.append(x)
            labels.append("xi%d=%d" % (k + 1, v))
    h, w, _ = cache.shape
    for kx, ky in ((0, 0), (1, 1), (w // 2, h // 2), (w - 1, h - 1), (w // 3, h - 1), (w - 1, h // 3)):
        rows.append(np.float32([(kx + 0.5) / w, (ky + 0.5) / h]))       # x = u W - 0.5 is an integer: fx = fy = 0
        labels.append("texel centre (%d,%d)" % (kx, ky))
        rows.append(np.float32([kx / w, ky / h]))                       # between two texels: fx = fy = 0.5; nearest's floor edge
        labels.append("texel corner (%d,%d)" % (kx, ky))
    ys, xs = np.nonzero(cache[..., 0] == np.float32(0.5))
    pick = np.linspace(0, len(ys) - 1, min(len(ys), 16)).astype(int) if len(ys) else []
    for j in pick:
        rows.append(np.float32([(xs[j] + 0.5) / w, (ys[j] + 0.5) / h]))
        labels.append("cache.x=0.5 at (%d,%d)" % (xs[j], ys[j]))
    return np.stack(rows).astype(np.float32), labels


# ---- which edge rows may be non-finite -------------------------------------------------------------------------------------
# NaN == NaN in same_bits must not hide a failure, so the rows of an edge set whose result is NOT finite are named here, by
# label, with the reason; the tests assert that the oracle's non-finite rows are exactly these.
_ZERO_ROUGHNESS = ("roughness=0", "roughness=-0", "roughness=minnormal", "roughness=subnormal",
                   "metallic=1,roughness=0,clearcoat=0,gloss=1")       # sqr(roughness) == 0 in smithG_GGX
_GRAZING = ("NV=0", "NL=0", "NV=+minsub", "NL=+minsub", "NV=-0")        # a cosine of 0, or so small that its reciprocal is inf


def expected_nonfinite(op, chapter, labels):
    """Boolean per row of the edge set of `op` (labels as the edge_* function returned them)."""
    parts = [l.split(" | ") for l in labels]
    if op == 11:            # ops 1 and 4 of the same row; op 4 is always finite
        return expected_nonfinite(1, 5, labels)
    if op == 12:            # the anisotropic evaluate (op 2 of chapter 4) and its pdf, which max(1e-10, .) keeps finite
        return expected_nonfinite(2, 4, labels)
    if op == 13:            # the diffuse lobe is SampleBRDF's
        return expected_nonfinite(3, 5, labels)
    if op in (1, 2):
        # N.V == N.L == 0: 1 / (NdotL + NdotV) = inf times Fss = 0 in the subsurface term; L == -V grazing passes both sign
        # tests with H = normalize(0) = NaN.  Isotropic body only: smithG_GGX(0, 0) = 1 / (0 + sqrt(0)) = inf meets a zero
        # factor (the anisotropic body clamps its alphas to 0.001, so its G stays finite).
        iso = not (op == 2 and chapter == 4)
        return np.array([g in ("NV=0,NL=0", "L==-V,grazing") or (iso and g in _GRAZING and m in _ZERO_ROUGHNESS) for g, m in parts])
    if op == 3:
        # xi3 = 0 always takes the diffuse lobe; xi1 = xi2 = 1 there: r = 1, theta = 2 PI, and 1 - x*x - y*y with the fp32
        # sin / cos of 2 PI is a small negative number under the square root
        return np.array([p[0] == "xi=(1,1,0)" for p in parts])
    if op in (5, 10):
        return np.array([p[0] == "zero" for p in parts])   # theta = PI * (0.5 - NaN); hdrColor's lookup reads texel 0 instead
    return np.zeros(len(labels), bool)                     # ops 4 (max(1e-10, .) swallows a NaN), 6, 7, 9: always finite


# ---- the quilt: one scene whose triangles carry thousands of materials ------------------------------------------------------
def quilt_materials(n):
    """[n, 18] materials by triangle index from the generator of the function-level sets, arranged so that the builder of the
    device's distinct-material table meets, in every block of 64 triangles: two materials that differ only in the sign of a
    zero (0, 1), two that differ only in the unused IOR / transmission (2, 3), a run of four equal ones (4-7), one that
    re-appears after 40 others (8: the "same as the previous triangle" shortcut must not be the only road to an old row),
    an emitter (9, and 41: ~3 %).  Black base colours, metallic 1, roughness 0 come from the generator's own edge rows."""
    rng = np.random.default_rng(201)
    m = _materials(rng, n)
    m[:, 16:18] = rng.uniform(1.0, 2.0, (n, 2)).astype(np.float32)
    for i in range(n):
        k = i % 64
        if k == 1:
            m[i - 1, 11] = np.float32(0.0)
            m[i] = m[i - 1]
            m[i, 11] = np.float32(-0.0)
        elif k == 3:
            m[i] = m[i - 1]
            m[i, 16:18] = m[i - 1, 16:18] + np.float32(0.25)
        elif 5 <= k <= 7:
            m[i] = m[i - 1]
        elif k == 8 and i >= 40:
            m[i] = m[i - 40]
        elif k in (9, 41):
            m[i, 0:3] = rng.uniform(0.5, 12.0, 3).astype(np.float32)
    return m


def distinct_materials(m18):
    """Number of bitwise distinct rows, and each row's class id."""
    _, inv = np.unique(np.ascontiguousarray(m18, np.float32).view(np.uint32).reshape(len(m18), 18), axis=0, return_inverse=True)
    return int(inv.max()) + 1, inv.reshape(-1)


def quilt_scene(subdiv=0):
    """The Bunny over the floor quad under the shipped map (ezrt_amd.scenes.bunny_scene: host-built SAH tree), every triangle
    re-dressed with quilt_materials by its index in the encoded arrays.  Materials do not enter the tree, so the arrays stay a
    valid scene.  Deterministic: generator and tests rebuild the same arrays."""
    from ezrt_amd import scenes
    bs = scenes.bunny_scene(subdiv=subdiv, hdr="shipped", want_cache=True)
    tri = np.array(bs.tri, np.float32).reshape(-1, 36)
    tri[:, 18:36] = quilt_materials(len(tri))
    bs.tri = np.ascontiguousarray(tri)
    return bs

"""Stream-ordered shading queries (include/ezrt_shade.h, ezrt_amd/shade.py): material, BRDF evaluation and sampling per integrator,
environment lookup and sampling, on device tensors, compared ON THE BITS (a NaN equals a NaN) with the CPU oracle's
ezrt_debug_fn fed the same operands and the materials b = tri36[tri_id, 18:36] -- never with the HIP library's own hook.

The operands are those of the function-level pins (tests/fn_operands.py); the materials are NOT passed in: they come from the
scene's own tables by triangle id -- the quilt scene (5 300 triangles, 4 969 distinct materials) for the random sets, a small scene
whose triangles carry fn_operands.edge_materials() for the edge sets.

NaN == NaN must not hide a failure: on every random set the ORACLE's result may be non-finite in at most 1 % of the rows (measured
with the quilt's materials: 0 of 100 000 rows for every op, test_oracle_nonfinite_share_with_quilt_materials, which runs
without a GPU), and on the edge sets exactly the rows fn_operands.expected_nonfinite names.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fn_operands as F  # noqa: E402

from ezrt_amd import scene as S  # noqa: E402
from ezrt_amd import scenes, trace  # noqa: E402

gpu = pytest.mark.gpu

EZRT_ERR_INVALID = -1
NONFINITE_CAP = 0.01
INTEGRATORS = (3, 4, 50, 51, 52)
f32 = np.float32
PI = f32(3.1415926)                                    # oracle/ezrt_oracle.c: #define PI EZ_PI (include/ezrt_detmath.h)
CONST_PDF = f32(1.0) / (f32(2.0) * PI)                 # its chapter-3/4/5 loop: float pdf = 1.0f / (2.0f * PI);
# integrator -> (operands of its evaluation, the oracle's op and chapter for it); 3 has no op: baseColor / PI
EVAL_CASES = {4: ("uniform", 2, 4), 50: ("iso", 1, 5), 51: ("iso", 11, 5), 52: ("uniform", 12, 5)}
SAMPLE_OPS = {51: 3, 52: 13}                            # integrators 3, 4, 50: op 9 on (xi1, xi2, N)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(torch):
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def shade(torch):
    from ezrt_amd import shade
    return shade


@pytest.fixture(scope="module")
def quilt():
    return F.quilt_scene(0)


@pytest.fixture(scope="module")
def quilt_gpu(hip, quilt):
    return quilt.upload(hip)


@pytest.fixture(scope="module")
def edge_scene():
    """(tri36, nodes, id of every material row of fn_operands.edge_materials() by its bytes): one small triangle per material."""
    mats, _ = F.edge_materials()
    n = len(mats)
    rng = np.random.default_rng(301)
    T = np.zeros((n, 36), f32)
    c = rng.uniform(-2, 2, (n, 1, 3))
    T[:, :9] = (c + rng.uniform(-0.2, 0.2, (n, 3, 3))).reshape(n, 9)
    T[:, 9:18] = np.tile(f32([0, 0, 1]), 3)
    T[:, 18:36] = mats
    hs = S.HostScene()
    hs.addTriangles(np.ascontiguousarray(T))
    hs.buildBVHwithSAH(4)
    tri36, nodes = hs.encode()
    tri36 = np.ascontiguousarray(tri36, f32).reshape(-1, 36)
    ids = {tri36[i, 18:36].tobytes(): i for i in range(len(tri36))}
    assert len(ids) == n == len(tri36)                              # the edge materials are distinct on the bits
    return tri36, nodes, ids


def _edge_ids(edge_scene, b):
    tri36, _, ids = edge_scene
    out = np.array([ids[row.tobytes()] for row in np.ascontiguousarray(b, f32)], np.int32)
    assert F.same_bits(tri36[out, 18:36], b)
    return out


def _quilt_ids(quilt, seed, n=F.N_FN):
    return np.random.default_rng(seed).integers(0, len(quilt.tri), n).astype(np.int32)


def _f(torch, dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, f32)).to(dev)


def _i(torch, dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev)


def _np(torch, *xs):
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in xs)


def _same(name, got, want, a=None, labels=None):
    bad = F.mismatches(got, want)
    if bad.size:
        i = int(bad[0])
        pytest.fail("%s: device != oracle at %d of %d rows; first row %d%s\n operand %r\n device %r\n oracle %r" % (
            name, bad.size, len(want), i, " [%s]" % labels[i] if labels else "", None if a is None else a[i], got[i], want[i]))


def _capped(name, want):
    share = float(F.nonfinite_rows(want).mean())
    print("%s: oracle non-finite share %.5f %% of %d rows (cap 1 %%)" % (name, 100.0 * share, len(want)))
    assert share <= NONFINITE_CAP, "%s: %.3f %% of the oracle's rows are not finite" % (name, 100.0 * share)


def _named(name, want, labels, expect):
    nf = F.nonfinite_rows(want)
    print("%s: oracle non-finite rows %d of %d, all named" % (name, int(nf.sum()), len(want)))
    assert np.array_equal(nf, expect), "%s: non-finite rows are not the named ones: %s" % (
        name, [labels[i] for i in np.flatnonzero(nf != expect)[:8]])


def _eval_operands(kind):
    return (F.evaluate_iso_random() if kind == "iso" else F.evaluate_uniform_random())[0]


def _want_eval(oracle, integ, a, b):
    """(f_r [n, 3], pdf [n]) of integrator `integ` from the oracle, for V N L = a and the materials b."""
    const = np.full(len(a), CONST_PDF, f32)
    if integ == 3:                                       # f_r = vdivs(hit.material.baseColor, PI): three float32 divisions
        return (np.ascontiguousarray(b[:, 3:6], f32) / PI).astype(f32), const
    _, op, ch = EVAL_CASES[integ]
    w = oracle.debug_fn(None, op, ch, a, b)
    return (w[:, 0:3], w[:, 3]) if op in (11, 12) else (w, const)


def _evaluate(torch, shade, dev, sg, ids, a, integ, want_pdf=True, stream=None):
    f, p = shade.evaluate(sg, _i(torch, dev, ids), _f(torch, dev, a[:, 0:3]), _f(torch, dev, a[:, 3:6]), _f(torch, dev, a[:, 6:9]),
                          integrator=integ, want_pdf=want_pdf, stream=stream)
    return _np(torch, f, p)


def _sample(torch, shade, dev, sg, ids, xi, V, N, integ, stream=None):
    return _np(torch, shade.sample(sg, _i(torch, dev, ids), _f(torch, dev, xi), _f(torch, dev, V), _f(torch, dev, N), integrator=integ,
                                   stream=stream))[0]


def _hemisphere_operands(a5):
    """op 9's (xi1, xi2, N) as the sample call's operands: xi3 and V are NaN -- integrators 3, 4, 50 must not read them."""
    nan = np.full((len(a5), 1), np.nan, f32)
    return np.concatenate([a5[:, 0:2], nan], 1), np.full((len(a5), 3), np.nan, f32), a5[:, 2:5]


# ---- the cap on what NaN == NaN may hide: the oracle alone, on the CPU

def test_oracle_nonfinite_share_with_quilt_materials(oracle, quilt):
    """Measured: 0 of 100 000 rows for ops 1, 2 (chapter 4), 11, 12, 3 and 13 with the quilt's materials by seeded random id."""
    m = quilt.tri[:, 18:36]
    for integ, (kind, op, ch) in sorted(EVAL_CASES.items()):
        a = _eval_operands(kind)
        _capped("op %d chapter %d, quilt materials" % (op, ch), oracle.debug_fn(None, op, ch, a, m[_quilt_ids(quilt, 400 + integ)]))
    a = F.sample_brdf_random()[0]
    for integ, op in sorted(SAMPLE_OPS.items()):
        _capped("op %d, quilt materials" % op, oracle.debug_fn(None, op, 5, a, m[_quilt_ids(quilt, 500 + integ)]))
    _capped("op 9", oracle.debug_fn(None, 9, 5, F.hemisphere_random()))


# ---- material

@gpu
def test_material_of_every_quilt_triangle(torch, shade, dev, hip, quilt, quilt_gpu):
    from ezrt_amd import refit
    tri36 = quilt.tri
    n_tri = len(tri36)
    n_distinct, _ = F.distinct_materials(tri36[:, 18:36])
    assert n_tri == 5300 and n_distinct == 4969
    want = np.ascontiguousarray(tri36[:, 18:36])
    assert (np.signbit(want) & (want == 0)).any()                    # a negative zero is among them
    every = np.arange(n_tri, dtype=np.int32)
    rng = np.random.default_rng(11)
    shuffled = np.concatenate([rng.permutation(every), rng.integers(0, n_tri, 3 * n_tri).astype(np.int32), every[::-1]])
    outside = np.array([-1, n_tri, 0, -2, n_tri + 1, np.iinfo(np.int32).max, np.iinfo(np.int32).min, n_tri - 1], np.int32)

    def check(sg, what):
        got, = _np(torch, shade.material(sg, _i(torch, dev, every)))
        assert got.shape == (n_tri, 18) and got.dtype == np.float32
        assert np.array_equal(F.bits(got), F.bits(want)), "%s: %d rows differ" % (what, int((F.bits(got) != F.bits(want)).any(1).sum()))
        got, = _np(torch, shade.material(sg, _i(torch, dev, shuffled)))
        assert np.array_equal(F.bits(got), F.bits(want[shuffled])), what
        got, = _np(torch, shade.material(sg, _i(torch, dev, outside)))
        ok = (outside >= 0) & (outside < n_tri)
        assert np.array_equal(F.bits(got[ok]), F.bits(want[outside[ok]])) and not F.bits(got[~ok]).any(), what

    sg = quilt.upload(hip)
    check(sg, "fresh")
    # a refit rewrites the per-triangle records the material index lives in: the materials stay
    th = 0.6
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float64)
    moved = tri36.copy()
    for k in range(6):
        moved[:, 3 * k:3 * k + 3] = (tri36[:, 3 * k:3 * k + 3].astype(np.float64) @ R.T + (0.3 if k < 3 else 0.0)).astype(f32)
    for what, t2 in (("identity refit", tri36), ("rigid refit", moved)):
        refit.refit(sg, np.ascontiguousarray(t2))
        check(sg, what)


# ---- evaluation and sampling on the random sets, materials from the quilt by triangle id

@gpu
@pytest.mark.parametrize("integ", INTEGRATORS)
def test_evaluate_equals_the_oracle_on_quilt_materials(torch, shade, dev, oracle, quilt, quilt_gpu, integ):
    a = _eval_operands(EVAL_CASES[integ][0] if integ != 3 else "iso")
    ids = _quilt_ids(quilt, 400 + integ)
    b = np.ascontiguousarray(quilt.tri[ids, 18:36])
    assert F.distinct_materials(b)[0] > 4000
    wf, wp = _want_eval(oracle, integ, a, b)
    _capped("integrator %d f_r" % integ, wf)
    _capped("integrator %d pdf" % integ, wp)
    f, p = _evaluate(torch, shade, dev, quilt_gpu, ids, a, integ)
    _same("integrator %d f_r" % integ, f, wf, a)
    _same("integrator %d pdf" % integ, p, wp, a)
    f2, p2 = _evaluate(torch, shade, dev, quilt_gpu, ids, a, integ, want_pdf=False)       # the pdf is optional
    assert p2 is None and F.same_bits(f2, f)
    assert float(np.abs(wf[np.isfinite(wf)]).max()) > 0.1 and float(wp.max()) > 0.1
    if integ != 3:
        assert 0.02 < float((wf == 0).all(1).mean()) < 0.5             # V or L below the horizon: the early return, and mostly not
    if integ in (51, 52):
        assert 0.02 < float((wp == 0).mean()) < 0.5 and np.unique(wp).size > 1000
    else:
        assert (wp == CONST_PDF).all()


@gpu
def test_evaluations_differ_between_integrators_as_the_oracle_says(torch, shade, dev, oracle, quilt, quilt_gpu):
    """One operand set through all five: 4 and 52 share their f_r, 50 and 51 theirs, the two pairs and 3 differ."""
    a = F.evaluate_uniform_random()[0]
    ids = _quilt_ids(quilt, 77)
    got = {k: _evaluate(torch, shade, dev, quilt_gpu, ids, a, k) for k in INTEGRATORS}
    b = np.ascontiguousarray(quilt.tri[ids, 18:36])
    for k, op, ch in ((4, 2, 4), (50, 2, 5), (51, 11, 5), (52, 12, 5)):
        _same("integrator %d" % k, got[k][0], oracle.debug_fn(None, op, ch, a, b)[:, 0:3], a)
    assert F.same_bits(got[4][0], got[52][0]) and F.same_bits(got[50][0], got[51][0])
    assert not F.same_bits(got[4][0], got[50][0]) and not F.same_bits(got[3][0], got[50][0])
    assert not F.same_bits(got[51][1], got[52][1]) and not F.same_bits(got[51][1], got[50][1])


@gpu
@pytest.mark.parametrize("integ", INTEGRATORS)
def test_sample_equals_the_oracle_on_quilt_materials(torch, shade, dev, oracle, quilt, quilt_gpu, integ):
    ids = _quilt_ids(quilt, 500 + integ)
    b = np.ascontiguousarray(quilt.tri[ids, 18:36])
    if integ in SAMPLE_OPS:
        a = F.sample_brdf_random()[0]
        xi, V, N = a[:, 0:3], a[:, 3:6], a[:, 6:9]
        want = oracle.debug_fn(None, SAMPLE_OPS[integ], 5, a, b)
        # all three lobes are chosen (P5/fsh:645-661), in fp32 as the shader decides
        one = f32(1)
        r_d, r_c = one - b[:, 7], f32(0.25) * b[:, 14]
        r_sum = r_d + one + r_c
        p_d, p_s = r_d / r_sum, one / r_sum
        shares = (float((xi[:, 2] <= p_d).mean()), float(((p_d < xi[:, 2]) & (xi[:, 2] <= p_d + p_s)).mean()),
                  float((p_d + p_s < xi[:, 2]).mean()))
        assert all(s > 0.03 for s in shares), shares
    else:
        a = F.hemisphere_random()
        xi, V, N = _hemisphere_operands(a)
        want = oracle.debug_fn(None, 9, 5, a)
    _capped("integrator %d sample" % integ, want)
    got = _sample(torch, shade, dev, quilt_gpu, ids, xi, V, N, integ)
    _same("integrator %d sample" % integ, got, want, a)
    assert float(np.abs(want).max()) > 0.1
    if integ == 52:
        assert not F.same_bits(want, oracle.debug_fn(None, 3, 5, a, b))             # the specular lobe differs from 51's


@gpu
def test_misses_and_ids_beyond_the_scene_give_zeros(torch, shade, dev, oracle, quilt, quilt_gpu):
    n_tri = len(quilt.tri)
    a = F.evaluate_iso_random()[0][:4096]
    s = F.sample_brdf_random()[0][:4096]
    ids = _quilt_ids(quilt, 9, 4096)
    ids[::3] = -1
    ids[1::7] = n_tri
    ids[5::11] = np.iinfo(np.int32).min
    out = (ids < 0) | (ids >= n_tri)
    assert 0.3 < out.mean() < 0.7
    b = np.ascontiguousarray(quilt.tri[np.where(out, 0, ids), 18:36])
    for integ in INTEGRATORS:
        wf, wp = _want_eval(oracle, integ, a, b)
        f, p = _evaluate(torch, shade, dev, quilt_gpu, ids, a, integ)
        _same("integrator %d f_r of the hits" % integ, f[~out], wf[~out])
        _same("integrator %d pdf of the hits" % integ, p[~out], wp[~out])
        assert not F.bits(f[out]).any() and not F.bits(p[out]).any(), integ
        if integ in SAMPLE_OPS:
            xi, V, N = s[:, 0:3], s[:, 3:6], s[:, 6:9]
            want = oracle.debug_fn(None, SAMPLE_OPS[integ], 5, s, b)
        else:
            xi, V, N = _hemisphere_operands(np.concatenate([s[:, 0:2], s[:, 6:9]], 1))
            want = oracle.debug_fn(None, 9, 5, np.concatenate([s[:, 0:2], s[:, 6:9]], 1))
        L = _sample(torch, shade, dev, quilt_gpu, ids, xi, V, N, integ)
        _same("integrator %d sample of the hits" % integ, L[~out], want[~out])
        assert not F.bits(L[out]).any(), integ


# ---- the edge sets: a scene whose triangles carry the edge materials

@gpu
def test_evaluate_and_sample_on_the_edge_sets(torch, shade, dev, hip, oracle, edge_scene):
    tri36, nodes, _ = edge_scene
    sg = hip.scene_create(tri36, nodes)
    a, b, lab = F.edge_evaluate()
    ids = _edge_ids(edge_scene, b)
    for integ, (_, op, ch) in sorted(EVAL_CASES.items()):
        name = "integrator %d (op %d chapter %d) edge" % (integ, op, ch)
        wf, wp = _want_eval(oracle, integ, a, b)
        _named(name, np.concatenate([wf, wp[:, None]], 1), lab, F.expected_nonfinite(op, ch, lab))
        f, p = _evaluate(torch, shade, dev, sg, ids, a, integ)
        _same(name + " f_r", f, wf, a, lab)
        _same(name + " pdf", p, wp, a, lab)
        assert float(np.abs(wf[np.isfinite(wf)]).max()) > 0.1
    wf, wp = _want_eval(oracle, 3, a, b)
    assert np.isfinite(wf).all()                                      # baseColor / PI of finite colours
    f, p = _evaluate(torch, shade, dev, sg, ids, a, 3)
    _same("integrator 3 edge f_r", f, wf, a, lab)
    _same("integrator 3 edge pdf", p, wp, a, lab)
    assert (np.signbit(f) & (f == 0)).any()                          # black-0: -0.0 / PI = -0.0
    a, b, lab = F.edge_sample_brdf()
    ids = _edge_ids(edge_scene, b)
    for integ, op in sorted(SAMPLE_OPS.items()):
        want = oracle.debug_fn(None, op, 5, a, b)
        _named("op %d edge" % op, want, lab, F.expected_nonfinite(op, 5, lab))
        _same("integrator %d sample edge" % integ, _sample(torch, shade, dev, sg, ids, a[:, 0:3], a[:, 3:6], a[:, 6:9], integ), want, a, lab)
        assert float(np.abs(want[np.isfinite(want)]).max()) > 0.1
    a, lab = F.edge_hemisphere()
    want = oracle.debug_fn(None, 9, 5, a)
    _named("op 9 edge", want, lab, F.expected_nonfinite(9, 5, lab))
    xi, V, N = _hemisphere_operands(a)
    ids = (np.arange(len(a)) % len(tri36)).astype(np.int32)
    for integ in (3, 4, 50):
        _same("integrator %d sample edge" % integ, _sample(torch, shade, dev, sg, ids, xi, V, N, integ), want, a, lab)


# ---- environment

def _env_maps():
    shipped = scenes.shipped_hdr()
    return {"shipped": shipped,                                           # exact RGBE form
            "synthetic": scenes.synthetic_hdr(256, 128),
            "not rgbe": (shipped[::4, ::4] * f32(1.0000001) + f32(1e-3)).astype(f32)}


@gpu
@pytest.mark.parametrize("env", ["shipped", "synthetic", "not rgbe"])
def test_env_calls_under_every_layout(torch, shade, dev, hip, oracle, env):
    """hdrColor (clamp 0 and chapter 3's 10), hdrPdf, both at once and SampleHdr on the random and the edge operands, env_rgbe 0/1 x
    env_planes 0/1 x nearest / bilinear: eight device layouts per map against one oracle."""
    bs = scenes.bunny_scene(subdiv=0, hdr=np.ascontiguousarray(_env_maps()[env]), want_cache=True)
    L, xi = F.env_random()
    Le, Llab = F.edge_env_dirs()
    xe, xlab = F.edge_env_xi(bs.cache)
    sg, so = bs.upload(hip), bs.upload(oracle)
    for bil in (1, 0):
        sg.set_env(bs.hdr, bs.cache, bil)
        so.set_env(bs.hdr, bs.cache, bil)
        sets = []
        for tag, dirs, x, dl, xl in (("random", L, xi, None, None), ("edge", Le, xe, Llab, xlab)):
            w = {"pdf": oracle.debug_fn(so, 5, 5, dirs)[:, 0], "sample": oracle.debug_fn(so, 6, 5, x)}
            for clamp, ch in ((0.0, 5), (10.0, 3)):                    # the oracle's hook clamps at 10 in chapter 3 and not elsewhere
                w["colour", clamp] = oracle.debug_fn(so, 7, ch, dirs)
                both = oracle.debug_fn(so, 10, ch, dirs)
                assert F.same_bits(both[:, 0:3], w["colour", clamp]) and F.same_bits(both[:, 3], w["pdf"])   # the fused lookup is the two
            for key, arr in w.items():
                name = "%s %s %s bilinear=%d" % (env, tag, key, bil)
                if tag == "random":
                    _capped(name, arr)
                else:
                    op = 5 if key == "pdf" else 6 if key == "sample" else 7
                    _named(name, arr, xl if key == "sample" else dl, F.expected_nonfinite(op, 5, xl if key == "sample" else dl))
            sets.append((tag, dirs, x, dl, xl, w))
        w = sets[0][5]
        assert float(w["colour", 0.0].max()) > 0.1 and float(w["pdf"].max()) > 0.1 and float(np.abs(w["sample"]).max()) > 0.1
        if env == "shipped":
            assert float(w["colour", 10.0].max()) <= 10.0 < float(w["colour", 0.0].max())   # the clamp bites
        for rgbe in (1, 0):
            for planes in (1, 0):
                sg.set_option("env_rgbe", rgbe)
                sg.set_option("env_planes", planes)
                for tag, dirs, x, dl, xl, w in sets:
                    at = "%s %s bilinear=%d env_rgbe=%d env_planes=%d" % (env, tag, bil, rgbe, planes)
                    dL = _f(torch, dev, dirs)
                    for clamp in (0.0, 10.0):
                        c1, none = shade.env_evaluate(sg, dL, clamp, want_pdf=False)
                        assert none is None
                        c2, p2 = shade.env_evaluate(sg, dL, clamp)
                        c1, c2, p2 = _np(torch, c1, c2, p2)
                        _same(at + " colour alone, clamp %g" % clamp, c1, w["colour", clamp], dirs, dl)
                        _same(at + " colour beside the pdf, clamp %g" % clamp, c2, w["colour", clamp], dirs, dl)
                        _same(at + " pdf beside the colour, clamp %g" % clamp, p2, w["pdf"], dirs, dl)
                    none, p1 = shade.env_evaluate(sg, dL, want_colour=False)
                    assert none is None
                    _same(at + " pdf alone", _np(torch, p1)[0], w["pdf"], dirs, dl)
                    _same(at + " sample", _np(torch, shade.env_sample(sg, _f(torch, dev, x)))[0], w["sample"], x, xl)


# ---- composition: surface -> material -> sample -> evaluate, each stage against the oracle fed the device's own outputs

@gpu
def test_surface_material_sample_evaluate_compose(torch, shade, dev, oracle, quilt, quilt_gpu):
    from ezrt_amd import query
    rng = np.random.default_rng(61)
    n = 200_000
    o = np.tile(f32([0.0, 0.0, 4.0]), (n, 1))
    d = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), -1.5 * np.ones(n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = _f(torch, dev, np.concatenate([o, d], 1))
    xi = _f(torch, dev, rng.uniform(0, 1, (n, 3)))
    r = query.surface(quilt_gpu, rays, integrator=51)
    V = (-rays[:, 3:6]).contiguous()
    m = shade.material(quilt_gpu, r.tri)
    L = shade.sample(quilt_gpu, r.tri, xi, V, r.normal, integrator=51)
    f, p = shade.evaluate(quilt_gpu, r.tri, V, r.normal, L, integrator=51)
    tri, N, m, L, f, p, V, xi = _np(torch, r.tri, r.normal, m, L, f, p, V, xi)
    to, _ = quilt.upload(oracle).query_hits(rays.cpu().numpy())
    assert np.array_equal(tri, to)
    hit = tri >= 0
    assert 0.2 < hit.mean() < 1.0 and np.unique(tri[hit]).size > 1000
    b = np.ascontiguousarray(quilt.tri[tri[hit], 18:36])
    assert np.array_equal(F.bits(m[hit]), F.bits(b)) and not F.bits(m[~hit]).any()
    wantL = oracle.debug_fn(None, 3, 5, np.concatenate([xi, V, N], 1)[hit], b)
    _capped("composition: sampled directions", wantL)
    _same("composition: sample(51) of the surface's own normals", L[hit], wantL)
    want = oracle.debug_fn(None, 11, 5, np.concatenate([V, N, L], 1)[hit], b)
    _capped("composition: evaluation", want)
    _same("composition: f_r of the sampled directions", f[hit], want[:, 0:3])
    _same("composition: pdf of the sampled directions", p[hit], want[:, 3])
    assert not F.bits(L[~hit]).any() and not F.bits(f[~hit]).any() and not F.bits(p[~hit]).any()
    # all three lobes are chosen (P5/fsh:645-661), in fp32 as the shader decides
    one = f32(1)
    r_d, r_c = one - b[:, 7], f32(0.25) * b[:, 14]
    r_sum = r_d + one + r_c
    p_d, p_s = r_d / r_sum, one / r_sum
    x3 = xi[hit, 2]
    shares = (float((x3 <= p_d).mean()), float(((p_d < x3) & (x3 <= p_d + p_s)).mean()), float((p_d + p_s < x3).mean()))
    assert all(s > 0.03 for s in shares), shares
    assert float(want[:, 3].max()) > 0.1 and float(np.abs(want[:, 0:3]).max()) > 0.1 and (want[:, 3] > 0).mean() > 0.25


# ---- plumbing

@gpu
def test_optional_outputs_left_null_are_not_written(torch, dev, hip, oracle, quilt, quilt_gpu):
    n = 5000
    a = F.evaluate_iso_random()[0][:n]
    ids = _quilt_ids(quilt, 3, n)
    b = np.ascontiguousarray(quilt.tri[ids, 18:36])
    P = C.c_void_p
    canary = f32(-7.25)
    tri, V, N, L = _i(torch, dev, ids), _f(torch, dev, a[:, 0:3]), _f(torch, dev, a[:, 3:6]), _f(torch, dev, a[:, 6:9])
    pad = 64
    for integ in INTEGRATORS:
        wf, wp = _want_eval(oracle, integ, a, b)
        for with_pdf in (False, True):
            buf = torch.full((pad + 3 * n + pad + n + pad,), float(canary), device=dev)      # canary | f_r | canary | pdf | canary
            f_ptr, p_ptr = buf.data_ptr() + 4 * pad, buf.data_ptr() + 4 * (pad + 3 * n + pad)
            rc = hip.lib.ezrt_shade_eval_device(quilt_gpu._h, integ, P(tri.data_ptr()), P(V.data_ptr()), P(N.data_ptr()), P(L.data_ptr()), n,
                                                P(f_ptr), P(p_ptr) if with_pdf else None, None)
            assert rc == 0, hip.lib.ezrt_last_error()
            got, = _np(torch, buf)
            _same("integrator %d f_r" % integ, got[pad:pad + 3 * n].reshape(n, 3), wf)
            pdf_area = got[2 * pad + 3 * n:2 * pad + 4 * n]
            if with_pdf:
                _same("integrator %d pdf" % integ, pdf_area, wp)
            else:
                assert (pdf_area == canary).all()
            assert (got[:pad] == canary).all() and (got[pad + 3 * n:2 * pad + 3 * n] == canary).all() and (got[-pad:] == canary).all()
    sg, so = quilt_gpu, quilt.upload(oracle)
    dirs = F.env_random()[0][:n]
    wc, wp = oracle.debug_fn(so, 7, 5, dirs), oracle.debug_fn(so, 5, 5, dirs)[:, 0]
    dL = _f(torch, dev, dirs)
    for mask in (1, 2, 3):
        buf = torch.full((pad + 3 * n + pad + n + pad,), float(canary), device=dev)
        c_ptr, p_ptr = buf.data_ptr() + 4 * pad, buf.data_ptr() + 4 * (pad + 3 * n + pad)
        rc = hip.lib.ezrt_env_eval_device(sg._h, P(dL.data_ptr()), n, 0.0, P(c_ptr) if mask & 1 else None, P(p_ptr) if mask & 2 else None, None)
        assert rc == 0, hip.lib.ezrt_last_error()
        got, = _np(torch, buf)
        col, pdf_area = got[pad:pad + 3 * n], got[2 * pad + 3 * n:2 * pad + 4 * n]
        if mask & 1:
            _same("env colour, mask %d" % mask, col.reshape(n, 3), wc)
        else:
            assert (col == canary).all()
        if mask & 2:
            _same("env pdf, mask %d" % mask, pdf_area, wp)
        else:
            assert (pdf_area == canary).all()
        assert (got[:pad] == canary).all() and (got[pad + 3 * n:2 * pad + 3 * n] == canary).all() and (got[-pad:] == canary).all()


def _all_calls(torch, shade, dev, sg, ops, stream=None):
    """Every call once, integrators 4 and 52, on `stream`: a tuple of device tensors."""
    tri, V, N, L, xi3, dirs, xi2 = ops
    out = [shade.material(sg, tri, stream=stream)]
    for integ in (4, 52):
        out += list(shade.evaluate(sg, tri, V, N, L, integrator=integ, stream=stream))
        out.append(shade.sample(sg, tri, xi3, V, N, integrator=integ, stream=stream))
    out += list(shade.env_evaluate(sg, dirs, 10.0, stream=stream))
    out.append(shade.env_sample(sg, xi2, stream=stream))
    return tuple(out)


def _plumbing_operands(torch, dev, quilt, n, shape=None):
    a = F.evaluate_uniform_random()[0][:n]
    s = F.sample_brdf_random()[0][:n]
    dirs, xi2 = F.env_random()
    ids = _quilt_ids(quilt, 5, n)
    ids[::17] = -1
    ops = [_i(torch, dev, ids), _f(torch, dev, a[:, 0:3]), _f(torch, dev, a[:, 3:6]), _f(torch, dev, a[:, 6:9]), _f(torch, dev, s[:, 0:3]),
           _f(torch, dev, dirs[:n]), _f(torch, dev, xi2[:n])]
    if shape is not None:
        ops = [x.reshape(tuple(shape) + tuple(x.shape[1:])) for x in ops]
    return tuple(ops)


def _same_all(torch, got, want):
    got, want = _np(torch, *got), _np(torch, *want)
    return all(F.same_bits(g.reshape(w.shape), w) for g, w in zip(got, want))


@gpu
def test_streams_leading_dimensions_and_empty_inputs(torch, shade, dev, quilt, quilt_gpu):
    n = 60_000
    ops = _plumbing_operands(torch, dev, quilt, n)
    want = _all_calls(torch, shade, dev, quilt_gpu, ops)
    torch.cuda.synchronize()
    assert all(float(w.abs().max()) > 0.1 for w in want)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    assert _same_all(torch, _all_calls(torch, shade, dev, quilt_gpu, ops, stream=side), want)                 # a torch stream
    assert _same_all(torch, _all_calls(torch, shade, dev, quilt_gpu, ops, stream=side.cuda_stream), want)     # a raw handle
    with torch.cuda.stream(side):                                                                             # the current stream
        torch.cuda._sleep(200_000_000)
        late = _all_calls(torch, shade, dev, quilt_gpu, ops)
        done = side.query()
    assert not done                                                   # returned without waiting: the sleep is still running
    assert _same_all(torch, late, want)
    # leading dimensions are kept
    shaped = _all_calls(torch, shade, dev, quilt_gpu, _plumbing_operands(torch, dev, quilt, n, (20, 50, 60)))
    tails = [(18,), (3,), (), (3,), (3,), (), (3,), (3,), (), (3,)]
    assert [tuple(x.shape) for x in shaped] == [(20, 50, 60) + t for t in tails]
    assert _same_all(torch, shaped, want)
    # n == 0
    e = _all_calls(torch, shade, dev, quilt_gpu, _plumbing_operands(torch, dev, quilt, 0, (4, 0)))
    assert [tuple(x.shape) for x in e] == [(4, 0) + t for t in tails]
    P = C.c_void_p
    lib = quilt_gpu._tl.lib
    t = ops[0]
    assert lib.ezrt_query_material_device(quilt_gpu._h, P(t.data_ptr()), 0, P(ops[1].data_ptr()), None) == 0
    assert lib.ezrt_env_sample_device(quilt_gpu._h, P(ops[6].data_ptr()), 0, P(ops[1].data_ptr()), None) == 0


@gpu
def test_shading_queries_beside_a_render_call(torch, shade, dev, quilt, quilt_gpu):
    cfg = scenes.CONFIGS["C2"]
    eye, cam = S.camera(*cfg["camera"])
    p = trace.make_params(256, 256, eye, cam, 51, cfg["max_bounce"], spp=4, tile=(16, 16))
    sg = quilt_gpu
    ops = _plumbing_operands(torch, dev, quilt, F.N_FN)
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    alone = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sg.render_device(p, alone.data_ptr(), a.cuda_stream)
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms())
    want = _all_calls(torch, shade, dev, sg, ops, stream=b)
    torch.cuda.synchronize()
    assert (sg.counters(), sg.last_render_ms()) == before            # the queries leave counters and timings alone
    frame = torch.zeros((256, 256, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sg.render_device(p, frame.data_ptr(), a.cuda_stream)
    got = _all_calls(torch, shade, dev, sg, ops, stream=b)
    torch.cuda.synchronize()
    assert F.same_bits(frame.cpu().numpy(), alone.cpu().numpy()) and float(alone.abs().max()) > 0.1
    assert _same_all(torch, got, want)


@gpu
def test_errors(torch, shade, dev, hip, oracle, quilt, quilt_gpu, bunny_small):
    sg, lib = quilt_gpu, hip.lib
    n = 1000
    tri, V, N, L, xi3, dirs, xi2 = _plumbing_operands(torch, dev, quilt, n)
    P = C.c_void_p
    o3 = torch.full((n, 3), 3.0, device=dev)
    o1 = torch.full((n,), 3.0, device=dev)
    o18 = torch.full((n, 18), 3.0, device=dev)
    h3, h1, hi = np.full((n, 3), 3.0, f32), np.full(n, 3.0, f32), np.full(n, 5, np.int32)
    h18, h2 = np.full((n, 18), 3.0, f32), np.full((n, 2), 0.5, f32)
    H = lambda x: P(x.ctypes.data)                                    # noqa: E731
    D = lambda x: P(x.data_ptr())                                     # noqa: E731
    first = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def material(s=sg._h, t=D(tri), cnt=n, out=D(o18)):
        return lib.ezrt_query_material_device(s, t, cnt, out, None)

    def evaluate(s=sg._h, integ=51, t=D(tri), v=D(V), nn=D(N), ll=D(L), cnt=n, f=D(o3), pdf=D(o1)):
        return lib.ezrt_shade_eval_device(s, integ, t, v, nn, ll, cnt, f, pdf, None)

    def sample(s=sg._h, integ=51, t=D(tri), x=D(xi3), v=D(V), nn=D(N), cnt=n, out=D(o3)):
        return lib.ezrt_shade_sample_device(s, integ, t, x, v, nn, cnt, out, None)

    def env_eval(s=sg._h, ll=D(dirs), cnt=n, col=D(o3), pdf=D(o1)):
        return lib.ezrt_env_eval_device(s, ll, cnt, 0.0, col, pdf, None)

    def env_sample(s=sg._h, x=D(xi2), cnt=n, out=D(o3)):
        return lib.ezrt_env_sample_device(s, x, cnt, out, None)

    def invalid(rc, what, needle=None):
        assert rc == EZRT_ERR_INVALID, what
        msg = lib.ezrt_last_error()
        assert msg and (needle is None or needle in msg), (what, msg)

    # host memory in any position is rejected, never read or written
    for fn, kws in ((material, ({"t": H(hi)}, {"out": H(h18)})),
                    (evaluate, ({"t": H(hi)}, {"v": H(h3)}, {"nn": H(h3)}, {"ll": H(h3)}, {"f": H(h3)}, {"pdf": H(h1)})),
                    (sample, ({"t": H(hi)}, {"x": H(h3)}, {"v": H(h3)}, {"nn": H(h3)}, {"out": H(h3)})),
                    (env_eval, ({"ll": H(h3)}, {"col": H(h3)}, {"pdf": H(h1)})),
                    (env_sample, ({"x": H(h2)}, {"out": H(h3)}))):
        for kw in kws:
            invalid(fn(**kw), (fn.__name__, sorted(kw)), b"device memory")
    assert (h3 == 3.0).all() and (h1 == 3.0).all() and (h18 == 3.0).all() and (hi == 5).all() and (h2 == 0.5).all()
    # NULL scene or required pointer, both env outputs NULL, n < 0, unknown integrators
    for fn, names in ((material, ("s", "t", "out")), (evaluate, ("s", "t", "v", "nn", "ll", "f")), (sample, ("s", "t", "x", "v", "nn", "out")),
                      (env_eval, ("s", "ll")), (env_sample, ("s", "x", "out"))):
        for name in names:
            invalid(fn(**{name: None}), (fn.__name__, name))
        invalid(fn(cnt=-1), (fn.__name__, "n < 0"))
    invalid(env_eval(col=None, pdf=None), "both env outputs NULL")
    for integ in (0, 1, 2, 5, 49, 53, -1, 1000):
        invalid(evaluate(integ=integ), integ, b"integrator")
        invalid(sample(integ=integ), integ, b"integrator")
    # no environment; an environment without a cache
    bare = hip.scene_create(bunny_small.tri, bunny_small.nodes)
    invalid(env_eval(s=bare._h), "no environment", b"environment")
    invalid(env_sample(s=bare._h), "no environment", b"environment")
    assert material(s=bare._h, t=D(first)) == 0                                              # the material calls need none
    nocache = hip.scene_create(bunny_small.tri, bunny_small.nodes)
    nocache.set_env(bunny_small.hdr, None)
    invalid(env_eval(s=nocache._h), "pdf without a cache", b"cache")
    invalid(env_eval(s=nocache._h, col=None), "pdf without a cache", b"cache")
    invalid(env_sample(s=nocache._h), "sample without a cache", b"cache")
    torch.cuda.synchronize()
    assert (o3.cpu().numpy() == 3.0).all() and (o1.cpu().numpy() == 3.0).all()               # nothing was launched by any of them
    assert env_eval(s=nocache._h, pdf=None) == 0                                             # the colour alone needs no cache
    so = oracle.scene_create(bunny_small.tri, bunny_small.nodes)
    so.set_env(bunny_small.hdr, None)
    assert F.same_bits(_np(torch, o3)[0], oracle.debug_fn(so, 7, 5, dirs.cpu().numpy()))
    # n == 0 is fine and launches nothing
    o3.fill_(3.0)
    assert material(cnt=0) == 0 and evaluate(cnt=0) == 0 and sample(cnt=0) == 0 and env_eval(cnt=0) == 0 and env_sample(cnt=0) == 0
    # the rejected calls left no HIP error behind: the next call works
    got, = _np(torch, shade.material(sg, tri))
    ids = tri.cpu().numpy()
    assert np.array_equal(F.bits(got[ids >= 0]), F.bits(quilt.tri[ids[ids >= 0], 18:36])) and (_np(torch, o3)[0] == 3.0).all()
    # the wrapper: host tensors, other dtypes, other shapes, non-contiguous tensors, other integrators, the oracle's scenes
    for bad in (lambda: shade.material(sg, tri.cpu()), lambda: shade.material(sg, tri.long()), lambda: shade.material(sg, tri.float()),
                lambda: shade.evaluate(sg, tri, V.cpu(), N, L), lambda: shade.evaluate(sg, tri, V.double(), N, L),
                lambda: shade.evaluate(sg, tri, V, N.half(), L), lambda: shade.sample(sg, tri, xi3.double(), V, N),
                lambda: shade.env_evaluate(sg, dirs.double()), lambda: shade.env_sample(sg, xi2.cpu()),
                lambda: shade.material(quilt.upload(oracle), tri), lambda: shade.env_sample(None, xi2)):
        with pytest.raises(TypeError):
            bad()
    wide = torch.zeros((n, 6), device=dev)
    for bad in (lambda: shade.evaluate(sg, tri, V[:-1], N, L), lambda: shade.evaluate(sg, tri, V, N, L[:, :2]),
                lambda: shade.evaluate(sg, tri, wide[:, 0:3], N, L), lambda: shade.material(sg, torch.zeros((n, 2), dtype=torch.int32, device=dev)[:, 0]),
                lambda: shade.sample(sg, tri, xi2, V, N), lambda: shade.sample(sg, tri, xi3, V, wide[:, 3:6]),
                lambda: shade.evaluate(sg, tri, V, N, L, integrator=5), lambda: shade.sample(sg, tri, xi3, V, N, integrator=0),
                lambda: shade.env_evaluate(sg, xi2), lambda: shade.env_evaluate(sg, wide[:, 0:3]), lambda: shade.env_sample(sg, dirs),
                lambda: shade.env_evaluate(sg, dirs, want_colour=False, want_pdf=False)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(trace.TraceError):
        shade.env_sample(bare, xi2)

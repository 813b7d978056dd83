"""Device == oracle, FUNCTION BY FUNCTION, on the bits (a NaN equals a NaN): BRDF_Evaluate of chapters 4 and 5, SampleBRDF,
BRDF_Pdf, the hemisphere sampler, hdrPdf, SampleHdr, hdrColor and the fused hdr_color_pdf, through ezrt_debug_fn
(include/ezrt.h), whose kernel calls the device functions the shading kernels call.

The operands are those of tests/test_ref_fsh_pin.py (tests/fn_operands.py): there the executed shader equals the oracle on
them, here the oracle equals the device.  Materials travel the product's road -- packed into material-table rows on the host by the
function ezrt_scene_create uses, unpacked by the function shade_point uses -- and, second mode, are derived inside the kernel;
both must give the same bits.  The environment ops run under every device layout of the map and its cache.

NaN == NaN must not hide a failure: on the random sets the ORACLE's result may be non-finite in at most 1 % of the rows
(measured: 0 in every set), and on the edge sets exactly the rows fn_operands.expected_nonfinite names.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fn_operands as F  # noqa: E402

from ezrt_amd import scenes, trace  # noqa: E402

pytestmark = pytest.mark.gpu
# cache texels whose stored x is exactly 0.5 (SampleHdr's phi = 0): only the synthetic map's cache has such (256 of them; 16 are
# taken); the shipped map's cache and the cache of the map without an RGBE form have none -- counted, not assumed
CACHE_X_HALF_ROWS = {"shipped": 0, "synthetic": 16, "not rgbe": 0}
NONFINITE_CAP = 0.01


def _same(name, got, want, a, b=None, labels=None):
    bad = F.mismatches(got, want)
    if bad.size:
        i = int(bad[0])
        pytest.fail("%s: device != oracle at %d of %d rows; first row %d%s\n operand %r\n material %r\n device %r\n oracle %r" % (
            name, bad.size, len(want), i, " [%s]" % labels[i] if labels else "", a[i], None if b is None else b[i], got[i], want[i]))


def _capped(name, want):
    share = float(F.nonfinite_rows(want).mean())
    print("%s: oracle non-finite share %.5f %% of %d rows (cap 1 %%)" % (name, 100.0 * share, len(want)))
    assert share <= NONFINITE_CAP, "%s: %.3f %% of the oracle's rows are not finite" % (name, 100.0 * share)


def _named(name, want, labels, expect):
    nf = F.nonfinite_rows(want)
    print("%s: oracle non-finite rows %d of %d, all named" % (name, int(nf.sum()), len(want)))
    assert np.array_equal(nf, expect), "%s: non-finite rows are not the named ones: %s" % (
        name, [labels[i] for i in np.flatnonzero(nf != expect)[:8]])


def _both_modes(hip, oracle, name, op, chapter, a, m, labels=None):
    """Table mode == oracle, inline mode == table mode; returns the oracle's result."""
    want = oracle.debug_fn(None, op, chapter, a, m)
    table = hip.debug_fn(None, op, chapter, a, m)
    inline = hip.debug_fn(None, op, chapter, a, m, inline=True)
    _same(name + " (material table row)", table, want, a, m, labels)
    _same(name + " (derived in the kernel)", inline, want, a, m, labels)
    assert np.array_equal(F.bits(table), F.bits(inline)) or F.same_bits(table, inline)
    return want


def _horizon_shares(a):
    """Shares of rows with V, resp. L (columns 0-2, 6-8) below N's horizon (columns 3-5)."""
    nv = np.einsum("ij,ij->i", a[:, 0:3], a[:, 3:6])
    nl = np.einsum("ij,ij->i", a[:, 6:9], a[:, 3:6])
    return float((nv < 0).mean()), float((nl < 0).mean())


def test_brdf_evaluate_random(hip, oracle):
    a, m = F.evaluate_iso_random()
    w = _both_modes(hip, oracle, "op 1 BRDF_Evaluate", 1, 5, a, m)
    _capped("op 1 random", w)
    assert float(np.abs(w[np.isfinite(w)]).max()) > 0.1
    below = _horizon_shares(a)
    assert all(0.02 < s < 0.3 for s in below), below            # some V / L below the horizon, most above
    assert 0.02 < float((w == 0).all(1).mean()) < 0.5           # ... so the early return is taken, and mostly not
    a, m = F.evaluate_uniform_random()
    w4 = _both_modes(hip, oracle, "op 2 chapter 4 (anisotropic)", 2, 4, a, m)
    w5 = _both_modes(hip, oracle, "op 2 chapter 5 (isotropic body)", 2, 5, a, m)
    _capped("op 2 chapter 4 random", w4)
    _capped("op 2 chapter 5 random", w5)
    assert not F.same_bits(w4, w5) and float(np.abs(w4).max()) > 0.1
    assert F.same_bits(hip.debug_fn(None, 1, 5, a, m), w5)     # Q12: chapter 5's "aniso" IS its isotropic evaluate


def test_fused_evaluate_and_pdf_of_the_mis_loops_random(hip, oracle):
    """brdf_evaluate_pdf<false> / <true>: what integrators 51 / 52 call per evaluated direction (no shading kernel calls
    brdf_pdf alone).  Op 11 must be ops 1 and 4, op 12's colour op 2 of chapter 4; on random directions and on the directions
    the samplers of the same materials return (the use the integrators make of them)."""
    a, m = F.evaluate_iso_random()
    w = _both_modes(hip, oracle, "op 11 fused evaluate + pdf", 11, 5, a, m)
    _capped("op 11 random", w)
    assert F.same_bits(w[:, 0:3], oracle.debug_fn(None, 1, 5, a, m)) and F.same_bits(w[:, 3:4], oracle.debug_fn(None, 4, 5, a, m))
    assert float(np.abs(w[:, 0:3]).max()) > 0.1 and float(w[:, 3].max()) > 0.1 and 0.02 < float((w[:, 3] == 0).mean()) < 0.5
    a, m = F.evaluate_uniform_random()
    w = _both_modes(hip, oracle, "op 12 fused anisotropic evaluate + pdf", 12, 5, a, m)
    _capped("op 12 random", w)
    assert F.same_bits(w[:, 0:3], oracle.debug_fn(None, 2, 4, a, m))
    assert float(np.abs(w[:, 0:3]).max()) > 0.1 and float(w[:, 3].max()) > 0.1 and 0.02 < float((w[:, 3] == 0).mean()) < 0.5
    assert not F.same_bits(w, oracle.debug_fn(None, 11, 5, a, m))
    a, m, vn = F.sample_brdf_random()
    L3 = oracle.debug_fn(None, 3, 5, a, m)
    w = _both_modes(hip, oracle, "op 11 of the sampled directions", 11, 5, np.concatenate([vn[:, 0:6], L3], 1), m)
    _capped("op 11 sampled", w)
    L13 = _both_modes(hip, oracle, "op 13 sample_brdf_aniso", 13, 5, a, m)
    _capped("op 13 random", L13)
    assert float(np.abs(L13).max()) > 0.1 and not F.same_bits(L13, L3) and float((L13 == L3).all(1).mean()) > 0.2   # specular lobe differs
    w = _both_modes(hip, oracle, "op 12 of the directions op 13 sampled", 12, 5, np.concatenate([vn[:, 0:6], L13], 1), m)
    _capped("op 12 sampled", w)
    assert float(w[:, 3].max()) > 0.1


def test_sample_brdf_and_pdf_random(hip, oracle):
    a, m, vn = F.sample_brdf_random()
    w = _both_modes(hip, oracle, "op 3 SampleBRDF", 3, 5, a, m)
    _capped("op 3 random", w)
    # all three lobes are chosen (P5/fsh:645-661), in fp32 as the shader decides
    one = np.float32(1)
    r_d, r_c = one - m[:, 7], np.float32(0.25) * m[:, 14]
    r_sum = r_d + one + r_c
    p_d, p_s = r_d / r_sum, one / r_sum
    rd = a[:, 2]
    shares = (float((rd <= p_d).mean()), float(((p_d < rd) & (rd <= p_d + p_s)).mean()), float((p_d + p_s < rd).mean()))
    assert all(s > 0.03 for s in shares), shares
    assert float(np.abs(w).max()) > 0.1
    a2 = np.concatenate([vn[:, 0:6], w], 1)                     # the pdf of the directions just sampled ...
    w2 = _both_modes(hip, oracle, "op 4 BRDF_Pdf of the sampled directions", 4, 5, a2, m)
    w3 = _both_modes(hip, oracle, "op 4 BRDF_Pdf of random directions", 4, 5, vn, m)   # ... and of random ones
    _capped("op 4 sampled", w2)
    _capped("op 4 random", w3)
    assert float(w2.max()) > 0.1 and float(w3.max()) > 0.1 and 0.02 < float((w3 == 0).mean()) < 0.5


def test_hemisphere_sampling_random(hip, oracle):
    a = F.hemisphere_random()
    want = oracle.debug_fn(None, 9, 5, a)
    _same("op 9 toNormalHemisphere(SampleHemisphere)", hip.debug_fn(None, 9, 5, a), want, a)
    _capped("op 9 random", want)
    assert float(np.abs(want).max()) > 0.1 and int((np.abs(a[:, 2]) > 0.999).sum()) >= 16    # both helper axes of getTangent


def test_brdf_functions_on_the_edge_set(hip, oracle):
    a, m, lab = F.edge_evaluate()
    for op, ch in ((1, 5), (2, 4), (2, 5), (4, 5), (11, 5), (12, 5)):
        name = "op %d chapter %d edge" % (op, ch)
        w = _both_modes(hip, oracle, name, op, ch, a, m, lab)
        _named(name, w, lab, F.expected_nonfinite(op, ch, lab))
        assert float(np.abs(w[np.isfinite(w)]).max()) > 0.1
    a, m, lab = F.edge_sample_brdf()
    w = _both_modes(hip, oracle, "op 3 edge", 3, 5, a, m, lab)
    _named("op 3 edge", w, lab, F.expected_nonfinite(3, 5, lab))
    assert float(np.abs(w[np.isfinite(w)]).max()) > 0.1
    a2 = np.concatenate([a[:, 3:9], w], 1)
    w4 = _both_modes(hip, oracle, "op 4 of op 3's edge directions", 4, 5, a2, m, lab)
    _named("op 4 of op 3's edge directions", w4, lab, F.expected_nonfinite(4, 5, lab))     # NaN directions included: all finite
    assert float(w4.max()) > 0.1
    w = _both_modes(hip, oracle, "op 13 edge", 13, 5, a, m, lab)
    _named("op 13 edge", w, lab, F.expected_nonfinite(13, 5, lab))
    assert float(np.abs(w[np.isfinite(w)]).max()) > 0.1
    a, lab = F.edge_hemisphere()
    want = oracle.debug_fn(None, 9, 5, a)
    _same("op 9 edge", hip.debug_fn(None, 9, 5, a), want, a, None, lab)
    _named("op 9 edge", want, lab, F.expected_nonfinite(9, 5, lab))
    assert float(np.abs(want).max()) > 0.1


def _env_maps():
    shipped = scenes.shipped_hdr()
    return {"shipped": shipped,                                           # exact RGBE form
            "synthetic": scenes.synthetic_hdr(256, 128),
            "not rgbe": (shipped[::4, ::4] * np.float32(1.0000001) + np.float32(1e-3)).astype(np.float32)}


@pytest.mark.parametrize("env", ["shipped", "synthetic", "not rgbe"])
def test_env_functions_under_every_layout(hip, oracle, env):
    """hdrPdf, SampleHdr, hdrColor (chapter 3 clamps at 10) and the fused hdr_color_pdf on the random and the edge operands,
    env_rgbe 0/1 x env_planes 0/1 x nearest / bilinear: eight device layouts per map against one oracle."""
    bs = scenes.bunny_scene(subdiv=0, hdr=np.ascontiguousarray(_env_maps()[env]), want_cache=True)
    L, xi = F.env_random()
    Le, Llab = F.edge_env_dirs()
    xe, xlab = F.edge_env_xi(bs.cache)
    assert sum("texel" in l for l in xlab) == 12
    assert sum("cache.x=0.5" in l for l in xlab) == CACHE_X_HALF_ROWS[env] == min(16, int((bs.cache[..., 0] == np.float32(0.5)).sum()))
    sg, so = bs.upload(hip), bs.upload(oracle)
    for bil in (1, 0):
        sg.set_env(bs.hdr, bs.cache, bil)
        so.set_env(bs.hdr, bs.cache, bil)
        want = {}
        for tag, dirs, x, dl, xl in (("random", L, xi, None, None), ("edge", Le, xe, Llab, xlab)):
            cases = [(5, 5, dirs, dl), (6, 5, x, xl)] + [(7, c, dirs, dl) for c in (3, 4, 5)] + [(10, c, dirs, dl) for c in (3, 4, 5)]
            for op, ch, a, lab in cases:
                w = oracle.debug_fn(so, op, ch, a)
                name = "%s op %d chapter %d %s bilinear=%d" % (env, op, ch, tag, bil)
                if tag == "random":
                    _capped(name, w)
                else:
                    _named(name, w, lab, F.expected_nonfinite(op, ch, lab))
                want[(tag, op, ch)] = (a, lab, w)
            for c in (3, 4, 5):   # the fused lookup is the two separate ones
                w10 = want[(tag, 10, c)][2]
                assert F.same_bits(w10[:, 0:3], want[(tag, 7, c)][2]) and F.same_bits(w10[:, 3:4], want[(tag, 5, 5)][2])
        w7 = want[("random", 7, 4)][2]
        assert float(w7.max()) > 0.1 and float(want[("random", 5, 5)][2].max()) > 0.1
        assert float(np.abs(want[("random", 6, 5)][2]).max()) > 0.1
        if env == "shipped":
            assert float(want[("random", 7, 3)][2].max()) <= 10.0 < float(w7.max())   # chapter 3's clamp bites
        for rgbe in (1, 0):
            for planes in (1, 0):
                sg.set_option("env_rgbe", rgbe)
                sg.set_option("env_planes", planes)
                for (tag, op, ch), (a, lab, w) in want.items():
                    _same("%s op %d chapter %d %s bilinear=%d env_rgbe=%d env_planes=%d" % (env, op, ch, tag, bil, rgbe, planes),
                          hip.debug_fn(sg, op, ch, a), w, a, None, lab)


def test_hook_refuses_what_it_cannot_answer(hip, bunny_small):
    a = np.zeros((4, 9), np.float32)
    with pytest.raises(trace.TraceError):
        hip.debug_fn(None, 8, 5, np.zeros((4, 6), np.float32))       # hitBVH: the surface queries are its audit
    with pytest.raises(trace.TraceError):
        hip.debug_fn(None, 5, 5, np.zeros((4, 3), np.float32))       # env ops need a scene ...
    sg = hip.scene_create(bunny_small.tri, bunny_small.nodes)
    with pytest.raises(trace.TraceError):
        hip.debug_fn(sg, 7, 5, np.zeros((4, 3), np.float32))         # ... with an environment
    with pytest.raises(trace.TraceError):
        hip.debug_fn(None, 1, 5, a)                                   # ops 1-4 need materials
    assert hip.debug_fn(None, 9, 5, np.zeros((0, 5), np.float32)).shape == (0, 3)

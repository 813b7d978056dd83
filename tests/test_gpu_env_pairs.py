"""Bilinear environment lookups through the row-pair plane of the map's RGBE form (knob `env_pairs`; ezrt_device.h tex_fetch_rgbe,
DevScene::hdr_pairs): entry [j][x] holds the texels (row max(j - 1, 0), row min(j, H - 1)) of column x, so the 2 x 2 footprint of a
lookup is one 16-byte load at row (int)y0 + 1 instead of one 8-byte load per row.  The texels taken and the arithmetic on them are
the same, so every bit must be: the device's hdrColor (op 7, chapters 3 and 5: with and without the clamp) and the fused
hdr_color_pdf (op 10) through the function-level audit, with `env_pairs` 1 and 0, against the CPU oracle -- on directions straight up
and down (both clamped rows), on the +-x seam (both clamped columns), a few hundred random ones and ones with NaN components; on
maps of 2 x 2, 4 x 2 and 3 x 5 texels built here (every row pair is an edge pair or next to one) and on the shipped map; and one small
frame of integrators 50 and 51 under both settings.  Nearest filtering keeps its path and is checked with the knob set too.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fn_operands as F  # noqa: E402

from ezrt_amd import scene as S  # noqa: E402
from ezrt_amd import scenes, trace  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_MAPS = {"2x2": (2, 2), "4x2": (4, 2), "3x5": (3, 5)}  # width x height


def _rgbe_map(w, h, seed):
    """[h, w, 3] texels that are exactly (m / 256) 2^(E - 128) per channel with one E per texel and the largest mantissa >= 128: what
    HDRLoader decodes, so the device keeps the 4-byte form; all texels differ, so a wrong row or column shows"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 256, (h, w, 3))
    m[..., 0] = rng.integers(128, 256, (h, w))
    e = rng.integers(120, 134, (h, w, 1))
    return np.ldexp(m.astype(np.float32), e - 136).astype(np.float32)


def _directions():
    """-> (L [n, 3], labels)"""
    Le, lab = F.edge_env_dirs()  # both poles, the +-x seam with z = +-1e-20 and +-0, the axes
    rng = np.random.default_rng(38)
    R = rng.normal(size=(384, 3)).astype(np.float32)
    nan = np.float32("nan")
    N = np.float32([[nan, 0, 1], [0, nan, 1], [1, 0, nan], [nan, nan, nan]])
    return (np.concatenate([Le, R, N]).astype(np.float32),
            list(lab) + ["random %d" % i for i in range(len(R))] + ["NaN x", "NaN y", "NaN z", "NaN xyz"])


def _maps():
    out = {name: _rgbe_map(w, h, 100 + k) for k, (name, (w, h)) in enumerate(SMALL_MAPS.items())}
    out["shipped"] = scenes.shipped_hdr()
    return out


@pytest.mark.parametrize("env", ["2x2", "4x2", "3x5", "shipped"])
def test_lookups_with_and_without_the_pair_plane(hip, oracle, env):
    hdr = np.ascontiguousarray(_maps()[env])
    if env in SMALL_MAPS:
        assert hdr.shape[:2] == SMALL_MAPS[env][::-1] and len(np.unique(hdr.reshape(-1, 3), axis=0)) == hdr.shape[0] * hdr.shape[1]
    bs = scenes.bunny_scene(subdiv=0, hdr=hdr, want_cache=True)
    L, lab = _directions()
    sg, so = bs.upload(hip), bs.upload(oracle)
    for bil in (1, 0):
        sg.set_env(bs.hdr, bs.cache, bil)
        so.set_env(bs.hdr, bs.cache, bil)
        want = {(op, ch): oracle.debug_fn(so, op, ch, L) for op, ch in ((7, 3), (7, 5), (10, 3), (10, 5))}
        w7 = want[(7, 5)]
        assert float(w7[np.isfinite(w7)].max()) > 0.0
        assert F.same_bits(want[(10, 5)][:, 0:3], w7)
        if bil:  # the poles read the clamped rows: the top row's and the bottom row's texels alone
            flat = hdr.reshape(hdr.shape[0], -1)
            for row, pole in ((0, 0), (hdr.shape[0] - 1, 1)):
                assert lab[4 * pole].startswith("+y" if pole == 0 else "-y")
                c = w7[4 * pole]
                assert np.all(c >= flat[row].reshape(-1, 3).min(0)) and np.all(c <= flat[row].reshape(-1, 3).max(0))
        for pairs in (1, 0):
            sg.set_option("env_rgbe", 1)
            sg.set_option("env_pairs", pairs)
            for (op, ch), w in want.items():
                got = hip.debug_fn(sg, op, ch, L)
                bad = F.mismatches(got, w)
                assert bad.size == 0, "%s op %d chapter %d bilinear=%d env_pairs=%d: %d of %d rows differ from the oracle's; first [%s] %r: %r, oracle %r" % (
                    env, op, ch, bil, pairs, bad.size, len(w), lab[int(bad[0])], L[int(bad[0])], got[int(bad[0])], w[int(bad[0])])
        sg.set_option("env_rgbe", 0)  # (the float4 map keeps its path whatever env_pairs says)
        sg.set_option("env_pairs", 1)
        assert F.mismatches(hip.debug_fn(sg, 7, 5, L), w7).size == 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("integ", [50, 51])
def test_frames_under_both_settings(hip, oracle, bunny_small, integ):
    w, h = 64, 32
    eye, cam = S.camera(15, 8, 3.0)
    p = trace.make_params(w, h, eye, cam, integ, 4, spp=3, frame0=5)
    so = bunny_small.upload(oracle)
    so.counters_reset()
    want = so.render(p, np.zeros((h, w, 4), np.float32))
    cw = so.counters()
    assert cw["rays"] > cw["samples"] > 0 and float(want[..., :3].max()) > 0.0
    for pairs in (1, 0):
        sg = bunny_small.upload(hip)
        sg.set_option("env_pairs", pairs)
        sg.counters_reset()
        got = sg.render(p, np.zeros((h, w, 4), np.float32))
        cg = sg.counters()
        same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
        assert bool(same.all()), "integrator %d, env_pairs %d: %d pixels differ from the oracle's" % (integ, pairs, int((~same).any(-1).sum()))
        assert (cg["rays"], cg["samples"]) == (cw["rays"], cw["samples"])

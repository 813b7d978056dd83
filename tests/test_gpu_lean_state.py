"""The slimmed path data between the two big shading stages (ezrt_wavefront.h: LEAN_LIVE).

Integrator 50 hands its state to stage 1 without the s1 array: the sample slot and an "emits" bit ride in the bounce ray direction's
w, the primary hit's triangle in the origin's w.  That may not change a bit of a result: frames are compared with the CPU oracle's
(NaN == NaN), the `rays` and `samples` counters included, over the whole-frame and the general generators of the primary stage, the
redo route (`debug_force_pending`: stage-0 rays through the redo launch, pending paths through the second pass's re-read branch,
emptied slots in the next queue), the audit route (the path log reads the sample slot from its new place), chunked calls, and a scene
whose light is seen directly (the origin's w is read, Le0 is re-read at the path's end).  Integrator 51, whose state is untouched, runs
the same cases: the queues and the hand-over between the stages are shared code.

Bunny at subdiv 0, 4 bounces, 3 spp in one chunk, first frame 5.  Oracle frames are computed once per case and shared.
"""
import re

import numpy as np
import pytest

from ezrt_amd import scene as S
from ezrt_amd import scenes, trace

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # (imported before the HIP library is opened: both then share one HIP runtime)

BOUNCES, SPP, FRAME0 = 4, 3, 5
CAMERA = (15, 8, 3.0)
GENERAL, WHOLE, WHOLE_POW2 = "general", "whole frame", "whole frame, power-of-two"
# (id, width, height, rect / shard of make_params, the generator the call must run)
CASES = (("64x32", 64, 32, {}, WHOLE_POW2),
         ("48x80", 48, 80, {}, WHOLE),
         ("40x24", 40, 24, {}, GENERAL),                                    # not whole 16 x 16 blocks
         ("64x32-rect", 64, 32, dict(rect=(8, 8, 40, 24)), GENERAL),
         ("64x32-shard", 64, 32, dict(shard=(1, 2), tile=(16, 16)), GENERAL))
KEPT = np.float32(7.25)  # what the caller's buffer holds where the call owns no pixel

_oracle_frames = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _params(w, h, integ, spp=SPP, frame0=FRAME0, camera=CAMERA, **kw):
    eye, cam = S.camera(*camera)
    return trace.make_params(w, h, eye, cam, integ, BOUNCES, spp=spp, frame0=frame0, **kw)


def _render(scene, w, h, integ, into=None, **kw):
    """(frame, rays, samples) of one call into a buffer filled with KEPT (or into `into`)"""
    scene.counters_reset()
    img = scene.render(_params(w, h, integ, **kw), np.full((h, w, 4), KEPT, np.float32) if into is None else into)
    c = scene.counters()
    return img, c["rays"], c["samples"]


def _oracle_render(so, key, w, h, integ, **kw):
    if key not in _oracle_frames:
        img, rays, samples = _render(so, w, h, integ, **kw)
        img.setflags(write=False)
        _oracle_frames[key] = (img, rays, samples)
    return _oracle_frames[key]


def _generator(err):
    """which generator the primary stage's launches of the captured calls ran (debug_stages text), all the same one"""
    said = set(re.findall(r"\[ezrt\] primary generator: ([^\n]*)", err))
    assert len(said) == 1, "expected one generator, the library named %r" % sorted(said)
    return said.pop()


def _redone(err):
    """{stage: rays its redo launch re-traced}, summed over the captured calls' chunks (debug_stages text)"""
    out = {}
    for b, n in re.findall(r"\[ezrt\] stage (\d+): (\d+) rays re-traced in reference order", err):
        out[int(b)] = out.get(int(b), 0) + int(n)
    return out


@pytest.fixture(scope="module")
def so(oracle, bunny_small):
    return bunny_small.upload(oracle)


# the schedule whose primary stage generates its rays in the trace launch, set explicitly: the suite also runs with the library's
# defaults overridden through the environment (tools/gpu_suite_routes.sh), and which generator runs is what these tests assert
SCHEDULE = {"wide4": 1, "rel_boxes": 1, "gen_primary": 1, "prune": 2, "gen_whole": 1, "debug_stages": 1}


def _device_scene(hip, built, **options):
    sg = built.upload(hip)
    for k, v in dict(SCHEDULE, **options).items():
        sg.set_option(k, v)
    return sg


def _check(name, got, want):
    (img, r, s), (wimg, rays, samples) = got, want
    assert _same(img, wimg), "%s: %d pixels differ from the oracle's" % (name, int((_bits(img) != _bits(wimg)).any(-1).sum()))
    assert (r, s) == (rays, samples), "%s: rays, samples %r, the oracle %r" % (name, (r, s), (rays, samples))


@pytest.mark.parametrize("integ", [50, 51])
@pytest.mark.parametrize("name,w,h,kw,generator", CASES, ids=[c[0] for c in CASES])
def test_frames_and_counters_are_the_oracles(hip, so, bunny_small, capfd, name, w, h, kw, generator, integ):
    want = _oracle_render(so, (name, integ), w, h, integ, **kw)
    assert want[1] > want[2] > 0
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small), w, h, integ, **kw)
    assert _generator(capfd.readouterr().err) == generator
    _check("%s integrator %d" % (name, integ), got, want)


def test_light_seen_directly(hip, oracle, capfd):
    """cornell_scene(): the primary hit of the light's pixels emits, so those paths carry their triangle (the origin's w) into stage 1
    and re-read Le0 from it when they end"""
    built = scenes.cornell_scene()
    w = h = 32
    cam = (0, 0, 4)
    sc = built.upload(oracle)
    tri, _, _ = sc.render_paths(_params(w, h, 50, spp=1, camera=cam))
    first = tri[..., 0]
    emits = (_bits(built.tri[:, 18:21]) != 0).any(-1)  # per triangle: a set bit in its emission (what tri0 is carried for)
    lit = (first >= 0) & emits[np.clip(first, 0, None)]
    assert lit.sum() > 0, "no pixel sees the light directly: the case would pass without reading a carried triangle"
    assert ((first >= 0) & ~lit).sum() > 0
    want = _render(sc, w, h, 50, camera=cam)
    capfd.readouterr()
    got = _render(_device_scene(hip, built), w, h, 50, camera=cam)
    assert _generator(capfd.readouterr().err) == WHOLE_POW2
    _check("cornell", got, want)
    got = _render(_device_scene(hip, built, debug_force_pending=3), w, h, 50, camera=cam)
    assert _redone(capfd.readouterr().err).get(0, 0) > 0
    _check("cornell, redo route", got, want)


@pytest.mark.parametrize("integ", [50, 51])
@pytest.mark.parametrize("name,w,h,kw,generator", CASES[:2], ids=[c[0] for c in CASES[:2]])
def test_redo_route(hip, so, bunny_small, capfd, name, w, h, kw, generator, integ):
    """debug_force_pending = 3: every third ray slot of a 4-wide launch goes to the redo list and its path through the second pass's
    re-read branch, at stages 0 and 1; a pending path that left the scene leaves an empty slot (all zeros) in the next queue"""
    want = _oracle_render(so, (name, integ), w, h, integ, **kw)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, debug_force_pending=3), w, h, integ, **kw)
    err = capfd.readouterr().err
    assert _generator(err) == generator
    redone = _redone(err)
    assert redone.get(0, 0) > 0 and redone.get(1, 0) > 0, "redo launches re-traced %r" % redone
    _check("%s integrator %d, redo route" % (name, integ), got, want)


def test_audit_route(hip, so, bunny_small, capfd):
    """render_paths through the timed kernels: the path log finds every path's pixel through the sample slot the state carries"""
    w, h = 64, 32
    p = _params(w, h, 50, spp=1)
    capfd.readouterr()
    tri1, t1, col1 = _device_scene(hip, bunny_small, audit_via_queue=1).render_paths(p)
    assert _generator(capfd.readouterr().err) == WHOLE_POW2
    tri_o, t_o, col_o = so.render_paths(p)
    assert (tri_o[..., 2] >= -1).sum() > 0 and (tri_o[..., 4] >= 0).sum() > 0  # (paths reach the later stages, and hit there)
    assert np.array_equal(tri1, tri_o) and np.array_equal(_bits(t1), _bits(t_o)) and _same(col1, col_o)


@pytest.mark.parametrize("integ", [50, 51])
def test_chunked_calls(hip, so, bunny_small, capfd, integ):
    """the same frame as two chunks of one call (chunk_log2 12: 2 frames of 64 x 32 in flight), and as two calls, the second with
    frame0 > 0: the bits of the one-chunk frame"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", integ), w, h, integ)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, chunk_log2=12), w, h, integ)
    assert len(re.findall(r"\[ezrt\] primary generator", capfd.readouterr().err)) == 2  # (two chunks)
    _check("two chunks, integrator %d" % integ, got, want)
    sg = _device_scene(hip, bunny_small)
    sg.counters_reset()
    part = sg.render(_params(w, h, integ, spp=1, frame0=FRAME0), np.full((h, w, 4), KEPT, np.float32))
    part = sg.render(_params(w, h, integ, spp=SPP - 1, frame0=FRAME0 + 1), part)
    c = sg.counters()
    _check("two calls, integrator %d" % integ, (part, c["rays"], c["samples"]), want)

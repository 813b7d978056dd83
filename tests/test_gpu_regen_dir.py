"""The primary stage's shading passes generate a ray's direction again instead of reading it from the queue (knob `regen_dir`;
ezrt_wavefront.h shade_load REGEN, ezrt_traceq4.h WHOLE == 3).

A call that renders a whole frame whose width and height are powers of two, with integrator 50, 51 or 52, runs a primary trace launch
that stores no directions and two shading passes that compute them from the queue position with the launch's own generator.  Only a
ray handed to the redo list has its direction stored, by the lane that hands it over.  Every other call -- another frame shape, a
rect, a shard, the audit route -- and `regen_dir = 0` keep the stored directions.  None of this may change a bit: frames are compared
with the CPU oracle's and with each other (NaN == NaN), the `rays` and `samples` counters included, and which route ran is read from
the `debug_stages` text.

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
OTHER_CAMERA = (-40, 20, 2.5)
REGENERATED, STORED = "regenerated", "stored"
# (id, width, height, rect / shard of make_params): calls that are no whole power-of-two frame keep the stored directions
STORED_CASES = (("48x80", 48, 80, {}),
                ("64x48", 64, 48, {}),                                      # one power of two
                ("40x24", 40, 24, {}),                                      # not whole 16 x 16 blocks
                ("64x32-rect", 64, 32, dict(rect=(8, 8, 40, 24))),
                ("64x32-shard", 64, 32, dict(shard=(1, 2), tile=(16, 16))))
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


def _route(err):
    """which route the primary stage's passes of the captured calls took (debug_stages text), all the same one"""
    said = set(re.findall(r"\[ezrt\] primary directions: ([^\n]*)", err))
    assert len(said) == 1, "expected one route, the library named %r" % sorted(said)
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
# defaults overridden through the environment (tools/gpu_suite_routes.sh), and which route runs is what these tests assert
SCHEDULE = {"wide4": 1, "rel_boxes": 1, "gen_primary": 1, "prune": 2, "gen_whole": 1, "regen_dir": 1, "debug_stages": 1}


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
def test_both_routes_are_the_oracles(hip, so, bunny_small, capfd, integ):
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", integ), w, h, integ)
    assert want[1] > want[2] > 0
    capfd.readouterr()
    got1 = _render(_device_scene(hip, bunny_small), w, h, integ)
    ran1 = _route(capfd.readouterr().err)
    got0 = _render(_device_scene(hip, bunny_small, regen_dir=0), w, h, integ)
    ran0 = _route(capfd.readouterr().err)
    assert (ran1, ran0) == (REGENERATED, STORED)
    _check("integrator %d, regen_dir 1" % integ, got1, want)
    _check("integrator %d, regen_dir 0" % integ, got0, want)
    assert _same(got1[0], got0[0])


@pytest.mark.parametrize("name,w,h,kw", STORED_CASES, ids=[c[0] for c in STORED_CASES])
def test_other_calls_keep_the_stored_directions(hip, so, bunny_small, capfd, name, w, h, kw):
    want = _oracle_render(so, (name, 50), w, h, 50, **kw)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small), w, h, 50, **kw)
    assert _route(capfd.readouterr().err) == STORED
    _check(name, got, want)


@pytest.mark.parametrize("integ", [50, 51])
def test_redo_route(hip, so, bunny_small, capfd, integ):
    """debug_force_pending = 3: every third primary ray goes to the redo list, whose launch reads the ray's direction from the queue --
    where only the lane that handed the ray over can have put it"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", integ), w, h, integ)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, debug_force_pending=3), w, h, integ)
    err = capfd.readouterr().err
    assert _route(err) == REGENERATED
    assert _redone(err).get(0, 0) > 0, "redo launches re-traced %r" % _redone(err)
    _check("integrator %d, redo route" % integ, got, want)


def test_redo_route_after_another_camera(hip, so, bunny_small, capfd):
    """the same on a scene whose scratch sets hold another camera's directions, stored (regen_dir 0) by two earlier calls -- consecutive
    chunks alternate between the two sets --: a pass or a redo launch that read a slot nobody wrote in this call would shade that ray"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", 50), w, h, 50)
    sg = _device_scene(hip, bunny_small, regen_dir=0)
    stale = [_render(sg, w, h, 50, camera=OTHER_CAMERA)[0] for _ in range(2)]
    assert not _same(stale[0], want[0])
    sg.set_option("regen_dir", 1)
    for pending in (3, 0):
        sg.set_option("debug_force_pending", pending)
        capfd.readouterr()
        got = _render(sg, w, h, 50)
        err = capfd.readouterr().err
        assert _route(err) == REGENERATED
        assert (_redone(err).get(0, 0) > 0) == (pending > 0)
        _check("after another camera, debug_force_pending %d" % pending, got, want)


def test_light_seen_directly(hip, oracle, capfd):
    """cornell_scene(): the primary hit of the light's pixels emits, so tri0 and Le0 of the second pass take part"""
    built = scenes.cornell_scene()
    w = h = 32
    cam = (0, 0, 4)
    sc = built.upload(oracle)
    tri, _, _ = sc.render_paths(_params(w, h, 50, spp=1, camera=cam))
    first = tri[..., 0]
    emits = (_bits(built.tri[:, 18:21]) != 0).any(-1)  # per triangle: a set bit in its emission
    lit = (first >= 0) & emits[np.clip(first, 0, None)]
    assert lit.sum() > 0, "no pixel sees the light directly"
    want = _render(sc, w, h, 50, camera=cam)
    capfd.readouterr()
    got = _render(_device_scene(hip, built), w, h, 50, camera=cam)
    assert _route(capfd.readouterr().err) == REGENERATED
    _check("cornell", got, want)


@pytest.mark.parametrize("integ", [50, 51])
def test_chunked_calls(hip, so, bunny_small, capfd, integ):
    """the same frame as two chunks of one call (chunk_log2 12: 2 frames of 64 x 32 in flight), and as two calls into one buffer with
    frame0 0 and 3: the bits of the one-chunk frames"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", integ), w, h, integ)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, chunk_log2=12), w, h, integ)
    err = capfd.readouterr().err
    assert len(re.findall(r"\[ezrt\] primary directions", err)) == 2 and _route(err) == REGENERATED  # (two chunks)
    _check("two chunks, integrator %d" % integ, got, want)
    key = ("64x32-two-calls", integ)
    if key not in _oracle_frames:
        so.counters_reset()
        part = so.render(_params(w, h, integ, spp=3, frame0=0), np.full((h, w, 4), KEPT, np.float32))
        part = so.render(_params(w, h, integ, spp=2, frame0=3), part)
        c = so.counters()
        part.setflags(write=False)
        _oracle_frames[key] = (part, c["rays"], c["samples"])
    sg = _device_scene(hip, bunny_small)
    sg.counters_reset()
    part = sg.render(_params(w, h, integ, spp=3, frame0=0), np.full((h, w, 4), KEPT, np.float32))
    part = sg.render(_params(w, h, integ, spp=2, frame0=3), part)
    c = sg.counters()
    assert _route(capfd.readouterr().err) == REGENERATED
    _check("two calls, integrator %d" % integ, (part, c["rays"], c["samples"]), _oracle_frames[key])


def test_audit_route_keeps_the_stored_directions(hip, so, bunny_small, capfd):
    """render_paths through the timed kernels: the path log's route reads the queue, so it must report the stored route, and agree
    with the oracle's log"""
    w, h = 64, 32
    p = _params(w, h, 50, spp=1)
    capfd.readouterr()
    tri1, t1, col1 = _device_scene(hip, bunny_small, audit_via_queue=1).render_paths(p)
    assert _route(capfd.readouterr().err) == STORED
    tri_o, t_o, col_o = so.render_paths(p)
    assert (tri_o[..., 2] >= -1).sum() > 0 and (tri_o[..., 4] >= 0).sum() > 0  # (paths reach the later stages, and hit there)
    assert np.array_equal(tri1, tri_o) and np.array_equal(_bits(t1), _bits(t_o)) and _same(col1, col_o)

"""The primary trace launch generates a ray where a lane ADOPTS its queue position, not where the position is drawn (ezrt_traceq4.h,
the GEN instances: a drawn position is kept as a slot number alone), and the primary stage's regenerating shading passes take the
pixel, the frame and the sample slot from the generator's own arithmetic (ezrt_wavefront.h shade_body REGEN).  Neither may change a
bit: frames are compared with the CPU oracle's on the bits (NaN == NaN), the `rays` and `samples` counters included, for every
generator instance -- which one ran is read from the `debug_stages` text:

  64 x 32                     whole frame, power of two; directions regenerated (WHOLE 3: no store)
  64 x 32, regen_dir = 0      whole frame, power of two; directions stored, at adoption (WHOLE 2)
  48 x 80, 64 x 48            whole frame (WHOLE 1)
  40 x 24, a rect, a shard    the general generator, with slots of pixels the call does not own (WHOLE 0): nobody traces them, and
                              `rays` counts the owned ones alone

These frames hold fewer rays than the launch has lanes, so the queue runs out while lanes still hold drawn slots: idle lanes take
them over (the hand-over) and generate them.  With debug_force_pending the redo launch reads the directions from the queue, where
they must be by then.

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
POW2, WHOLE, GENERAL = "whole frame, power-of-two", "whole frame", "general"
REGENERATED, STORED = "regenerated", "stored"
# (id, width, height, options, rect / shard of make_params, generator, directions)
CASES = (("64x32", 64, 32, {}, {}, POW2, REGENERATED),
         ("64x32-stored", 64, 32, {"regen_dir": 0}, {}, POW2, STORED),
         ("48x80", 48, 80, {}, {}, WHOLE, STORED),
         ("64x48", 64, 48, {}, {}, WHOLE, STORED),
         ("40x24", 40, 24, {}, {}, GENERAL, STORED),
         ("64x32-rect", 64, 32, {}, dict(rect=(8, 8, 40, 24)), GENERAL, STORED),
         ("64x32-shard", 64, 32, {}, dict(shard=(1, 2), tile=(16, 16)), GENERAL, STORED))
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
    """(generator, directions) the primary stage of the captured calls ran with (debug_stages text), all the same"""
    gen = set(re.findall(r"\[ezrt\] primary generator: ([^\n]*)", err))
    dirs = set(re.findall(r"\[ezrt\] primary directions: ([^\n]*)", err))
    assert len(gen) == 1 and len(dirs) == 1, "expected one route, the library named %r, %r" % (sorted(gen), sorted(dirs))
    return gen.pop(), dirs.pop()


def _redone(err):
    """{stage: rays its redo launch re-traced}, summed over the captured calls' chunks (debug_stages text)"""
    out = {}
    for b, n in re.findall(r"\[ezrt\] stage (\d+): (\d+) rays re-traced in reference order", err):
        out[int(b)] = out.get(int(b), 0) + int(n)
    return out


@pytest.fixture(scope="module")
def so(oracle, bunny_small):
    return bunny_small.upload(oracle)


# the schedule whose primary stage generates its rays in the trace launch, set explicitly: which instance runs is what these tests assert
SCHEDULE = {"wide4": 1, "rel_boxes": 1, "gen_primary": 1, "prune": 2, "gen_whole": 1, "regen_dir": 1, "steal": 1, "handover": 1,
            "debug_stages": 1}


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
@pytest.mark.parametrize("name,w,h,options,kw,generator,directions", CASES, ids=[c[0] for c in CASES])
def test_every_generator_instance(hip, so, bunny_small, capfd, name, w, h, options, kw, generator, directions, integ):
    want = _oracle_render(so, (name.replace("-stored", ""), integ), w, h, integ, **kw)
    assert want[1] > want[2] > 0
    if generator == GENERAL and kw:  # (slots of pixels the call does not own: fewer samples than the frame has)
        assert want[2] < w * h * SPP and bool((want[0] == KEPT).all(-1).any())
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, **options), w, h, integ, **kw)
    assert _route(capfd.readouterr().err) == (generator, directions)
    _check("%s, integrator %d" % (name, integ), got, want)


REDO_CASES = tuple(c for c in CASES if c[0] in ("64x32", "64x32-stored", "48x80", "64x32-shard"))


@pytest.mark.parametrize("integ", [50, 51])
@pytest.mark.parametrize("name,w,h,options,kw,generator,directions", REDO_CASES, ids=[c[0] for c in REDO_CASES])
def test_redo_launch_finds_the_direction_in_the_queue(hip, so, bunny_small, capfd, name, w, h, options, kw, generator, directions, integ):
    """debug_force_pending = 3: every third primary ray goes to the redo list, whose launch reads the ray's direction from the queue --
    stored there when the slot was adopted, or (no store: WHOLE 3) by the lane that hands the ray over"""
    want = _oracle_render(so, (name.replace("-stored", ""), integ), w, h, integ, **kw)
    capfd.readouterr()
    got = _render(_device_scene(hip, bunny_small, debug_force_pending=3, **options), w, h, integ, **kw)
    err = capfd.readouterr().err
    assert _route(err) == (generator, directions)
    assert _redone(err).get(0, 0) > 0, "redo launches re-traced %r" % _redone(err)
    _check("%s, integrator %d, redo route" % (name, integ), got, want)


@pytest.mark.parametrize("regen", [1, 0])
def test_redo_route_after_another_camera(hip, so, bunny_small, capfd, regen):
    """the same on a scene whose scratch sets hold another camera's directions, stored by two earlier calls -- consecutive chunks
    alternate between the two sets --: a pass or a redo launch that read a slot nobody wrote in this call would shade that ray"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", 50), w, h, 50)
    sg = _device_scene(hip, bunny_small, regen_dir=0)
    stale = [_render(sg, w, h, 50, camera=OTHER_CAMERA)[0] for _ in range(2)]
    assert not _same(stale[0], want[0])
    sg.set_option("regen_dir", regen)
    for pending in (3, 0):
        sg.set_option("debug_force_pending", pending)
        capfd.readouterr()
        got = _render(sg, w, h, 50)
        err = capfd.readouterr().err
        assert _route(err) == (POW2, REGENERATED if regen else STORED)
        assert (_redone(err).get(0, 0) > 0) == (pending > 0)
        _check("after another camera, regen_dir %d, debug_force_pending %d" % (regen, pending), got, want)


@pytest.mark.parametrize("integ", [50, 51])
def test_chunked_calls(hip, so, bunny_small, capfd, integ):
    """the same frame as two chunks of one call (chunk_log2 12: 2 frames of 64 x 32 in flight), and as two calls into one buffer with
    frame0 0 and 3: the bits of the one-chunk frames"""
    w, h = 64, 32
    want = _oracle_render(so, ("64x32", integ), w, h, integ)
    for regen in (1, 0):
        capfd.readouterr()
        got = _render(_device_scene(hip, bunny_small, chunk_log2=12, regen_dir=regen), w, h, integ)
        err = capfd.readouterr().err
        assert len(re.findall(r"\[ezrt\] primary directions", err)) == 2  # (two chunks)
        assert _route(err) == (POW2, REGENERATED if regen else STORED)
        _check("two chunks, integrator %d, regen_dir %d" % (integ, regen), got, want)
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
    assert _route(capfd.readouterr().err) == (POW2, REGENERATED)
    _check("two calls, integrator %d" % integ, (part, c["rays"], c["samples"]), _oracle_frames[key])


def test_light_seen_directly(hip, oracle, capfd):
    """cornell_scene() at 32 x 32: the primary hit of the light's pixels emits, so tri0 and Le0 of the second pass take part"""
    built = scenes.cornell_scene()
    w = h = 32
    cam = (0, 0, 4)
    sc = built.upload(oracle)
    want = _render(sc, w, h, 50, camera=cam)
    assert float(want[0][..., :3].max()) > 0.0
    capfd.readouterr()
    got = _render(_device_scene(hip, built), w, h, 50, camera=cam)
    assert _route(capfd.readouterr().err) == (POW2, REGENERATED)
    _check("cornell", got, want)


def test_path_log_through_the_timed_kernels(hip, so, bunny_small, capfd):
    """render_paths through the timed kernels (audit_via_queue): the path log reads the queue, so the launch stores the directions --
    at adoption -- and the log must be the oracle's"""
    w, h = 64, 32
    p = _params(w, h, 50, spp=1)
    capfd.readouterr()
    tri1, t1, col1 = _device_scene(hip, bunny_small, audit_via_queue=1).render_paths(p)
    assert _route(capfd.readouterr().err) == (POW2, STORED)
    tri_o, t_o, col_o = so.render_paths(p)
    assert (tri_o[..., 2] >= -1).sum() > 0 and (tri_o[..., 4] >= 0).sum() > 0  # (paths reach the later stages, and hit there)
    assert np.array_equal(tri1, tri_o) and np.array_equal(_bits(t1), _bits(t_o)) and _same(col1, col_o)

"""The whole-frame ray generators of the primary stage's trace kernel (traceq4_kernel WHOLE; ezrt_kernels.h primary_dir_whole).

A call that renders a whole frame -- one shard, the full rectangle, width and height multiples of 16 -- runs an instance whose generator
finds a queue position's pixel by arithmetic (no ownership test, no load from the block list) and, when width and height are powers
of two, multiplies by their exact reciprocals instead of dividing.  Every other call keeps the general generator, and the knob
`gen_whole = 0` keeps it everywhere.  The three must give the same bits: frames are compared with the CPU oracle's and with each
other (NaN == NaN), ray and sample counters included, and which generator ran is read from the `debug_stages` text.

Bunny at subdiv 0, integrator 50, 2 bounces, 3 spp in one chunk, first frame 5.  Oracle frames are computed once per case and shared.
"""
import re

import numpy as np
import pytest

from ezrt_amd import scene as S
from ezrt_amd import trace

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # (imported before the HIP library is opened: both then share one HIP runtime)

INTEG, BOUNCES, SPP, FRAME0 = 50, 2, 3, 5
CAMERA = (15, 8, 3.0)
GENERAL, WHOLE, WHOLE_POW2 = "general", "whole frame", "whole frame, power-of-two"
# (id, width, height, rect / shard of make_params, the generator the call must run)
CASES = (("64x32", 64, 32, {}, WHOLE_POW2),
         ("48x80", 48, 80, {}, WHOLE),
         ("64x48", 64, 48, {}, WHOLE),                                      # one power of two: the true divisions
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


def _params(w, h, spp=SPP, frame0=FRAME0, **kw):
    eye, cam = S.camera(*CAMERA)
    return trace.make_params(w, h, eye, cam, INTEG, BOUNCES, spp=spp, frame0=frame0, **kw)


def _render(scene, w, h, **kw):
    """(frame, rays, samples) of one call into a buffer filled with KEPT"""
    scene.counters_reset()
    img = scene.render(_params(w, h, **kw), np.full((h, w, 4), KEPT, np.float32))
    c = scene.counters()
    return img, c["rays"], c["samples"]


def _oracle_render(so, key, w, h, **kw):
    if key not in _oracle_frames:
        img, rays, samples = _render(so, w, h, **kw)
        img.setflags(write=False)
        _oracle_frames[key] = (img, rays, samples)
    return _oracle_frames[key]


def _generator(err):
    """which generator the primary stage's launches of the captured calls ran (debug_stages text), all the same one"""
    said = set(re.findall(r"\[ezrt\] primary generator: ([^\n]*)", err))
    assert len(said) == 1, "expected one generator, the library named %r" % sorted(said)
    return said.pop()


@pytest.fixture(scope="module")
def so(oracle, bunny_small):
    return bunny_small.upload(oracle)


# the schedule whose primary stage generates its rays in the trace launch, set explicitly: the suite also runs with the library's
# defaults overridden through the environment (tools/gpu_suite_routes.sh), and which generator runs is what these tests assert
SCHEDULE = {"wide4": 1, "rel_boxes": 1, "gen_primary": 1, "prune": 2, "gen_whole": 1, "debug_stages": 1}


def _device_scene(hip, bunny_small, **options):
    sg = bunny_small.upload(hip)
    for k, v in dict(SCHEDULE, **options).items():
        sg.set_option(k, v)
    return sg


@pytest.mark.parametrize("name,w,h,kw,generator", CASES, ids=[c[0] for c in CASES])
def test_generators_agree_with_each_other_and_the_oracle(hip, so, bunny_small, capfd, name, w, h, kw, generator):
    want, rays, samples = _oracle_render(so, name, w, h, **kw)
    assert rays > samples > 0
    capfd.readouterr()
    got1 = _render(_device_scene(hip, bunny_small), w, h, **kw)
    ran1 = _generator(capfd.readouterr().err)
    got0 = _render(_device_scene(hip, bunny_small, gen_whole=0), w, h, **kw)
    ran0 = _generator(capfd.readouterr().err)
    assert ran1 == generator and ran0 == GENERAL
    for what, (img, r, s) in (("gen_whole 1", got1), ("gen_whole 0", got0)):
        assert _same(img, want), "%s %s: %d pixels differ from the oracle's" % (name, what, int((_bits(img) != _bits(want)).any(-1).sum()))
        assert (r, s) == (rays, samples), "%s %s: rays, samples %r, the oracle %r" % (name, what, (r, s), (rays, samples))
    assert _same(got1[0], got0[0])


@pytest.mark.parametrize("w,h,spp", [(16, 16, 1), (512, 16, SPP)], ids=["one-block", "one-block-row"])
def test_smallest_whole_frames(hip, so, bunny_small, capfd, w, h, spp):
    """one block at 1 spp -- fewer rays than waves in the launch, one scatter granule set -- and a single row of 32 blocks"""
    want, rays, samples = _oracle_render(so, (w, h, spp), w, h, spp=spp)
    capfd.readouterr()
    img, r, s = _render(_device_scene(hip, bunny_small), w, h, spp=spp)
    assert _generator(capfd.readouterr().err) == WHOLE_POW2
    assert _same(img, want) and (r, s) == (rays, samples)


def test_camera_rays_are_the_power_of_two_generators(hip, so, bunny_small, capfd):
    """ezrt_camera_rays_device divides by width and height; the power-of-two generator multiplies by their reciprocals.  The rays a
    caller is handed, traced by the oracle, give the hit records the primary stage leaves (path log through the timed kernels),
    on the bits; and the records of every stage are the same with gen_whole 0 and 1."""
    from ezrt_amd import path
    w, h = 64, 32
    p = _params(w, h, spp=1)
    sg = _device_scene(hip, bunny_small, audit_via_queue=1)
    ys, xs = np.mgrid[0:h, 0:w]
    xyf = np.stack([xs.ravel(), ys.ravel(), np.full(w * h, FRAME0)], 1).astype(np.uint32)
    dx = torch.from_numpy(xyf.view(np.int32)).to(torch.device("cuda", 0)).view(torch.uint32)
    rays = path.camera_rays(sg, p, dx)
    torch.cuda.synchronize()
    tri_o, t_o = so.query_hits(rays.cpu().numpy())
    capfd.readouterr()
    tri1, t1, col1 = sg.render_paths(p)
    assert _generator(capfd.readouterr().err) == WHOLE_POW2
    tri0, t0, col0 = _device_scene(hip, bunny_small, audit_via_queue=1, gen_whole=0).render_paths(p)
    assert _generator(capfd.readouterr().err) == GENERAL
    hit = tri_o >= 0
    assert 0.2 < hit.mean() < 1.0
    assert np.array_equal(tri1[..., 0].ravel(), tri_o), "%d primary hit ids differ" % int((tri1[..., 0].ravel() != tri_o).sum())
    assert np.array_equal(_bits(t1[..., 0].ravel()[hit]), _bits(t_o[hit]))
    assert np.array_equal(tri1, tri0) and np.array_equal(_bits(t1), _bits(t0)) and _same(col1, col0)
    tri_a, t_a, col_a = so.render_paths(p)
    assert np.array_equal(tri1, tri_a) and np.array_equal(_bits(t1), _bits(t_a)) and _same(col1, col_a)

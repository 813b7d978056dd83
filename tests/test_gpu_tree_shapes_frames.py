"""The render on every tree shape a caller can pass (tests/tree_shapes.py: coloured, CAMERAS): `render` / `render_device` -- the chunk
pipeline that bench.py times: chunk_prologue, per bounce a traceq4_kernel instance, the redo launch and the shading stages, then
accumulate_kernel -- on a median tree with leaves of one triangle, leaves of 128, a chain of depth 63, a root that is a leaf, a root
with two leaves, triangles that no leaf holds, loose boxes, a leaf box that misses a vertex and the device LBVH builder's trees; every
shape that walks with the re-tree off and on.  tests/test_gpu_tree_shapes_rays.py reaches traceq4_kernel only through the device-query
route (one instance, its own scratch and redo launch); here its instances of a render call run: the primary stage with generated
rays, the common-origin variant, the bounce stages plain, SEMI and with the scattered draw.

Every triangle carries a material of its own and a byte-identical copy never its original's, so a frame shows which of the two won
a tie (tests/test_tree_shapes.py: 4 to 17 % of the pixels of the small frame depend on it, and 6 % on the triangles that no leaf
holds being left unseen).  Every comparison is on the bits with the CPU oracle on the same arrays, computed once per shape and shared
by the re-tree settings; nothing of the product is in an expectation.  No oracle frame holds a NaN (asserted on the CPU)."""
import os
import sys

import numpy as np
import pytest

from ezrt_amd import refit, trace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_shapes as T  # noqa: E402
from test_gpu_timed_kernel_audit import _camera_rays  # noqa: E402
from test_gpu_tree_shapes_rays import CASES, STEP, _ids, _route, _scene  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INTEGRATORS = (3, 4, 50, 51, 52)
AUDITED = (50, 51)
AUDIT_FRAMES = (0, 7)
RAGGED = (61, 45)                                                      # not whole 16 x 16 blocks: the eager-direction path
RECT = dict(rect=(5, 3, 57, 44), tile=(16, 16), shard=(1, 3))
KEPT = np.float32(7.25)                                                # what the caller's buffer holds where a shard does not own the pixel
# one fresh scene per option set; every one only reschedules the same arithmetic
SCHEDULE = ({"gen_primary": 0}, {"rel_boxes": 0}, {"bounce_scatter": 0}, {"semi": 0}, {"semi": 2}, {"prune": 0}, {"prune": 1},
            {"prune_mis": 0}, {"prune_mis": 1}, {"tie_lca": 0}, {"anyhit": 0}, {"steal": 0}, {"handover": 0}, {"lds_nodes": 0},
            {"leaf_threshold": 1}, {"leaf_threshold": 64}, {"stack_cap": 4}, {"debug_force_pending": 3}, {"lazy_dir": 0}, {"wide4": 0},
            {"wide4": 0, "steal": 0}, {"megakernel": 1}, {"pipeline_calls": 0}, {"instrumentation": 1})
# chain and median1: a ring of four rows and a spill area of 0, 4, 16 (the production size) and 28 entries per lane (4 + 28: the
# production depth of 32)
STACK_CAPS = ({"debug_stack_cap": 1}, {"debug_stack_cap": 2}, {"debug_stack_cap": 5}, {"debug_stack_cap": 8})
POOL_SHAPES = ("chain", "median1", "leaf128", "uncovered", "lbvh1")
POOL_CASES = [(n, r) for n, r in CASES if n in POOL_SHAPES]
POOL_FRAME = dict(w=256, h=192, spp=16)                               # 786 432 pixel-samples in one chunk: static rounds >= 2 with pools of 8
POOL_INTEGRATORS = ((50, 4), (51, 2))
SMALL_POOLS = {"bounce_scatter": 1, "pool_max": 8, "pipeline_calls": 0, "static_pct": 50}
REFIT_CASES = [(n, r) for n, r in CASES if n in ("median1", "uncovered")]
SECOND_EYE = np.float64([0.5, 0.25, -0.5])                             # the second camera of the stream-order test: the eye moved by this

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _env_scene(lib, arrays):
    s = lib.scene_create(*arrays)
    s.set_env(*T.frame_env())
    return s


def _device_scene(hip, name, retree, arrays=None, **options):
    sg = _scene(hip, name, retree, arrays or T.coloured(name))
    sg.set_env(*T.frame_env())
    for k, v in options.items():
        if k == "instrumentation":
            sg.set_instrumentation(v)
        else:
            sg.set_option(k, v)
    return sg


def _differ(got, want):
    return int((~T.same_pixels(got, want)).sum())


def _same(got, want, what):
    n = _differ(got, want)
    assert n == 0, "%s: %d of %d pixels differ from the oracle's" % (what, n, want.shape[0] * want.shape[1])


def _calls(lib_scene, name, integ):
    """the four calls of one integrator on a scene: the small frame, its continuation into the same accumulator, the ragged frame and
    the rect of one tile shard over a buffer the caller filled"""
    first = lib_scene.render(T.frame_params(name, integ)).copy()
    acc = lib_scene.render(T.frame_params(name, integ, frame0=T.FRAME_SPP, spp=3), first.copy())
    ragged = lib_scene.render(T.frame_params(name, integ, w=RAGGED[0], h=RAGGED[1]))
    shard = lib_scene.render(T.frame_params(name, integ, **RECT), np.full((T.FRAME_H, T.FRAME_W, 4), KEPT, np.float32))
    return dict(first=first, continued=acc, ragged=ragged, shard=shard)


def _oracle_calls(oracle, name):
    def make():
        so = _env_scene(oracle, T.coloured(name))
        out = {integ: _calls(so, name, integ) for integ in INTEGRATORS}
        out["counters"] = so.counters()
        return out
    return _once(("calls", name), make)


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_frames_equal_the_oracles(hip, oracle, name, retree):
    """integrators 3, 4, 50, 51 and 52 at 3 bounces: 64 x 48 at 4 spp, continued with frames 4 .. 6 into the same accumulator, a ragged
    61 x 45 frame, and a rect of one tile shard of three, whose other pixels keep the caller's values; the ray and sample counts"""
    want = _oracle_calls(oracle, name)
    sg = _device_scene(hip, name, retree)
    _route(sg, name, retree)
    for integ in INTEGRATORS:
        got = _calls(sg, name, integ)
        for key in ("first", "continued", "ragged", "shard"):
            _same(got[key], want[integ][key], "%s, integrator %d, %s" % (name, integ, key))
        kept = (want[integ]["shard"] == KEPT).all(-1)
        assert 0.5 < kept.mean() < 0.95 and not T.same_pixels(want[integ]["first"], want[integ]["continued"]).all()
    c = sg.counters()
    assert c["rays"] == want["counters"]["rays"] > 0 and c["samples"] == want["counters"]["samples"] > 0, (c, want["counters"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_every_stage_queue_of_a_frame(hip, oracle, name, retree):
    """audit_via_queue = 1: render_paths from the hit records the stages of a render call leave -- ids, distances and colours of every
    ray slot of every path.  This sees the id of a tie's winner directly.  (Not the any-hit kernel of the MIS shadow rays, which the
    path log switches off; the frames above see that one.)"""
    sg = _device_scene(hip, name, retree, audit_via_queue=1)
    for integ in AUDITED:
        for frame in AUDIT_FRAMES:
            p = T.frame_params(name, integ, spp=1, frame0=frame)
            to, do, co = _once(("paths", name, integ, frame), lambda: _env_scene(oracle, T.coloured(name)).render_paths(p))
            tg, dg, cg = sg.render_paths(p)
            what = "%s, integrator %d, frame %d" % (name, integ, frame)
            assert np.array_equal(tg, to), "%s: the ids of %d ray slots differ" % (what, int((tg != to).sum()))
            assert np.array_equal(_bits(dg), _bits(do)), what
            assert np.array_equal(_bits(cg), _bits(co)), what
            assert (to[..., 0] >= 0).any() and (to[..., 1:] >= -1).any()


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_the_cameras_primary_rays_through_the_common_origin_variant(hip, oracle, name, retree):
    """audit_via_queue = 2: query_hits treats the rays as sharing ray 0's origin -- the primary stage's instance without the ray
    generation, on boxes translated by the eye"""
    eye, cam = T._look_at(*T.CAMERAS[name])
    rays = _camera_rays(T.FRAME_W, T.FRAME_H, eye, cam, T.SEEDS[name])
    to, do = _once(("primary", name), lambda: oracle.scene_create(*T.coloured(name)).query_hits(rays))
    assert (to >= 0).mean() > 0.05
    for options in ({}, {"rel_boxes": 0}):
        tg, dg = _device_scene(hip, name, retree, audit_via_queue=2, **options).query_hits(rays)
        assert np.array_equal(tg, to) and np.array_equal(_bits(dg), _bits(do)), (name, options)


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_the_schedule_on_the_tree(hip, oracle, name, retree):
    """Every option set on a fresh scene: the frames of integrators 50 and 51 are the ORACLE's, not merely the default's.  On chain
    and median1 also the tiny rings of debug_stack_cap with spill areas of 0 to 28 entries (wide4 0 puts the binary kernel on the
    chain's depth of 63)."""
    want = _oracle_calls(oracle, name)
    for options in SCHEDULE + (STACK_CAPS if name in ("chain", "median1") else ()):
        sg = _device_scene(hip, name, retree, **options)
        for integ in AUDITED:
            _same(sg.render(T.frame_params(name, integ)), want[integ]["first"], "%s, integrator %d, %r" % (name, integ, options))


def test_a_spill_area_beyond_the_production_depth_is_refused(hip):
    sg = _device_scene(hip, "root_leaf_8", None)
    sg.set_option("debug_stack_cap", 8)
    for value in (9, 64, -1):
        with pytest.raises(trace.TraceError, match="outside"):
            sg.set_option("debug_stack_cap", value)


@pytest.mark.parametrize("name,retree", POOL_CASES, ids=_ids(POOL_CASES))
def test_pools_static_rounds_and_stealing(hip, oracle, name, retree):
    """256 x 192 at 16 spp -- 786 432 pixel-samples in one chunk -- by default and with pools of 8 rays dealt half statically under the
    scattered draw (static rounds >= 2), against the oracle"""
    for integ, bounces in POOL_INTEGRATORS:
        p = T.frame_params(name, integ, bounces=bounces, **POOL_FRAME)
        want = _once(("pool", name, integ), lambda: _env_scene(oracle, T.coloured(name)).render(p))
        for options in ({}, SMALL_POOLS):
            _same(_device_scene(hip, name, retree, **options).render(p), want, "%s, integrator %d, %r" % (name, integ, options))


def _moved(name):
    """the arrays moved by STEP, with refit_nodes: every triangle, or on `uncovered` only the triangles that no leaf holds"""
    tri, nodes = T.coloured(name)
    which = T.shape(name)[2].get("uncovered", slice(None))
    moved = np.array(tri)
    for v in range(3):
        moved[which, 3 * v:3 * v + 3] += STEP
    assert np.array_equal((moved[:, :9] != tri[:, :9]).any(1).nonzero()[0], np.arange(tri.shape[0])[which])
    return moved, refit.refit_nodes(moved, nodes)


@pytest.mark.parametrize("name,retree", REFIT_CASES, ids=_ids(REFIT_CASES))
def test_a_refit_by_an_exact_step(hip, oracle, name, retree):
    """The triangles move by (0.25, -0.5, 0.25), exact on the base set's multiples of 1/4, under a camera that stays: the frames are the
    oracle's on the moved arrays with refit_nodes and those of a scene created afresh from them; refitted back, the first call's bits.
    (The triangles that no leaf holds are never seen: moving them must change no pixel.)"""
    arrays = _moved(name)
    want = _oracle_calls(oracle, name)
    sg = _device_scene(hip, name, retree)
    info = sg.prune_info()
    first = {integ: sg.render(T.frame_params(name, integ)) for integ in AUDITED}
    for integ in AUDITED:
        _same(first[integ], want[integ]["first"], "%s, integrator %d" % (name, integ))
    refit.refit(sg, arrays[0])
    assert sg.prune_info()["mode"] == info["mode"] and sg.prune_info()["records4"] == info["records4"]
    afresh = _device_scene(hip, name, retree, arrays)
    for integ in AUDITED:
        p = T.frame_params(name, integ)
        moved = _once(("moved", name, integ), lambda: _env_scene(oracle, arrays).render(p))
        assert (_differ(moved, want[integ]["first"]) > 0.5 * T.FRAME_W * T.FRAME_H) == (name != "uncovered")
        _same(sg.render(p), moved, "%s, integrator %d, moved" % (name, integ))
        _same(afresh.render(p), moved, "%s, integrator %d, created afresh" % (name, integ))
    refit.refit(sg, np.array(T.coloured(name)[0]))
    for integ in AUDITED:
        _same(sg.render(T.frame_params(name, integ)), first[integ], "%s, integrator %d, moved back" % (name, integ))


@pytest.mark.parametrize("name,retree", CASES, ids=_ids(CASES))
def test_two_calls_on_one_stream_into_two_buffers(hip, oracle, name, retree):
    """render_device twice on one stream with two cameras and no host wait between the calls: each buffer is the oracle's frame"""
    dev = torch.device("cuda", 0)
    eye, target = (np.float64(x) for x in T.CAMERAS[name])
    p = [trace.make_params(T.FRAME_W, T.FRAME_H, *T._look_at(e, target), integ, T.FRAME_BOUNCES, spp=T.FRAME_SPP)
         for e, integ in ((eye, 50), (eye + SECOND_EYE, 51))]
    want = _once(("stream", name), lambda: [_env_scene(oracle, T.coloured(name)).render(q) for q in p])
    assert _differ(want[0], want[1]) > 0.1 * T.FRAME_W * T.FRAME_H
    sg = _device_scene(hip, name, retree)
    frames = [hip.frame(T.FRAME_W, T.FRAME_H) for _ in p]
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sg.render_device(p[0], frames[0].ptr, s.cuda_stream)
    sg.render_device(p[1], frames[1].ptr, s.cuda_stream)
    s.synchronize()
    for k in (0, 1):
        _same(frames[k].read(), want[k], "%s, call %d" % (name, k))

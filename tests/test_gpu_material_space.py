"""The whole pipeline across material space: device == oracle on the bits for a QUILT scene -- the Bunny over the floor quad
under the shipped map, every triangle dressed with its own material from the generator of the function-level tests
(tests/fn_operands.py: quilt_scene).  The device finds the distinct materials at ezrt_scene_create, derives their constants
on the host, packs one table row each and reaches them through an index per triangle; the fixtures of the other GPU tests
have at most a few dozen rows.  Here there are ~5 000, with pairs that differ only in the sign of a zero or only in the
unused IOR / transmission, runs of equal materials, materials that come back after others, emitters, black and
single-parameter-edge rows.

Frames of integrators 3, 4, 50, 51, 52 with the filters and clamp of their chapters, a non-power-of-two frame, path
records, every route (default, megakernel, audit_via_queue, env_planes = 0, env_rgbe = 0, chunk_log2 = 12), and once more
after an identity refit and a rigid one (the materials must survive).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fn_operands as F  # noqa: E402

from ezrt_amd import refit, scene as S, trace  # noqa: E402

W, H = 203, 117
CAMERA = (30, 20, 2.5)
FRAMES = [  # (integrator, max_bounce, env filter, env clamp): the chapters' settings, as tests/test_ref_fsh_pin.py FRAME_CASES
    (3, 4, 0, 10.0),
    (4, 4, 0, 0.0),
    (50, 4, 1, 0.0),
    (51, 4, 1, 0.0),
    (52, 4, 1, 0.0),
    (51, 8, 1, 0.0),
]
ROUTES = [(), (("megakernel", 1),), (("audit_via_queue", 1),), (("env_planes", 0),), (("env_rgbe", 0),), (("chunk_log2", 12),)]


@pytest.fixture(scope="module")
def quilt():
    return F.quilt_scene()


def _same(a, b):
    return F.same_bits(a, b)


def _params(integ, mb, clamp, spp=2, frame0=0):
    eye, cam = S.camera(*CAMERA)
    return trace.make_params(W, H, eye, cam, integ, mb, spp=spp, frame0=frame0, env_clamp=clamp)


def test_quilt_has_the_material_patterns_it_claims(quilt):
    m = quilt.tri[:, 18:36]
    n_distinct, cls = F.distinct_materials(m)
    print("quilt: %d triangles, %d distinct materials" % (len(m), n_distinct))
    assert n_distinct >= 4096
    b = m.view(np.uint32)
    i = np.arange(len(m))
    k1 = i[(i % 64 == 1)]
    assert (m[k1] == m[k1 - 1]).all() and (b[k1, 11] != b[k1 - 1, 11]).all() and (cls[k1] != cls[k1 - 1]).all()   # -0.0 / +0.0
    k3 = i[(i % 64 == 3)]
    assert (b[k3, :16] == b[k3 - 1, :16]).all() and (cls[k3] != cls[k3 - 1]).all()                            # IOR / transmission only
    k7 = i[(i % 64 == 7)]
    assert (cls[k7] == cls[k7 - 3]).all()                                                                    # a run of four
    k8 = i[(i % 64 == 8) & (i >= 40)]
    assert (cls[k8] == cls[k8 - 40]).all() and (cls[k8] != cls[k8 - 1]).all()                                # comes back after others
    assert 0.02 < float((m[:, 0:3].sum(1) > 0).mean()) < 0.05                                                # emitters


@pytest.mark.gpu
def test_quilt_frames_and_paths_equal_the_oracle_on_every_route(hip, oracle, quilt):
    sg, so = quilt.upload(hip), quilt.upload(oracle)
    assert sg.stats()["n_tri"] == len(quilt.tri)
    _, cls = F.distinct_materials(quilt.tri[:, 18:36])
    reached = set()
    for integ, mb, filt, clamp in FRAMES:
        sg.set_env(quilt.hdr, quilt.cache, filt)
        so.set_env(quilt.hdr, quilt.cache, filt)
        p = _params(integ, mb, clamp)
        want = so.render(p)
        to, do, co = so.render_paths(p)
        later = to[..., 1:]
        reached.update(np.unique(later[later >= 0]).tolist())
        assert np.isfinite(want[..., :3]).mean() > 0.99 and float(np.nanmax(want[..., :3])) > 0.5
        for route in ROUTES:
            for name, v in route:
                sg.set_option(name, v)
            assert _same(sg.render(p), want), (integ, mb, route, "frame")
            tg, dg, cg = sg.render_paths(p)
            assert np.array_equal(tg, to) and _same(dg, do) and _same(cg, co), (integ, mb, route, "paths")
            for name, v in route:
                sg.set_option(name, {"megakernel": 0, "audit_via_queue": 0, "env_planes": 1, "env_rgbe": 1, "chunk_log2": 26}[name])
    # not vacuous: the paths' later hits land on more than a thousand materials, the awkward ones among them
    ids = np.array(sorted(reached))
    m = quilt.tri[ids, 18:36]
    n_reached = np.unique(cls[ids]).size
    print("quilt: bounce hits on %d triangles, %d distinct materials; emitters %d, black %d, metallic==1 %d" % (
        ids.size, n_reached, int((m[:, 0:3].sum(1) > 0).sum()), int((m[:, 3:6] == 0).all(1).sum()), int((m[:, 7] == 1).sum())))
    assert n_reached >= 1000
    assert (m[:, 0:3].sum(1) > 0).any() and (m[:, 3:6] == 0).all(1).any() and (m[:, 7] == 1).any()


def _rigid(tri, th, shift):
    t = tri.copy()
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float64)
    P = t[:, :9].reshape(-1, 3, 3).astype(np.float64)
    t[:, :9] = (P @ R.T + np.asarray(shift)).reshape(-1, 9).astype(np.float32)
    N = t[:, 9:18].reshape(-1, 3, 3).astype(np.float64)
    t[:, 9:18] = (N @ R.T).reshape(-1, 9).astype(np.float32)
    return t


@pytest.mark.gpu
def test_quilt_materials_survive_a_refit(hip, oracle, quilt):
    sg = quilt.upload(hip)
    for what, tri2 in (("identity", quilt.tri), ("rigid", _rigid(quilt.tri, 0.6, (0.3, -0.2, 0.1)))):
        refit.refit(sg, np.ascontiguousarray(tri2))
        so = oracle.scene_create(tri2, refit.refit_nodes(tri2, quilt.nodes))
        for integ, mb, filt, clamp in ((4, 4, 0, 0.0), (51, 4, 1, 0.0), (52, 4, 1, 0.0)):
            sg.set_env(quilt.hdr, quilt.cache, filt)
            so.set_env(quilt.hdr, quilt.cache, filt)
            p = _params(integ, mb, clamp)
            assert _same(sg.render(p), so.render(p)), (what, integ, "frame")
            a, b = sg.render_paths(p), so.render_paths(p)
            assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]), (what, integ, "paths")

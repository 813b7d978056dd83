"""Stream-ordered path queries (include/ezrt_path.h, ezrt_amd/path.py): the render's primary rays and the radiance an integrator
returns along caller rays, on device tensors, compared ON THE BITS (a NaN equals a NaN) with the path audit (ezrt_render_paths) of
the CPU oracle and of the HIP library, and -- for rays that are no camera's -- with a numpy-float32 composition of the existing
device queries.  Frames are 40 x 24: no power of two and W != H, so the divisions of the ray generator are real ones.
"""
import ctypes as C

import numpy as np
import pytest

from ezrt_amd import refit, trace
from ezrt_amd import scene as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EZRT_ERR_INVALID = -1
W, H = 40, 24
FRAMES = (0, 7)
CAMERAS = ((15, 8, 3.0), (90, 10, 2), (33, -20, 1.2))          # the last one is close to the mesh
CASES = ((3, 2), (4, 4), (50, 4), (51, 2), (51, 3), (52, 2))   # (integrator, max_bounce)
f32 = np.float32
u32 = np.uint32
MISS_T = f32(114514.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def path():
    from ezrt_amd import path
    return path


@pytest.fixture(scope="module")
def sg(hip, bunny_small):
    return bunny_small.upload(hip)


@pytest.fixture(scope="module")
def so(oracle, bunny_small):
    return bunny_small.upload(oracle)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _clamp(integ):
    return 10.0 if integ == 3 else 0.0


def _params(cam, integ, mb, frame=0):
    eye, rot = S.camera(*cam)
    return trace.make_params(W, H, eye, rot, integ, mb, frame0=frame, env_clamp=_clamp(integ))


def _frame_xyf(frame, w=W, h=H):
    """(ix, iy, frame) of every pixel of a frame, row-major as the audit's arrays"""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel(), np.full(w * h, frame)], 1).astype(u32)


def _dev_xyf(xyf, dev):
    return torch.from_numpy(np.ascontiguousarray(xyf, u32).view(np.int32)).to(dev).view(torch.uint32)


def _np(*xs):
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in xs)


_AUDITS = {}


def _audit(so, cam, integ, mb, frame, sampler=8):
    """The oracle's path audit of one frame, computed once and shared: (ids [H*W, slots], t, colour [H*W, 3]), read-only."""
    key = (cam, integ, mb, frame, sampler)
    if key not in _AUDITS:
        tri, t, col = so.render_paths(_params(cam, integ, mb, frame))
        out = (tri.reshape(W * H, -1), t.reshape(W * H, -1), col.reshape(W * H, 3))
        for a in out:
            a.setflags(write=False)
        _AUDITS[key] = out
    return _AUDITS[key]


# ---- 1. camera rays are the render's

def test_camera_rays_are_the_renders(path, dev, sg, so):
    from ezrt_amd import query
    for cam in CAMERAS:
        for frame in FRAMES:
            p = _params(cam, 50, 0, frame)
            rays = path.camera_rays(sg, p, _dev_xyf(_frame_xyf(frame), dev))
            tri, t = query.closest(sg, rays)
            rays, tri, t = _np(rays, tri, t)
            ids, tt, _ = _audit(so, cam, 50, 0, frame)
            assert rays.shape == (W * H, 6) and rays.dtype == np.float32
            assert np.array_equal(_bits(rays[:, 0:3]), _bits(np.tile(np.array(list(p.eye), f32), (W * H, 1))))   # the origin is eye
            assert np.isfinite(rays[:, 3:6]).all()
            assert np.abs(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) - 1.0).max() < 1e-6
            assert np.array_equal(tri, ids[:, 0]), "%s frame %d: %d ids differ" % (cam, frame, int((tri != ids[:, 0]).sum()))
            assert np.array_equal(_bits(t), _bits(tt[:, 0]))
            assert 0.2 < (ids[:, 0] >= 0).mean() < 1.0 and (t[tri < 0] == MISS_T).all()
    # the jitter is the pixel-sample's: another frame, other directions
    p = _params(CAMERAS[0], 50, 0)
    a, b = _np(path.camera_rays(sg, p, _dev_xyf(_frame_xyf(0), dev)), path.camera_rays(sg, p, _dev_xyf(_frame_xyf(7), dev)))
    assert (_bits(a[:, 3:6]) != _bits(b[:, 3:6])).any(1).mean() > 0.9
    # a pixel beyond the frame is computed like any other: the direction of its pixel centre, within the jitter's half pixel
    xyf = np.array([[W - 1, 3, 0], [W + 5, 3, 0], [2, H + 9, 1]], u32)
    got, = _np(path.camera_rays(sg, p, _dev_xyf(xyf, dev)))
    assert np.isfinite(got).all()
    m = np.array(list(p.camera_rotate), np.float64).reshape(4, 4).T
    v = np.stack([(xyf[:, 0] + 0.5) / W * 2 - 1, (xyf[:, 1] + 0.5) / H * 2 - 1, np.full(3, -1.5)], 1)
    want = v @ m[:3, :3].T
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(got[:, 3:6] - want).max() < 1.0 / min(W, H) and not _same(got[0, 3:6], got[1, 3:6])
    # the pixel rect, the tiles and the shard of the params are not applied
    eye, rot = S.camera(*CAMERAS[0])
    q = trace.make_params(W, H, eye, rot, 50, 0, rect=(8, 8, 16, 16), tile=(8, 8), shard=(1, 3))
    assert _same(_np(path.camera_rays(sg, q, _dev_xyf(_frame_xyf(0), dev)))[0], a)


# ---- 2. radiance equals the path audit

def _check_against_audits(path, dev, sg, so, integ, mb, sampler=8):
    for frame in FRAMES:
        cam = CAMERAS[0]
        p = _params(cam, integ, mb, frame)
        ids, _, want = _audit(so, cam, integ, mb, frame, sampler)
        assert (ids[:, 0] >= 0).mean() >= 0.2, "too few paths hit the mesh"
        assert (ids[:, -1] >= -1).any(), "no path reaches the last bounce"
        tg, _, cg = sg.render_paths(p)
        assert np.array_equal(tg.reshape(ids.shape), ids) and _same(cg.reshape(-1, 3), want)     # the HIP library's own audit
        xyf = _dev_xyf(_frame_xyf(frame), dev)
        got, = _np(path.radiance(sg, path.camera_rays(sg, p, xyf), xyf, integrator=integ, max_bounce=mb, env_clamp=_clamp(integ)))
        bad = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all(1)
        assert not bad.any(), "integrator %d, %d bounces, frame %d: %d of %d pixels differ; first %d: %r != %r" % (
            integ, mb, frame, int(bad.sum()), len(bad), int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])
        assert float(np.nanmax(want)) > 0.1 and np.isnan(want).any(1).mean() < 0.01           # NaN == NaN hides next to nothing


@pytest.mark.parametrize("integ,mb", CASES)
def test_radiance_of_camera_rays_equals_the_path_audit(path, dev, sg, so, integ, mb):
    _check_against_audits(path, dev, sg, so, integ, mb)


def test_radiance_with_sixteen_sobol_dimensions(path, dev, hip, oracle, bunny_small):
    """ezrt_scene_set_sampler(16): 4 bounces (dimensions 0-7 only), and 6, where dimensions 8-11 are in use."""
    sg, so = bunny_small.upload(hip), bunny_small.upload(oracle)
    sg.set_sampler(16)
    so.set_sampler(16)
    _check_against_audits(path, dev, sg, so, 50, 4, sampler=16)
    _check_against_audits(path, dev, sg, so, 50, 6, sampler=16)
    # the setting is in use: with eight dimensions bounces 4 and 5 wrap to dimensions 0-3 and the same frame comes out differently.
    # (Frame 7 -- at frame 0 the Sobol index is 1, whose point is 0.5 in EVERY dimension, so no frame 0 can tell the settings apart.)
    eight = bunny_small.upload(oracle).render_paths(_params(CAMERAS[0], 50, 6, 7))[2].reshape(-1, 3)
    assert not _same(_audit(so, CAMERAS[0], 50, 6, 7, 16)[2], eight)
    assert _same(_audit(so, CAMERAS[0], 50, 6, 0, 16)[2], bunny_small.upload(oracle).render_paths(_params(CAMERAS[0], 50, 6, 0))[2].reshape(-1, 3))


# ---- 3. batch shape and order are free

def test_batch_shape_and_order_are_free(path, dev, sg, so):
    integ, mb = 51, 2
    rays, xyf, want = [], [], []
    for k, cam in enumerate(CAMERAS):
        frame = FRAMES[k % 2]
        x = _frame_xyf(frame)
        rays.append(path.camera_rays(sg, _params(cam, integ, mb, frame), _dev_xyf(x, dev)))
        xyf.append(x)
        want.append(_audit(so, cam, integ, mb, frame)[2])
    rays, xyf, want = torch.cat(rays), np.concatenate(xyf), np.concatenate(want)
    perm = np.random.default_rng(5).permutation(len(xyf))
    rays = rays[torch.from_numpy(perm).to(dev)].contiguous()                            # three eyes mixed: no shared origin
    xyf, want = xyf[perm], want[perm]
    assert np.unique(_np(rays)[0][:300, 0:3], axis=0).shape[0] == 3
    dx = _dev_xyf(xyf, dev)
    full, = _np(path.radiance(sg, rays, dx, integrator=integ, max_bounce=mb))
    assert _same(full, want)
    for n in (1, 63, 64, 65, 257):
        got, = _np(path.radiance(sg, rays[:n].contiguous(), dx[:n].contiguous(), integrator=integ, max_bounce=mb))
        assert got.shape == (n, 3) and _same(got, want[:n]), n
    # leading dimensions are kept
    lead = (3, H, W)
    got = path.radiance(sg, rays.reshape(lead + (6,)), dx.reshape(lead + (3,)), integrator=integ, max_bounce=mb)
    assert tuple(got.shape) == lead + (3,) and _same(_np(got)[0].reshape(-1, 3), want)
    assert tuple(path.camera_rays(sg, _params(CAMERAS[0], integ, mb), dx.reshape(lead + (3,))).shape) == lead + (6,)
    # int32 tensors with the same bits are taken as they are
    assert _same(_np(path.radiance(sg, rays, dx.view(torch.int32), integrator=integ, max_bounce=mb))[0], want)
    # n == 0
    e = path.radiance(sg, rays[:0].contiguous(), dx[:0].contiguous(), integrator=integ, max_bounce=mb)
    assert tuple(e.shape) == (0, 3) and tuple(path.camera_rays(sg, _params(CAMERAS[0], integ, mb), dx[:0].contiguous()).shape) == (0, 6)


# ---- 4. the pixel-sample is independent of the ray: integrator 50, one bounce, as a composition of the other device queries

def _wang(seed):
    seed = (seed ^ u32(61)) ^ (seed >> u32(16))
    seed = seed * u32(9)
    seed = seed ^ (seed >> u32(4))
    seed = seed * u32(0x27d4eb2d)
    return seed ^ (seed >> u32(15))


def _cp_offsets(ix, iy):
    """CranleyPattersonRotation's offsets of pixel (ix, iy), the hash restated on uint32 arrays (they wrap as the device's)"""
    s = (ix * u32(1973) + iy * u32(9277) + u32(59) * u32(26699)) | u32(1)
    s = _wang(s)
    u = s.astype(f32) / f32(4294967296.0)
    s = _wang(s)
    return u, s.astype(f32) / f32(4294967296.0)


def _cp_rotate(p, off):
    p = (p + off).astype(f32)
    p = np.where(p > f32(1), p - f32(1), p).astype(f32)
    return np.where(p < f32(0), p + f32(1), p).astype(f32)


def _dot(a, b):
    """the device's dot: left to right, every product and sum rounded to float32"""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


def test_the_pixel_sample_is_independent_of_the_ray(path, dev, sg, oracle):
    from ezrt_amd import query, shade
    n = 2000
    rng = np.random.default_rng(41)
    o = rng.uniform(-2, 2, (n, 3))
    o[:, 1] = rng.uniform(-1.3, 2, n)
    tgt = rng.uniform(-1.5, 1.5, (n, 3))
    tgt[:, 1] = rng.uniform(-1.6, 1.0, n)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays_np = np.concatenate([o, d], 1).astype(f32)
    xyf = np.stack([rng.integers(0, 5000, n), rng.integers(0, 5000, n), rng.integers(0, 64, n)], 1).astype(u32)
    rays, dx = torch.from_numpy(rays_np).to(dev), _dev_xyf(xyf, dev)
    got1, got0 = _np(path.radiance(sg, rays, dx, integrator=50, max_bounce=1), path.radiance(sg, rays, dx, integrator=50, max_bounce=0))

    # the same path out of the other queries
    s = query.surface(sg, rays, integrator=50)
    sob = oracle.sobol(1, 64, 8)                                    # row f: sobol(d, gray_code(f + 1))
    cpu, cpv = _cp_offsets(xyf[:, 0], xyf[:, 1])
    xi = np.zeros((n, 3), f32)
    xi[:, 0] = _cp_rotate(sob[xyf[:, 2], 0], cpu)
    xi[:, 1] = _cp_rotate(sob[xyf[:, 2], 1], cpv)
    V = (-rays[:, 3:6]).contiguous()
    L = shade.sample(sg, s.tri, torch.from_numpy(xi).to(dev), V, s.normal, integrator=50)
    f_r, _ = shade.evaluate(sg, s.tri, V, s.normal, L, integrator=50, want_pdf=False)
    up = torch.tensor([0.0, 1.0, 0.0], device=dev).expand(n, 3)
    Lq = torch.where((s.tri >= 0)[:, None], L, up).contiguous()     # a primary miss has no next ray: any direction but (0, 0, 0)
    nt, _ = query.closest(sg, torch.cat([s.point, Lq], 1))
    sky, _ = shade.env_evaluate(sg, Lq, 0.0, want_pdf=False)
    sky0, _ = shade.env_evaluate(sg, rays[:, 3:6].contiguous(), 0.0, want_pdf=False)
    Le0, Le1 = shade.material(sg, s.tri)[:, 0:3], shade.material(sg, nt)[:, 0:3]
    tri, N, L, f_r, nt, sky, sky0, Le0, Le1 = _np(s.tri, s.normal, L, f_r, nt, sky, sky0, Le0, Le1)
    miss, then_sky, then_hit = tri < 0, (tri >= 0) & (nt < 0), (tri >= 0) & (nt >= 0)
    assert miss.mean() >= 0.1 and then_sky.mean() >= 0.1 and then_hit.mean() >= 0.1, (miss.mean(), then_sky.mean(), then_hit.mean())

    PI = f32(3.1415926)
    pdf = f32(1.0) / (f32(2.0) * PI)
    zero = f32(0)
    dln = _dot(L, N)
    cosine = np.where(zero < dln, dln, zero).astype(f32)[:, None]   # ez_max(0, dot(L, N))
    light = np.where((nt < 0)[:, None], sky, Le1).astype(f32)       # history = (1, 1, 1): history * light is light
    Lo = (zero + (((light * f_r).astype(f32) * cosine).astype(f32) / pdf).astype(f32)).astype(f32)
    want1 = np.where(miss[:, None], sky0, (Le0 + Lo).astype(f32)).astype(f32)
    want0 = np.where(miss[:, None], sky0, (Le0 + zero).astype(f32)).astype(f32)
    for name, got, want in (("one bounce", got1, want1), ("no bounce", got0, want0)):
        bad = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all(1)
        assert not bad.any(), "%s: %d of %d rays differ; first %d: %r != %r" % (
            name, int(bad.sum()), n, int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])
    assert np.isfinite(want1).all() and float(np.abs(Lo[then_sky]).max()) > 0.1 and (Lo[then_hit] != 0).any()
    # the random numbers are those of the pixel-sample named, not of the ray's position in the batch: another sample, another bounce
    other, = _np(path.radiance(sg, rays, _dev_xyf(xyf + u32(1), dev), integrator=50, max_bounce=1))
    assert _same(other[miss], got1[miss]) and (_bits(other[~miss]) != _bits(got1[~miss])).any(1).mean() > 0.5


# ---- 5. ordering

def _one_frame(path, dev, sg, so, integ=51, mb=2, frame=7):
    cam = CAMERAS[1]
    x = _dev_xyf(_frame_xyf(frame), dev)
    return path.camera_rays(sg, _params(cam, integ, mb, frame), x), x, _audit(so, cam, integ, mb, frame)[2]


def test_a_query_sees_what_its_stream_wrote_before(path, dev, sg, so):
    rays, xyf, want = _one_frame(path, dev, sg, so)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        r2 = torch.zeros_like(rays)
        x2 = torch.zeros_like(xyf.view(torch.int32))
        torch.cuda._sleep(20_000_000)                       # the writes below are still queued when the query is enqueued
        r2.copy_(rays)
        x2.copy_(xyf.view(torch.int32))
        got = path.radiance(sg, r2, x2, integrator=51, max_bounce=2)          # the current stream: `side`
        again = path.radiance(sg, r2, x2, integrator=51, max_bounce=2, stream=side.cuda_stream)
    assert _same(_np(got)[0], want) and _same(_np(again)[0], want)


def test_queries_beside_a_render_call(path, dev, hip, so, bunny_small):
    sg = bunny_small.upload(hip)
    rays, xyf, want = _one_frame(path, dev, sg, so)
    eye, rot = S.camera(*CAMERAS[0])
    p = trace.make_params(128, 96, eye, rot, 51, 2, spp=4, tile=(16, 16))
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def render():
        frame = torch.zeros((96, 128, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        sg.counters_reset()
        sg.render_device(p, frame.data_ptr(), a.cuda_stream)
        return frame

    alone = render()
    torch.cuda.synchronize()
    before = (sg.counters(), sg.last_render_ms()[2])
    beside = render()
    got = path.radiance(sg, rays, xyf, integrator=51, max_bounce=2, stream=b)
    cams = path.camera_rays(sg, _params(CAMERAS[1], 51, 2, 7), xyf, stream=b)
    torch.cuda.synchronize()
    assert _same(beside.cpu().numpy(), alone.cpu().numpy()) and float(alone.abs().max()) > 0.1
    assert (sg.counters(), sg.last_render_ms()[2]) == before                  # the queries leave counters and launch counts alone
    assert _same(_np(got)[0], want) and _same(_np(cams)[0], _np(rays)[0])


def test_radiance_after_a_refit(path, dev, hip, bunny_small):
    th = 0.6
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float64)
    moved = bunny_small.tri.copy()
    for k in range(6):
        moved[:, 3 * k:3 * k + 3] = (bunny_small.tri[:, 3 * k:3 * k + 3].astype(np.float64) @ R.T).astype(f32)
    fresh = hip.scene_create(moved, refit.refit_nodes(moved, bunny_small.nodes))
    fresh.set_env(bunny_small.hdr, bunny_small.cache)
    sg = bunny_small.upload(hip)
    xyf = _dev_xyf(_frame_xyf(7), dev)
    rays = path.camera_rays(sg, _params(CAMERAS[0], 51, 2, 7), xyf)
    before, = _np(path.radiance(sg, rays, xyf, integrator=51, max_bounce=2))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    pending = path.radiance(sg, rays, xyf, integrator=51, max_bounce=2, stream=side)      # the refit waits for it
    refit.refit(sg, moved)
    after = path.radiance(sg, rays, xyf, integrator=51, max_bounce=2)
    want, = _np(path.radiance(fresh, rays, xyf, integrator=51, max_bounce=2))
    assert _same(_np(after)[0], want) and _same(_np(pending)[0], before) and not _same(before, want)


# ---- 6. errors

def test_errors(path, dev, hip, sg, bunny_small):
    lib = hip.lib
    n = 100
    P = C.c_void_p
    xyf = _dev_xyf(_frame_xyf(0)[:n], dev)
    p = _params(CAMERAS[0], 51, 2)
    rays = path.camera_rays(sg, p, xyf)
    sentinel = 3.0
    o6 = torch.full((n, 6), sentinel, device=dev)
    o3 = torch.full((n, 3), sentinel, device=dev)
    spare = torch.empty((n, 6), device=dev)
    h6, h3, hx = np.full((n, 6), sentinel, f32), np.full((n, 3), sentinel, f32), np.full((n, 3), 5, u32)
    Hp = lambda x: P(x.ctypes.data)                                   # noqa: E731
    D = lambda x: P(x.data_ptr())                                     # noqa: E731
    torch.cuda.synchronize()

    def camera(s=sg._h, pp=C.byref(p), x=D(xyf), cnt=n, out=D(o6)):
        return lib.ezrt_camera_rays_device(s, pp, x, cnt, out, None)

    def radiance(s=sg._h, integ=51, mb=2, r=D(rays), x=D(xyf), cnt=n, out=D(o3)):
        return lib.ezrt_query_radiance_device(s, integ, mb, 0.0, r, x, cnt, out, None)

    def invalid(rc, what, needle=None):
        assert rc == EZRT_ERR_INVALID, what
        msg = lib.ezrt_last_error()
        assert msg and (needle is None or needle in msg), (what, msg)

    # host memory in any position is rejected, never read or written
    for fn, kws in ((camera, ({"x": Hp(hx)}, {"out": Hp(h6)})), (radiance, ({"r": Hp(h6)}, {"x": Hp(hx)}, {"out": Hp(h3)}))):
        for kw in kws:
            invalid(fn(**kw), (fn.__name__, sorted(kw)), b"device memory")
    assert (h6 == sentinel).all() and (h3 == sentinel).all() and (hx == 5).all()
    # NULL scene, params or pointer; n < 0
    for fn, names in ((camera, ("s", "pp", "x", "out")), (radiance, ("s", "r", "x", "out"))):
        for name in names:
            invalid(fn(**{name: None}), (fn.__name__, name))
        invalid(fn(cnt=-1), (fn.__name__, "n < 0"))
    # width or height <= 0
    for w, h in ((0, H), (W, 0), (-3, H)):
        q = _params(CAMERAS[0], 51, 2)
        q.width, q.height = w, h
        invalid(camera(pp=C.byref(q)), (w, h), b"width/height")
    # max_bounce < 0, unknown integrators
    invalid(radiance(mb=-1), "max_bounce < 0", b"max_bounce")
    for integ in (0, 1, 2, 5, 49, 53, -1, 1000):
        invalid(radiance(integ=integ), integ, b"integrator")
    # no environment; integrators 51 / 52 on an environment without a cache
    bare = hip.scene_create(bunny_small.tri, bunny_small.nodes)
    for integ in (3, 4, 50, 51, 52):
        invalid(radiance(s=bare._h, integ=integ), "no environment", b"environment")
    assert camera(s=bare._h, out=D(spare)) == 0                                              # the ray generator needs none
    nocache = hip.scene_create(bunny_small.tri, bunny_small.nodes)
    nocache.set_env(bunny_small.hdr, None)
    for integ in (51, 52):
        invalid(radiance(s=nocache._h, integ=integ), "MIS without a cache", b"cache")
    torch.cuda.synchronize()
    assert (o6.cpu().numpy() == sentinel).all() and (o3.cpu().numpy() == sentinel).all()     # nothing was launched by any of them
    # n == 0 is fine and launches nothing
    assert camera(cnt=0) == 0 and radiance(cnt=0) == 0
    torch.cuda.synchronize()
    assert (o6.cpu().numpy() == sentinel).all() and (o3.cpu().numpy() == sentinel).all()
    # the rejected calls left no HIP error behind: the next calls work, integrator 50 without a cache included
    assert radiance(s=nocache._h, integ=50) == 0 and camera() == 0
    torch.cuda.synchronize()
    assert _same(o6.cpu().numpy(), _np(rays)[0]) and np.isfinite(o3.cpu().numpy()).all() and (o3.cpu().numpy() != sentinel).any()
    # the wrapper: host tensors, other dtypes and shapes, non-contiguous tensors, other integrators, the oracle's scenes
    for bad in (lambda: path.camera_rays(sg, p, xyf.cpu()), lambda: path.camera_rays(sg, p, xyf.view(torch.int32).long()),
                lambda: path.camera_rays(sg, p, xyf.view(torch.int32).float()), lambda: path.camera_rays(sg, None, xyf),
                lambda: path.radiance(sg, rays.cpu(), xyf), lambda: path.radiance(sg, rays.double(), xyf),
                lambda: path.radiance(sg, rays, xyf.cpu()), lambda: path.radiance(None, rays, xyf)):
        with pytest.raises(TypeError):
            bad()
    wide = torch.zeros((n, 12), device=dev)
    for bad in (lambda: path.radiance(sg, rays[:, :3].contiguous(), xyf), lambda: path.radiance(sg, rays, xyf[:-1].contiguous()),
                lambda: path.radiance(sg, wide[:, :6], xyf), lambda: path.radiance(sg, rays, xyf, integrator=5),
                lambda: path.radiance(sg, rays, xyf, max_bounce=-1),
                lambda: path.camera_rays(sg, p, torch.zeros((n, 2), dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(trace.TraceError):
        path.radiance(bare, rays, xyf, integrator=50)

"""Stream-ordered ray queries on device tensors (include/ezrt_query.h, include/ezrt_surface.h).

    tri, t = query.closest(scene, rays)               # the reference's closest hit of every ray
    tri, t = query.closest(scene, rays, t_max)        # ... if it lies below t_max, else a miss
    hit = query.occluded(scene, rays, t_max)          # is anything in the way before t_max?  (bool)
    tri, t, point, normal, inside = query.surface(scene, rays)   # closest hit + hit point, shading normal, side (include/ezrt_surface.h)

`scene` is a `trace.Scene` of the HIP library, `rays` a contiguous float32 GPU tensor of shape [..., 6] (origin, direction) and
`t_max` (optional) a float32 GPU tensor of shape rays.shape[:-1].  The outputs keep the leading dimensions.  The work is enqueued on
`stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current stream of the rays' device) and the functions
return without waiting for it.  There is no t_min: a triangle is accepted at t >= 0.0005 only, so a ray leaving a surface needs its
origin offset by the caller.  A miss is (-1, 114514.0): ezrt_query_hits' miss (the reference's INF).
"""
import collections
import ctypes as C

import torch

from . import _abi, trace


Surface = collections.namedtuple("Surface", "tri t point normal inside")


def _scene_lib(scene, abi):
    """The library of an open scene of the HIP product, with the entry points of `abi` declared."""
    if not isinstance(scene, trace.Scene) or not scene._h:
        raise TypeError("scene must be an open trace.Scene")
    lib = scene._tl.lib
    try:
        if not scene._tl.backend().startswith("hip:"):
            raise AttributeError
        _abi._declare(lib, abi)
    except AttributeError:
        raise TypeError("device queries need a scene of the HIP library (backend %r)" % scene._tl.backend()) from None
    return lib


def _check(scene, rays, t_max):
    lib = _scene_lib(scene, _abi.QUERY_ABI)
    if not isinstance(rays, torch.Tensor) or not rays.is_cuda:
        raise TypeError("rays must be a GPU tensor")
    if rays.dtype != torch.float32:
        raise TypeError("rays must be float32, not %s" % rays.dtype)
    if rays.dim() < 1 or rays.shape[-1] != 6:
        raise ValueError("rays must have shape [..., 6], not %s" % (tuple(rays.shape),))
    if not rays.is_contiguous():
        raise ValueError("rays must be contiguous")
    if t_max is not None:
        if not isinstance(t_max, torch.Tensor) or not t_max.is_cuda:
            raise TypeError("t_max must be a GPU tensor")
        if t_max.dtype != torch.float32:
            raise TypeError("t_max must be float32, not %s" % t_max.dtype)
        if t_max.device != rays.device:
            raise ValueError("t_max is on %s, the rays on %s" % (t_max.device, rays.device))
        if tuple(t_max.shape) != tuple(rays.shape[:-1]):
            raise ValueError("t_max must have shape %s, not %s" % (tuple(rays.shape[:-1]), tuple(t_max.shape)))
        if not t_max.is_contiguous():
            raise ValueError("t_max must be contiguous")
    n = rays.numel() // 6
    if n > 2**31 - 1:
        raise ValueError("at most 2^31 - 1 rays per call")
    return lib, n


def _stream(rays, stream):
    """(raw handle, torch.cuda.Stream or None): the stream the query is enqueued on."""
    if stream is None:
        s = torch.cuda.current_stream(rays.device)
        return s.cuda_stream, s
    if isinstance(stream, torch.cuda.Stream):
        return stream.cuda_stream, stream
    return int(stream), None


def _keep(tensors, ts, rays):
    # the caching allocator must not hand these blocks out again before the query's stream is done with them
    if ts is not None and ts != torch.cuda.current_stream(rays.device):
        for x in tensors:
            if x is not None:
                x.record_stream(ts)


def _call(scene, rc):
    if rc != 0:
        raise trace.TraceError("%s (rc=%d)" % (scene._tl.lib.ezrt_last_error().decode(), rc))


def closest(scene, rays, t_max=None, stream=None):
    """(tri int32, t float32), each of shape rays.shape[:-1]: the reference's closest hit where it lies below t_max, else (-1, 114514)."""
    lib, n = _check(scene, rays, t_max)
    lead = tuple(rays.shape[:-1])
    tri = torch.empty(lead, dtype=torch.int32, device=rays.device)
    t = torch.empty(lead, dtype=torch.float32, device=rays.device)
    if n == 0:
        return tri, t
    h, ts = _stream(rays, stream)
    _call(scene, lib.ezrt_query_closest_device(scene._h, C.c_void_p(rays.data_ptr()),
                                               C.c_void_p(t_max.data_ptr()) if t_max is not None else None, n,
                                               C.c_void_p(tri.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(h)))
    _keep((rays, t_max, tri, t), ts, rays)
    return tri, t


def occluded(scene, rays, t_max=None, stream=None):
    """bool of shape rays.shape[:-1]: whether the ray hits a triangle at a distance below t_max (any distance without t_max)."""
    lib, n = _check(scene, rays, t_max)
    out = torch.empty(tuple(rays.shape[:-1]), dtype=torch.uint8, device=rays.device)
    if n == 0:
        return out.view(torch.bool)
    h, ts = _stream(rays, stream)
    _call(scene, lib.ezrt_query_occluded_device(scene._h, C.c_void_p(rays.data_ptr()),
                                                C.c_void_p(t_max.data_ptr()) if t_max is not None else None, n,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(h)))
    _keep((rays, t_max, out), ts, rays)
    return out.view(torch.bool)


_SURFACE_INTEGRATORS = (_abi.INTEGRATOR_P3_DIFFUSE, _abi.INTEGRATOR_P4_DISNEY, _abi.INTEGRATOR_P5_SOBOL, _abi.INTEGRATOR_P5_MIS,
                        _abi.INTEGRATOR_P5_MIS_ANISO)


def surface(scene, rays, t_max=None, integrator=_abi.INTEGRATOR_P5_SOBOL, stream=None):
    """Surface(tri, t, point, normal, inside): `closest` plus the reference's hitTriangle fields of each hit -- point = o + d * t
    (float32 [..., 3]), normal = the smooth shading normal, facing the ray's side (float32 [..., 3]), inside = the ray meets the
    triangle's back (bool).  `integrator` picks the form of the smooth normal as a render call does: 3 and 4 the chapter-3/4 form, 50,
    51 and 52 chapter 5's.  A miss gives zeros in point, normal and inside.  The winner's material is tri36[tri, 18:36]."""
    lib, n = _check(scene, rays, t_max)
    _abi._declare(lib, _abi.SURFACE_ABI)
    if integrator not in _SURFACE_INTEGRATORS:
        raise ValueError("integrator must be one of %s, not %r" % (_SURFACE_INTEGRATORS, integrator))
    lead = tuple(rays.shape[:-1])
    tri = torch.empty(lead, dtype=torch.int32, device=rays.device)
    t = torch.empty(lead, dtype=torch.float32, device=rays.device)
    point = torch.empty(lead + (3,), dtype=torch.float32, device=rays.device)
    normal = torch.empty(lead + (3,), dtype=torch.float32, device=rays.device)
    inside = torch.empty(lead, dtype=torch.uint8, device=rays.device)
    if n == 0:
        return Surface(tri, t, point, normal, inside.view(torch.bool))
    h, ts = _stream(rays, stream)
    P = C.c_void_p
    _call(scene, lib.ezrt_query_surface_device(scene._h, P(rays.data_ptr()), P(t_max.data_ptr()) if t_max is not None else None,
                                               n, int(integrator), P(tri.data_ptr()), P(t.data_ptr()), P(point.data_ptr()),
                                               P(normal.data_ptr()), P(inside.data_ptr()), P(h)))
    _keep((rays, t_max, tri, t, point, normal, inside), ts, rays)
    return Surface(tri, t, point, normal, inside.view(torch.bool))

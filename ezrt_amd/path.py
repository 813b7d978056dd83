"""Stream-ordered path queries on device tensors (include/ezrt_path.h): the render's primary rays, and radiance along any rays.

    rays = path.camera_rays(scene, params, xyf)                          # [..., 6] the primary rays a render call of `params` shoots
    rad = path.radiance(scene, rays, xyf, integrator=51, max_bounce=2)   # [..., 3] what the integrator returns along `rays`

`scene` is a `trace.Scene` of the HIP library; `params` an `EzrtRenderParams` (trace.make_params: width, height, eye and
camera_rotate are read); `xyf` a contiguous GPU tensor of shape [..., 3] holding uint32 values (ix, iy, frame) -- dtype torch.uint32,
or torch.int32 with the same bits: the PIXEL-SAMPLE whose random numbers an element uses, not where its ray points; `rays` a
contiguous float32 GPU tensor of shape xyf.shape[:-1] + (6,) (origin, direction; used as given, never normalised).  With
rays = camera_rays(scene, params, xyf) the radiance is, on the bits, the `colour` of `scene.render_paths` for those pixels and
frames; with rays of your own (a light map's texels, a probe's directions, another camera model) it is what the integrator would
have returned had the render shot them.  The work is enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle;
default: the current stream of the tensors' device) and the functions return without waiting for it.
"""
import ctypes as C

import torch

from . import _abi
from .query import _OnStream, _scene_lib
from .shade import _integrator, _tensor

_XYF_DTYPES = tuple(d for d in (getattr(torch, "uint32", None), torch.int32) if d is not None)


def _xyf(xyf, device=None):
    if not isinstance(xyf, torch.Tensor):
        raise TypeError("xyf must be a GPU tensor")
    if xyf.dtype not in _XYF_DTYPES:
        raise TypeError("xyf must be uint32 (or int32 holding the same bits), not %s" % xyf.dtype)
    return _tensor("xyf", xyf, xyf.dtype, last=3, device=device)


def camera_rays(scene, params, xyf, stream=None):
    """float32 xyf.shape[:-1] + (6,): (eye, direction) of the primary ray a render call of `params` shoots for pixel (ix, iy) of frame
    `frame`.  The pixel rect, the tiles and the shard of `params` are not applied, and ix / iy may lie beyond the frame."""
    lib = _scene_lib(scene, _abi.PATH_ABI)
    if not isinstance(params, _abi.EzrtRenderParams):
        raise TypeError("params must be an EzrtRenderParams (trace.make_params)")
    _xyf(xyf)
    rays = torch.empty(tuple(xyf.shape[:-1]) + (6,), dtype=torch.float32, device=xyf.device)
    n = xyf.numel() // 3
    if n > 0:
        _OnStream(scene, xyf, stream).run(lib.ezrt_camera_rays_device, C.byref(params), xyf, n, rays)
    return rays


def radiance(scene, rays, xyf, integrator=_abi.INTEGRATOR_P5_MIS, max_bounce=2, env_clamp=0.0, stream=None):
    """float32 rays.shape[:-1] + (3,): the colour the path tracing of `integrator` returns along each ray with `max_bounce` bounces and
    the environment clamped to `env_clamp` (> 0; else no clamp), with the random numbers of pixel-sample xyf.  A ray that misses
    gives the environment along it; max_bounce = 0 the emission of what it hits."""
    lib = _scene_lib(scene, _abi.PATH_ABI)
    integrator = _integrator(integrator)
    _tensor("rays", rays, torch.float32, last=6)
    _xyf(xyf, rays.device)
    if tuple(xyf.shape[:-1]) != tuple(rays.shape[:-1]):
        raise ValueError("xyf must have shape %s, not %s" % (tuple(rays.shape[:-1]) + (3,), tuple(xyf.shape)))
    if int(max_bounce) < 0:
        raise ValueError("max_bounce must not be negative")
    out = torch.empty(tuple(rays.shape[:-1]) + (3,), dtype=torch.float32, device=rays.device)
    n = rays.numel() // 6
    if n > 0:
        _OnStream(scene, rays, stream).run(lib.ezrt_query_radiance_device, integrator, int(max_bounce), float(env_clamp), rays, xyf, n, out)
    return out

"""Move a scene's triangles without re-creating it (include/ezrt_refit.h).

    refit.refit(scene, tri)              # new positions and normals into an open trace.Scene (HIP library), topology kept
    nodes2 = refit.refit_nodes(tri, nodes)   # the host definition: the caller's node arrays with every box recomputed

`tri` is the scene's triangle array with new vertices: shape (n_tri, 36) or (n_tri * 36,), float32, in the triangle order given to
scene_create.  Only floats 0-17 of each triangle (p1 p2 p3 n1 n2 n3) are read; the scene keeps its materials.  A GPU tensor on the
scene's device is read where it lies; a numpy array (or a CPU tensor) is copied to the scene's device first.  After refit() returns,
the scene answers every render and query exactly as `scene_create(tri, refit_nodes(tri, nodes))` would.  The call is synchronous: it
waits for the render calls and queries already issued on the scene, runs on `stream` (a torch.cuda.Stream or a raw hipStream_t;
default: the current stream of the scene's device) and returns once the scene is updated.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, trace
from .scene import refitBVH


def refit_nodes(tri, nodes):
    """The encoded node array [n_nodes, 12] with the box of every node but node 0 recomputed from the triangles' p1 p2 p3: a leaf's
    box is the builder's fold over its triangle range, an inner node's the union of its children's (ezrt_host_refit_nodes)."""
    return refitBVH(tri, nodes)


def _lib(scene):
    if not isinstance(scene, trace.Scene) or not scene._h:
        raise TypeError("scene must be an open trace.Scene")
    lib = scene._tl.lib
    try:
        if not scene._tl.backend().startswith("hip:"):
            raise AttributeError
        _abi._declare(lib, _abi.REFIT_ABI)
    except AttributeError:
        raise TypeError("a device refit needs a scene of the HIP library (backend %r)" % scene._tl.backend()) from None
    return lib


def refit(scene, tri, stream=None, device=None):
    """Refit `scene` to the triangle array `tri` (see the module docstring).  `device`: where a host array is copied to (default:
    the current CUDA device, which is the scene's when it was created there)."""
    lib = _lib(scene)
    if isinstance(tri, torch.Tensor) and tri.is_cuda:
        t = tri
    else:
        a = np.ascontiguousarray(tri.cpu().numpy() if isinstance(tri, torch.Tensor) else tri, np.float32)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        t = torch.from_numpy(a).to(dev)
        if stream is not None:
            torch.cuda.current_stream(dev).synchronize()  # the copy, before a refit on another stream reads it
    if t.dtype != torch.float32:
        raise TypeError("tri must be float32, not %s" % t.dtype)
    if not t.is_contiguous():
        raise ValueError("tri must be contiguous")
    if not (t.dim() == 2 and t.shape[1] == 36) and not (t.dim() == 1 and t.numel() % 36 == 0):
        raise ValueError("tri must have shape (n_tri, 36) or (n_tri * 36,), not %s" % (tuple(t.shape),))
    n = t.numel() // 36
    if stream is None:
        h = torch.cuda.current_stream(t.device).cuda_stream
    elif isinstance(stream, torch.cuda.Stream):
        h = stream.cuda_stream
    else:
        h = int(stream)
    rc = lib.ezrt_scene_refit_device(scene._h, C.c_void_p(t.data_ptr()), n, C.c_void_p(h))
    if rc != 0:
        raise trace.TraceError("%s (rc=%d)" % (lib.ezrt_last_error().decode(), rc))

"""Stream-ordered shading queries on device tensors (include/ezrt_shade.h): what lies behind a hit of `query.surface`.

    m = shade.material(scene, tri)                                   # [..., 18] the triangle's material floats
    f_r, pdf = shade.evaluate(scene, tri, V, N, L, integrator=51)    # what the surface reflects from L towards V, and L's pdf
    L = shade.sample(scene, tri, xi, V, N, integrator=51)            # the direction the integrator continues in
    colour, pdf = shade.env_evaluate(scene, L, env_clamp=0.0)        # the environment along L, and L's pdf under env_sample
    L = shade.env_sample(scene, xi)                                  # a direction drawn from the environment

`scene` is a `trace.Scene` of the HIP library; `tri` a contiguous int32 GPU tensor of any shape (triangle ids as `query.closest` /
`query.surface` return them; a miss, -1, gives zeros); V, N, L contiguous float32 GPU tensors of shape tri.shape + (3,), used as
given (never normalised): V points away from the surface (minus the ray direction), N is `query.surface`'s normal; xi float32
random numbers in [0, 1], tri.shape + (3,) for `sample` and [..., 2] for `env_sample`.  The outputs keep the leading dimensions.
Every value is what a render call of that integrator computes, on the bits.  The work is enqueued on `stream` (a
torch.cuda.Stream or a raw hipStream_t handle; default: the current stream of the tensors' device) and the functions return
without waiting for it.
"""
import torch

from . import _abi
from .query import _SURFACE_INTEGRATORS as INTEGRATORS
from .query import _OnStream, _scene_lib
from .query import _tensor as _query_tensor


def _tensor(name, x, dtype, shape=None, last=None, device=None):
    # query.py's checks, and a bound on the tensor as a whole
    return _query_tensor(name, x, dtype, shape, last, device, max_numel=2**31 - 1)


def _integrator(integrator):
    if integrator not in INTEGRATORS:
        raise ValueError("integrator must be one of %s, not %r" % (INTEGRATORS, integrator))
    return int(integrator)


def material(scene, tri, stream=None):
    """float32 tri.shape + (18,): the material floats of each triangle as given at scene creation (emissive, baseColor, subsurface,
    metallic, specular, specularTint, roughness, anisotropic, sheen, sheenTint, clearcoat, clearcoatGloss, IOR, transmission)."""
    lib = _scene_lib(scene, _abi.SHADE_ABI)
    _tensor("tri", tri, torch.int32)
    out = torch.empty(tuple(tri.shape) + (18,), dtype=torch.float32, device=tri.device)
    n = tri.numel()
    if n > 0:
        _OnStream(scene, tri, stream).run(lib.ezrt_query_material_device, tri, n, out)
    return out


def evaluate(scene, tri, V, N, L, integrator=_abi.INTEGRATOR_P5_MIS, want_pdf=True, stream=None):
    """(f_r float32 tri.shape + (3,), pdf float32 tri.shape or None): the BRDF value and the pdf of the direction L as the bounce loop
    of `integrator` computes them -- 3: baseColor / PI; 4: the anisotropic Disney BRDF; 50: the isotropic one (3, 4, 50: the
    constant pdf of the uniform hemisphere); 51 / 52: the isotropic / anisotropic BRDF with the pdf of its importance sampling."""
    lib = _scene_lib(scene, _abi.SHADE_ABI)
    integrator = _integrator(integrator)
    _tensor("tri", tri, torch.int32)
    v3 = tuple(tri.shape) + (3,)
    for name, x in (("V", V), ("N", N), ("L", L)):
        _tensor(name, x, torch.float32, v3, device=tri.device)
    f_r = torch.empty(v3, dtype=torch.float32, device=tri.device)
    pdf = torch.empty(tuple(tri.shape), dtype=torch.float32, device=tri.device) if want_pdf else None
    n = tri.numel()
    if n > 0:
        _OnStream(scene, tri, stream).run(lib.ezrt_shade_eval_device, integrator, tri, V, N, L, n, f_r, pdf)
    return f_r, pdf


def sample(scene, tri, xi, V, N, integrator=_abi.INTEGRATOR_P5_MIS, stream=None):
    """float32 tri.shape + (3,): the direction the bounce loop of `integrator` continues in for the random numbers xi -- 3, 4, 50: the
    uniform hemisphere about N (xi[..., 2] and V are not read); 51: the Disney BRDF's importance sampling; 52: its anisotropic form.
    The direction may point below the surface (the render ends such a path)."""
    lib = _scene_lib(scene, _abi.SHADE_ABI)
    integrator = _integrator(integrator)
    _tensor("tri", tri, torch.int32)
    v3 = tuple(tri.shape) + (3,)
    for name, x in (("xi", xi), ("V", V), ("N", N)):
        _tensor(name, x, torch.float32, v3, device=tri.device)
    L = torch.empty(v3, dtype=torch.float32, device=tri.device)
    n = tri.numel()
    if n > 0:
        _OnStream(scene, tri, stream).run(lib.ezrt_shade_sample_device, integrator, tri, xi, V, N, n, L)
    return L


def env_evaluate(scene, L, env_clamp=0.0, want_colour=True, want_pdf=True, stream=None):
    """(colour float32 L.shape or None, pdf float32 L.shape[:-1] or None): the environment's radiance along L (every channel clamped to
    env_clamp where that is > 0, as EzrtRenderParams.env_clamp) and the pdf of L under `env_sample`."""
    lib = _scene_lib(scene, _abi.SHADE_ABI)
    _tensor("L", L, torch.float32, last=3)
    if not want_colour and not want_pdf:
        raise ValueError("one of want_colour and want_pdf is required")
    colour = torch.empty(tuple(L.shape), dtype=torch.float32, device=L.device) if want_colour else None
    pdf = torch.empty(tuple(L.shape[:-1]), dtype=torch.float32, device=L.device) if want_pdf else None
    n = L.numel() // 3
    if n > 0:
        _OnStream(scene, L, stream).run(lib.ezrt_env_eval_device, L, n, float(env_clamp), colour, pdf)
    return colour, pdf


def env_sample(scene, xi, stream=None):
    """float32 xi.shape[:-1] + (3,): a direction per pair of random numbers, drawn from the environment's importance cache."""
    lib = _scene_lib(scene, _abi.SHADE_ABI)
    _tensor("xi", xi, torch.float32, last=2)
    L = torch.empty(tuple(xi.shape[:-1]) + (3,), dtype=torch.float32, device=xi.device)
    n = xi.numel() // 2
    if n > 0:
        _OnStream(scene, xi, stream).run(lib.ezrt_env_sample_device, xi, n, L)
    return L

"""The directional emitter on top of the C ABI (include/hf.h): ``DirectionalLight`` is the reference's
``directional`` (src/emitters/directional.cpp), a distant light of a given irradiance; ``directional_lighting`` is the
fused lighting row of a RIG of up to 8 of them (``hf_directional_lighting``: one launch, one image per light, the cast
shadows traced in the kernel) and ``directional_rays`` the shadow rays towards one light.  ``to_light`` and
``irradiance`` may be tensors of the user's graph or duals.  They are the emitter's host-side parameters
(hf_directional_light_t is host memory): expected as HOST tensors, read at every call.  ``direct_lighting`` (the caller's
visibility, constant lights) is unchanged.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check
from .shape import (_detached_f32, _empty_rays, _p3, _ptr, _ref, _row_ptrs, _stream_of, _value_outputs, _weighted_grads,
                    _weighted_tangents, _with_weight)

MAX_LIGHTS = 8
_WORKSPACES = {}


def _workspace(device):
    """the adjoint's workspace (4 numbers per light and block): one per (device, stream), kept, as the spot row's; sized
    for the largest rig"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_directional_workspace_floats(MAX_LIGHTS), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


def _host64(x):
    """a host-side parameter as a float64 host tensor that keeps the user's graph (or dual)"""
    if isinstance(x, torch.Tensor):
        return x.to(device="cpu", dtype=torch.float64)
    return torch.as_tensor(np.asarray(x, np.float64))


class DirectionalLight:
    """The ``directional`` emitter (src/emitters/directional.cpp): a distant light that delivers ``irradiance`` (W/m^2) to
    a surface facing it.  ``to_light`` points from the scene TOWARDS the light and may have any finite length > 0 (it is
    normalised once, in double; the outputs do not depend on its length); the reference's ``direction`` property is
    ``-to_light`` (``from_direction``).  Both parameters may be tensors of the user's graph or duals (host tensors, read
    at every call).  Out of scope: sample_ray, RGB."""

    def __init__(self, to_light, irradiance=1.0):
        self.to_light = to_light
        self.irradiance = irradiance

    @classmethod
    def from_direction(cls, direction, irradiance=1.0):
        """the reference's parameterisation: ``direction`` is the way the light travels, ``-to_light``"""
        d = direction if isinstance(direction, torch.Tensor) else torch.as_tensor(np.asarray(direction, np.float64))
        return cls(-d, irradiance)

    @property
    def to_light(self):
        return self._to_light

    @to_light.setter
    def to_light(self, v):
        """3 numbers; a tensor stays the user's (its graph, its dual), anything else becomes a float64 host tensor"""
        self._to_light = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float64))
        if self._to_light.numel() != 3:
            raise ValueError("DirectionalLight: to_light has 3 components (got %d)" % self._to_light.numel())
        n = float(torch.linalg.vector_norm(self._to_light.detach().to(dtype=torch.float64)))
        if not (np.isfinite(n) and n > 0.0):
            raise ValueError("DirectionalLight: to_light must have a finite length > 0 (got %r)" % (self._to_light.tolist(),))


def _rig(lights):
    """one DirectionalLight, a sequence of 1..8, or the [K, 4] tensor of direct_lighting (to_light, irradiance), as a
    tuple of lights; rows of a tensor stay views of it (its graph, its dual)"""
    if isinstance(lights, DirectionalLight):
        lights = (lights,)
    elif isinstance(lights, (torch.Tensor, np.ndarray)):
        rows = lights if isinstance(lights, torch.Tensor) else torch.as_tensor(np.asarray(lights, np.float64))
        if rows.dim() != 2 or rows.shape[1] != _capi.HF_DIRECTIONAL_PARAMS:
            raise ValueError("directional_lighting: a tensor of lights is [K, 4] (got %r)" % (tuple(rows.shape),))
        rows = _host64(rows)
        lights = tuple(DirectionalLight(r[:3], r[3]) for r in rows)
    else:
        lights = tuple(lights)
    if not 1 <= len(lights) <= MAX_LIGHTS or not all(isinstance(l, DirectionalLight) for l in lights):
        raise ValueError("directional_lighting: lights is one DirectionalLight, a sequence of 1..%d or a [K, 4] tensor (got %d)"
                         % (MAX_LIGHTS, len(lights)))
    return lights


def _stacked(lights):
    """the rig's parameters as one [K, 4] float64 host tensor, stacked with torch: autograd hands each light's own tensors
    their gradients (and forward mode their tangents)"""
    return torch.stack([torch.cat([_host64(l.to_light).reshape(3), _host64(l.irradiance).reshape(1)]) for l in lights])


def _structs(par):
    """the hf_directional_light_t array of the given (primal) [K, 4] parameters: host values"""
    L = (_capi.hf_directional_light_t * par.shape[0])()
    for k, q in enumerate(par.detach().tolist()):
        L[k] = _capi.hf_directional_light_t((C.c_double * 3)(*q[:3]), q[3])
    return L


class _DirectionalLightingOp(torch.autograd.Function):
    """(images [K, n / spp], per-sample values [K, n], visibility bytes) of hf_directional_lighting; backward =
    hf_directional_lighting_adjoint (gradients of sh_n, weight and the K x 4 parameters), jvp =
    hf_directional_lighting_tangent.  Both read the visibility byte the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, dd, tt, vis, *rest):
        """what hf_directional_lighting_adjoint / _tangent start with (rest: the weight if there is one)"""
        spp, L, K, albedo = ctx.misc
        ww = rest[-1] if ctx.weighted else None
        return (sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), K, L, albedo, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, weight, par, shape, p, nrm, d, t, albedo, spp):
        sn, pp, gn, dd, tt, ww = map(_detached_f32, (sh_n, p, nrm, d, t, weight))
        n, device, K = sn.shape[1], sn.device, par.shape[0]
        ctx.misc = (spp, _structs(par), K, albedo)
        image = torch.empty((K, n // max(spp, 1)), dtype=torch.float32, device=device)
        value = torch.empty((K, n), dtype=torch.float32, device=device)
        vis = torch.empty(n, dtype=torch.uint8, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_directional_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                      C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), K, ctx.misc[1], albedo,
                                                      image.data_ptr(), value.data_ptr(), vis.data_ptr(), _stream_of(device)))
        saved = _with_weight(ctx, (sn, dd, tt, vis), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, value, vis

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dpar, *_):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        # (held until the call has been enqueued)
        dl = dpar.detach().to(device=sn.device, dtype=torch.float32).contiguous() if dpar is not None else None
        dimage = torch.empty((K, sn.shape[1] // max(ctx.misc[0], 1)), dtype=torch.float32, device=sn.device)
        dvalue = torch.empty((K, sn.shape[1]), dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_directional_lighting_tangent(*_DirectionalLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                              _ptr(dw), _ptr(dl), dimage.data_ptr(), dvalue.data_ptr(),
                                                              _stream_of(sn.device)))
        return dimage, dvalue, None

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gv = _detached_f32(grad_value)
        reduced = ctx.needs_input_grad[2]
        gl = torch.zeros((K, _capi.HF_DIRECTIONAL_PARAMS), dtype=torch.float32, device=sn.device) if reduced else None
        if sn.shape[1]:
            check(_capi.lib().hf_directional_lighting_adjoint(*_DirectionalLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv),
                                                              C.byref(_p3(gn)), _ptr(gw), _ptr(gl),
                                                              _ptr(_workspace(sn.device)) if reduced else None,
                                                              _stream_of(sn.device)))
        gpar = gl.to(device="cpu", dtype=torch.float64) if reduced else None
        return (gn, gw, gpar) + (None,) * 7


def directional_lighting(shape, si, ray, lights, albedo=1.0, spp=1, weight=None, return_value=False, return_visibility=False):
    """Diffuse lighting under a rig of ``DirectionalLight``s + box-filter film, every light's shadow ray traced inside ONE
    lighting kernel (``hf_directional_lighting``): a sample that faces light k traces ``si.spawn_ray(l_k)`` and, where
    nothing is in the way, gets ``weight * albedo / pi * irradiance_k * <sh_n, l_k>`` with ``l_k`` the unit ``to_light``.
    ``lights``: one ``DirectionalLight``, a sequence of up to 8, or the [K, 4] tensor ``direct_lighting`` takes (a host
    tensor; it may require a gradient).  Returns the [K, n // spp] images; with ``return_value`` also the [K, n]
    per-sample values, with ``return_visibility`` the [n] uint8 row (bit k: lit by light k and unoccluded).
    Differentiable with respect to ``si.sh_frame.n``, ``weight`` ([n], optional) and every light's ``to_light`` and
    ``irradiance``, in reverse and forward mode; the visibility and the masks are held (the silhouette part of a moving
    shadow is the reparameterisation's business)."""
    shape._check_ray(ray)
    par = _stacked(_rig(lights))
    image, value, vis = _DirectionalLightingOp.apply(si.sh_frame.n, weight, par, shape, si.p, si.n, ray.d, si.t, float(albedo),
                                                     int(spp))
    return _value_outputs(image, value, vis, return_value, return_visibility)


def directional_rays(si, ray, light):
    """The shadow ray of every sample towards one ``DirectionalLight`` as a Ray3f (``hf_directional_rays``): what the
    fused kernel traces for that light, bit for bit, ``maxt = inf``.  Lanes it does not trace (no hit, seen from behind,
    facing away) get a zero origin and direction and ``maxt = -1``, a miss."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        L = _structs(_stacked(_rig(light)))
        check(_capi.lib().hf_directional_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                              tt.data_ptr(), L, C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(),
                                              _stream_of(pp.device)))
    return r

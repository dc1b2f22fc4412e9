"""Specular highlights on top of the C ABI (include/hf.h): ``specular_lighting`` is the GGX reflection lobe
of a rough surface (the reference's roughplastic / roughconductor ``eval``: F D G / (4 cos theta_i)) under the rig of
``directional_lighting``, for all lights in one launch (``hf_specular_lighting``).  It traces nothing: the visibility byte
of ``directional_lighting(..., return_visibility=True)`` is its mask, so a diffuse + specular image is two launches and
one shadow walk per light.  The lights are ``DirectionalLight``s, marshalled by directional.py's functions.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import ctypes as C
import math

import torch

from . import _capi
from ._capi import check
from .directional import MAX_LIGHTS, _rig, _stacked, _structs
from .shape import (_detached_f32, _glossy_alpha, _p3, _ptr, _ref, _row_ptrs, _stream_of, _weighted_grads, _weighted_tangents,
                    _with_weight)

_WORKSPACES = {}


def _workspace(device):
    """the adjoint's workspace (4 numbers per light and block): one per (device, stream), kept, as the directional row's;
    sized for the largest rig"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_specular_workspace_floats(MAX_LIGHTS), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


class _SpecularLightingOp(torch.autograd.Function):
    """(images [K, n / spp], per-sample values [K, n]) of hf_specular_lighting; backward = hf_specular_lighting_adjoint
    (gradients of sh_n, weight, alpha and the K x 4 parameters), jvp = hf_specular_lighting_tangent.  All three read the
    visibility byte and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, dd, al, vis, *rest):
        """what every hf_specular_* entry starts with (rest: the weight if there is one)"""
        spp, L, K, eta = ctx.misc
        ww = rest[-1] if ctx.weighted else None
        return (sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), _ptr(ww), al.data_ptr(), eta, K, L, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, weight, alpha, par, d, vis, eta, spp):
        sn, dd, ww, al = map(_detached_f32, (sh_n, d, weight, alpha))
        n, device, K = sn.shape[1], sn.device, par.shape[0]
        ctx.misc = (spp, _structs(par), K, eta)
        image = torch.empty((K, n // max(spp, 1)), dtype=torch.float32, device=device)
        value = torch.empty((K, n), dtype=torch.float32, device=device)
        saved = _with_weight(ctx, (sn, dd, al, vis), ww)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_specular_lighting(*_SpecularLightingOp._prefix(ctx, *saved), image.data_ptr(),
                                                   value.data_ptr(), _stream_of(device)))
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        return image, value

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dalpha, dpar, *_):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        da = _detached_f32(dalpha)
        # (held until the call has been enqueued)
        dl = dpar.detach().to(device=sn.device, dtype=torch.float32).contiguous() if dpar is not None else None
        dimage = torch.empty((K, sn.shape[1] // max(ctx.misc[0], 1)), dtype=torch.float32, device=sn.device)
        dvalue = torch.empty((K, sn.shape[1]), dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_specular_lighting_tangent(*_SpecularLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                           _ptr(dw), _ptr(da), _ptr(dl), dimage.data_ptr(), dvalue.data_ptr(),
                                                           _stream_of(sn.device)))
        return dimage, dvalue

    @staticmethod
    def backward(ctx, grad_image, grad_value):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gv = _detached_f32(grad_value)
        ga = torch.empty_like(sn[0]) if ctx.needs_input_grad[2] else None
        reduced = ctx.needs_input_grad[3]
        gl = torch.zeros((K, _capi.HF_DIRECTIONAL_PARAMS), dtype=torch.float32, device=sn.device) if reduced else None
        if sn.shape[1]:
            check(_capi.lib().hf_specular_lighting_adjoint(*_SpecularLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv),
                                                           C.byref(_p3(gn)), _ptr(gw), _ptr(ga), _ptr(gl),
                                                           _ptr(_workspace(sn.device)) if reduced else None,
                                                           _stream_of(sn.device)))
        gpar = gl.to(device="cpu", dtype=torch.float64) if reduced else None
        return (gn, gw, ga, gpar) + (None,) * 4


def specular_lighting(si, ray, lights, vis, alpha, eta=1.5, spp=1, weight=None, return_value=False):
    """Specular highlights under a rig of ``DirectionalLight``s + box-filter film, every light in ONE launch
    (``hf_specular_lighting``): where bit k of ``vis`` is set, a sample gets
    ``weight * irradiance_k * F(<wi, h>, eta) * D(<sh_n, h>, a) * G1(<sh_n, wi>, a) * G1(<sh_n, l_k>, a) / (4 <sh_n, wi>)``
    with ``wi = -ray.d``, ``l_k`` the unit ``to_light``, ``h`` the half vector, ``a = max(alpha, 1e-4)`` and the isotropic GGX
    distribution ``D``; exactly 0 elsewhere.  ``lights``: as ``directional_lighting`` takes them.  ``vis``: the [n] uint8 row
    of ``directional_lighting(..., return_visibility=True)`` (nothing is traced here).  ``alpha``: a float, a 0-d tensor or
    an [n] tensor (a scalar is expanded with torch, which then reduces its gradient).  ``eta``: the relative index of
    the interface, 0 an ideal mirror (F = 1).  Returns the [K, n // spp] images; with ``return_value`` also the [K, n]
    per-sample values.  Differentiable with respect to ``si.sh_frame.n``, ``weight`` ([n], optional), ``alpha`` and every
    light's ``to_light`` and ``irradiance``, in reverse and forward mode; ``vis`` and the masks are held."""
    sh_n = si.sh_frame.n
    n = sh_n.shape[1]
    if not isinstance(vis, torch.Tensor) or vis.dtype != torch.uint8 or vis.dim() != 1 or vis.shape[0] != n:
        raise ValueError("specular_lighting: vis is the [%d] uint8 row of directional_lighting(..., return_visibility=True)" % n)
    if vis.device != sh_n.device:
        raise ValueError("specular_lighting: vis must be on the wavefront's device")
    eta, spp = float(eta), int(spp)
    if not (math.isfinite(eta) and eta >= 0.0):
        raise ValueError("specular_lighting: eta must be finite and not negative (got %r)" % eta)
    if spp < 1 or n % spp:
        raise ValueError("specular_lighting: n (%d) must be a multiple of spp (%d)" % (n, spp))
    if weight is not None and weight.numel() != n:
        raise ValueError("specular_lighting: weight has %d elements (got %d)" % (n, weight.numel()))
    if ray.d.shape != sh_n.shape:
        raise ValueError("specular_lighting: ray.d must be [3, %d]" % n)
    par = _stacked(_rig(lights))
    image, value = _SpecularLightingOp.apply(sh_n, weight, _glossy_alpha(alpha, n, sh_n.device), par, ray.d, vis.contiguous(),
                                             eta, spp)
    return (image, value) if return_value else image

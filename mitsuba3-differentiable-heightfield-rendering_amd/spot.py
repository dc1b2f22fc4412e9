"""The spot emitter on top of the C ABI (include/hf.h): ``SpotLight`` is the reference's ``spot``
(src/emitters/spot.cpp), a point emitter whose intensity falls off linearly between ``beam_width`` and ``cutoff_angle``;
``spot_lighting`` is the fused lighting row of a RIG of up to 8 of them (``hf_spot_lighting``: one launch, one image per
light) and ``spot_rays`` the shadow rays towards one light.  ``to_world``, ``intensity``, ``cutoff_angle`` and
``beam_width`` may be tensors of the user's graph or duals.  They are the emitter's host-side parameters (hf_spot_light_t
is host memory): expected as HOST tensors, read at every call.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import ctypes as C

import numpy as np
import torch

from . import _capi, workload
from ._capi import check
from .shape import (_detached_f32, _empty_rays, _p3, _ptr, _ref, _row_ptrs, _stream_of, _value_outputs, _weighted_grads,
                    _weighted_tangents, _with_weight)

MAX_LIGHTS = 8
_WORKSPACES = {}


def _workspace(device):
    """the adjoint's workspace (15 numbers per light and block): one per (device, stream), kept, as the sensor's; sized
    for the largest rig"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_spot_workspace_floats(MAX_LIGHTS), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


def _host64(x):
    """a host-side parameter as a float64 host tensor that keeps the user's graph (or dual)"""
    if isinstance(x, torch.Tensor):
        return x.to(device="cpu", dtype=torch.float64)
    return torch.as_tensor(float(x), dtype=torch.float64)


class SpotLight:
    """The ``spot`` emitter (src/emitters/spot.cpp): a point at ``to_world``'s translation that shines along its z axis with
    ``intensity`` (W/sr) inside ``beam_width`` degrees of the axis, falling off linearly to 0 at ``cutoff_angle`` degrees;
    ``beam_width=None`` is 3/4 of the cutoff, the reference's default.  ``0 < beam_width <= cutoff_angle <= 180``;
    ``cutoff_angle = beam_width = 180`` is the reference's point light.  ``to_world``'s linear part must not scale.  Every
    parameter may be a tensor of the user's graph or a dual (host tensors, read at every call).  Out of scope: the
    ``texture`` parameter (a textured cone is ``Projector``'s business), sample_ray, RGB."""

    def __init__(self, to_world, intensity=1.0, cutoff_angle=20.0, beam_width=None):
        self.to_world = to_world
        self.intensity, self.cutoff_angle = intensity, cutoff_angle
        self.beam_width = cutoff_angle * 0.75 if beam_width is None else beam_width
        cut, beam = (float(x.detach()) if isinstance(x, torch.Tensor) else float(x) for x in (self.cutoff_angle, self.beam_width))
        if not (0.0 < beam <= cut <= 180.0):
            raise ValueError("SpotLight: 0 < beam_width <= cutoff_angle <= 180 degrees (got %r, %r)" % (beam, cut))

    @classmethod
    def look_at(cls, origin, target, up, **kw):
        return cls(workload.look_at(origin, target, up), **kw)

    @property
    def to_world(self):
        return self._to_world

    @to_world.setter
    def to_world(self, m):
        """3x4 or 4x4 (the last row is not read); a tensor stays the user's (its graph, its dual), anything else
        becomes a float64 host tensor"""
        self._to_world = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m, np.float64))
        assert self._to_world.numel() in (12, 16), "to_world is 3x4 or 4x4"


def _rig(lights):
    """one SpotLight or a sequence of 1..8 as a tuple"""
    lights = (lights,) if isinstance(lights, SpotLight) else tuple(lights)
    if not 1 <= len(lights) <= MAX_LIGHTS or not all(isinstance(l, SpotLight) for l in lights):
        raise ValueError("spot_lighting: lights is one SpotLight or a sequence of 1..%d (got %d)" % (MAX_LIGHTS, len(lights)))
    return lights


def _stacked(lights):
    """the rig's parameters as one [K, 12] and one [K, 3] float64 host tensor, stacked with torch: autograd hands each
    light's own tensors their gradients (and forward mode their tangents)"""
    tw = torch.stack([_host64(l.to_world).reshape(-1)[:12] for l in lights])
    par = torch.stack([torch.stack([_host64(x).reshape(()) for x in (l.intensity, l.cutoff_angle, l.beam_width)]) for l in lights])
    return tw, par


def _structs(tw, par):
    """the hf_spot_light_t array of the given (primal) [K, 12] and [K, 3] parameters: host values"""
    K = tw.shape[0]
    L = (_capi.hf_spot_light_t * K)()
    for k, (m, q) in enumerate(zip(tw.detach().tolist(), par.detach().tolist())):
        L[k] = _capi.hf_spot_light_t((C.c_double * 12)(*m), *q)
    return L


def _rows15(dtw, dpar, device):
    """jvp: the tangents of the stacked parameters as the [K, 15] float32 device rows of the C ABI (None: zero)"""
    if dtw is None and dpar is None:
        return None
    K = (dtw if dtw is not None else dpar).shape[0]
    out = torch.zeros((K, _capi.HF_SPOT_PARAMS), dtype=torch.float64)
    if dtw is not None:
        out[:, :12] = dtw.detach()
    if dpar is not None:
        out[:, 12:] = dpar.detach()
    return out.to(device=device, dtype=torch.float32).contiguous()


class _SpotLightingOp(torch.autograd.Function):
    """(images [K, n / spp], per-sample values [K, n], visibility bytes) of hf_spot_lighting; backward =
    hf_spot_lighting_adjoint (gradients of sh_n, p, weight and the K x 15 parameters), jvp = hf_spot_lighting_tangent.
    Both read the visibility byte the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, pp, dd, tt, vis, *rest):
        """what hf_spot_lighting_adjoint / _tangent start with (rest: the weight if there is one)"""
        spp, L, K, albedo = ctx.misc
        ww = rest[-1] if ctx.weighted else None
        return (sn.shape[1], spp, C.byref(_p3(pp)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), K, L, albedo,
                vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, p, weight, tw, par, shape, nrm, d, t, albedo, spp):
        sn, pp, gn, dd, tt, ww = map(_detached_f32, (sh_n, p, nrm, d, t, weight))
        n, device, K = sn.shape[1], sn.device, tw.shape[0]
        ctx.misc = (spp, _structs(tw, par), K, albedo)
        image = torch.empty((K, n // max(spp, 1)), dtype=torch.float32, device=device)
        value = torch.empty((K, n), dtype=torch.float32, device=device)
        vis = torch.empty(n, dtype=torch.uint8, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_spot_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                               C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), K, ctx.misc[1], albedo,
                                               image.data_ptr(), value.data_ptr(), vis.data_ptr(), _stream_of(device)))
        saved = _with_weight(ctx, (sn, pp, dd, tt, vis), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, value, vis

    @staticmethod
    def jvp(ctx, dsh_n, dp, dweight, dtw, dpar, *_):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dq, dl = _detached_f32(dp), _rows15(dtw, dpar, sn.device)  # (held until the call has been enqueued)
        dimage = torch.empty((K, sn.shape[1] // max(ctx.misc[0], 1)), dtype=torch.float32, device=sn.device)
        dvalue = torch.empty((K, sn.shape[1]), dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_spot_lighting_tangent(*_SpotLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                       _ref(_row_ptrs(dq)), _ptr(dw), _ptr(dl), dimage.data_ptr(),
                                                       dvalue.data_ptr(), _stream_of(sn.device)))
        return dimage, dvalue, None

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis):
        saved = ctx.saved_tensors
        sn, K = saved[0], ctx.misc[2]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gv, gp = _detached_f32(grad_value), torch.empty_like(sn)
        reduced = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        gl = torch.zeros((K, _capi.HF_SPOT_PARAMS), dtype=torch.float32, device=sn.device) if reduced else None
        if sn.shape[1]:
            check(_capi.lib().hf_spot_lighting_adjoint(*_SpotLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv),
                                                       C.byref(_p3(gn)), C.byref(_p3(gp)), _ptr(gw), _ptr(gl),
                                                       _ptr(_workspace(sn.device)) if reduced else None, _stream_of(sn.device)))
        gtw = gpar = None
        if reduced:
            host = gl.to(device="cpu", dtype=torch.float64)
            gtw, gpar = host[:, :12].contiguous(), host[:, 12:].contiguous()
        return (gn, gp, gw, gtw, gpar) + (None,) * 6


def spot_lighting(shape, si, ray, lights, albedo=1.0, spp=1, weight=None, return_value=False, return_visibility=False):
    """Diffuse lighting under a rig of ``SpotLight``s + box-filter film, every light's shadow ray traced inside ONE lighting
    kernel (``hf_spot_lighting``): a sample inside light k's cone that faces it traces ``si.spawn_ray_to(light origin)``
    and, where nothing is in the way, gets ``weight * albedo / pi * intensity_k * falloff * <sh_n, c - p> / |c - p|^3``.
    ``lights``: one ``SpotLight`` or a sequence of up to 8.  Returns the [K, n // spp] images; with ``return_value`` also the
    [K, n] per-sample values, with ``return_visibility`` the [n] uint8 row (bit k: lit by light k and unoccluded).
    Differentiable with respect to ``si.sh_frame.n``, ``si.p``, ``weight`` ([n], optional) and every light's ``to_world``,
    ``intensity``, ``cutoff_angle`` and ``beam_width``, in reverse and forward mode; the visibility, the masks and the branch
    of the falloff are held."""
    shape._check_ray(ray)
    tw, par = _stacked(_rig(lights))
    image, value, vis = _SpotLightingOp.apply(si.sh_frame.n, si.p, weight, tw, par, shape, si.n, ray.d, si.t, float(albedo), int(spp))
    return _value_outputs(image, value, vis, return_value, return_visibility)


def spot_rays(si, ray, light):
    """The shadow ray of every sample towards one ``SpotLight`` as a Ray3f (``hf_spot_rays``): what the fused kernel traces
    for that light, bit for bit, ``maxt`` just short of the light.  Lanes it does not trace (no hit, seen from behind,
    outside the cone, facing away) get ``maxt = -1``, a miss."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        L = _structs(*_stacked(_rig(light)))
        check(_capi.lib().hf_spot_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), L,
                                       C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(), _stream_of(pp.device)))
    return r

"""The projector emitter on top of the C ABI (include/hf.h): ``Projector`` is the reference's ``projector``
(src/emitters/projector.cpp), a pinhole that throws an irradiance texture onto the terrain -- structured light;
``projector_lighting`` is the fused lighting row (``hf_projector_lighting``) and ``projector_rays`` its shadow rays.
``to_world``, ``fov`` and ``scale`` may be tensors of the user's graph or duals.  They are the emitter's host-side
parameters (hf_projector_t is host memory): expected as HOST tensors, read at every call.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import ctypes as C

import numpy as np
import torch

from . import _capi, workload
from ._capi import check
from .sensor import _host_float, _scalar_grad, _scalar_like, _scalar_tangent
from .shape import (_WRAPS, Bitmap, _detached_f32, _empty_rays, _p3, _ptr, _ref, _row_ptrs, _stream_of, _texel_grad,
                    _texel_tangent, _tw_grad, _tw_like, _tw_tangent, _value_outputs, _weighted_grads, _weighted_tangents,
                    _with_weight)

_WORKSPACES = {}


def _workspace(device):
    """the adjoint's workspace (14 numbers per block): one per (device, stream), kept, as the sensor's"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_projector_workspace_floats(), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


class Projector:
    """The ``projector`` emitter (src/emitters/projector.cpp): a pinhole at ``to_world``'s translation that looks along
    its z axis with the horizontal field of view ``fov`` (degrees) and throws ``scale * irradiance`` onto the scene; the
    irradiance at distance 1 on the axis is ``scale * I``.  ``to_world``'s linear part must not scale.  ``irradiance``: a
    ``Bitmap`` (its own ``wrap`` is used) or a [TH, TW] float32 device tensor (``wrap``: ``"repeat"``, the reference's
    default, or ``"clamp"``), kept by reference -- it may require grad; None: uniform irradiance 1 with the aspect of
    ``resolution`` = (TW, TH) (default (1, 1)).  The frustum's aspect is TW / TH.  ``to_world``, ``fov`` and ``scale`` may be
    tensors of the user's graph or duals (host tensors, read at every call).  Out of scope: sample_ray, RGB, the other
    fov_axis values."""

    def __init__(self, to_world, fov, irradiance=None, scale=1.0, wrap="repeat", resolution=None):
        self.to_world = to_world
        self.fov, self.scale = fov, scale
        if isinstance(irradiance, Bitmap):
            irradiance, wrap = irradiance.data, irradiance.wrap
        if wrap not in _WRAPS:
            raise ValueError("Projector: wrap must be 'clamp' or 'repeat' (got %r)" % (wrap,))
        if irradiance is not None and (not isinstance(irradiance, torch.Tensor) or irradiance.dtype != torch.float32 or
                                       irradiance.dim() != 2 or irradiance.shape[0] < 1 or irradiance.shape[1] < 1):
            raise ValueError("Projector: irradiance must be a Bitmap or a float32 tensor [TH >= 1, TW >= 1]")
        if irradiance is not None and resolution is not None:
            raise ValueError("Projector: resolution is the texture's")
        self.irradiance, self.wrap = irradiance, wrap
        self._resolution = (1, 1) if resolution is None else (int(resolution[0]), int(resolution[1]))

    @classmethod
    def look_at(cls, origin, target, up, fov, **kw):
        return cls(workload.look_at(origin, target, up), fov, **kw)

    @property
    def to_world(self):
        return self._to_world

    @to_world.setter
    def to_world(self, m):
        """3x4 or 4x4 (the last row is not read); a tensor stays the user's (its graph, its dual), anything else
        becomes a float64 host tensor"""
        self._to_world = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m, np.float64))
        assert self._to_world.numel() in (12, 16), "to_world is 3x4 or 4x4"

    @property
    def resolution(self):
        """(TW, TH)"""
        return self._resolution if self.irradiance is None else (self.irradiance.shape[1], self.irradiance.shape[0])

    def _struct(self, to_world, fov, scale):
        """the hf_projector_t of the given (primal) parameters: host values, in double"""
        m = to_world.detach().to(device="cpu", dtype=torch.float64).reshape(-1)[:12].tolist()
        return _capi.hf_projector_t((C.c_double * 12)(*m), _host_float(fov), _host_float(scale))


def _texture_in(res, dat, wrap):
    """the texture's C arguments: TW, TH, tex (NULL: uniform), wrap"""
    return res[0], res[1], _ptr(dat), wrap


class _ProjectorLightingOp(torch.autograd.Function):
    """(image, per-sample value, visibility bytes, uv) of hf_projector_lighting; backward = hf_projector_lighting_adjoint
    (gradients of sh_n, p, weight, the texels, to_world, fov and scale), jvp = hf_projector_lighting_tangent.  Both read the
    visibility byte the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, pp, dd, tt, vis, *rest):
        """what hf_projector_lighting_adjoint / _tangent start with (rest: the texels if there are any, then the weight)"""
        spp, s, res, wrap, albedo = ctx.misc
        dat = rest[0] if ctx.textured else None
        ww = rest[-1] if ctx.weighted else None
        return (sn.shape[1], spp, C.byref(_p3(pp)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), C.byref(s),
                *_texture_in(res, dat, wrap), albedo, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, p, weight, texture, to_world, fov, scale, shape, nrm, d, t, proj, albedo, spp):
        sn, pp, gn, dd, tt, ww, dat = map(_detached_f32, (sh_n, p, nrm, d, t, weight, texture))
        n, device = sn.shape[1], sn.device
        ctx.misc = (spp, proj._struct(to_world, fov, scale), proj.resolution, _WRAPS[proj.wrap], albedo)
        ctx.textured = dat is not None
        ctx.likes = (_tw_like(to_world), _scalar_like(fov), _scalar_like(scale))
        image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=device)
        value = torch.empty(n, dtype=torch.float32, device=device)
        vis = torch.empty(n, dtype=torch.uint8, device=device)
        uv = torch.empty((2, n), dtype=torch.float32, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_projector_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                    C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), C.byref(ctx.misc[1]),
                                                    *_texture_in(ctx.misc[2], dat, ctx.misc[3]), albedo, image.data_ptr(),
                                                    value.data_ptr(), vis.data_ptr(), _ref(_row_ptrs(uv)), _stream_of(device)))
        saved = _with_weight(ctx, (sn, pp, dd, tt, vis) + ((dat,) if ctx.textured else ()), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis, uv)
        return image, value, vis, uv

    @staticmethod
    def jvp(ctx, dsh_n, dp, dweight, dtexture, dtw, dfov, dscale, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dq, df = _detached_f32(dp), _texel_tangent(dtexture if ctx.textured else None)  # (held until the call has been enqueued)
        d12, dfo, dsc = _tw_tangent(dtw, sn.device), _scalar_tangent(dfov, sn.device), _scalar_tangent(dscale, sn.device)
        dimage = torch.empty(sn.shape[1] // max(ctx.misc[0], 1), dtype=torch.float32, device=sn.device)
        dvalue = torch.empty_like(sn[0])
        if sn.shape[1]:
            check(_capi.lib().hf_projector_lighting_tangent(*_ProjectorLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                            _ref(_row_ptrs(dq)), _ptr(dw), _ptr(df), _ptr(d12), _ptr(dfo),
                                                            _ptr(dsc), dimage.data_ptr(), dvalue.data_ptr(),
                                                            _stream_of(sn.device)))
        return dimage, dvalue, None, None

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis, _grad_uv):
        saved = ctx.saved_tensors
        sn = saved[0]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gv, gp = _detached_f32(grad_value), torch.empty_like(sn)
        gd = _texel_grad(ctx, 3, saved[5]) if ctx.textured else None
        g12 = torch.zeros(12, dtype=torch.float32, device=sn.device) if ctx.needs_input_grad[4] else None
        gf, gs = (torch.zeros(1, dtype=torch.float32, device=sn.device) if ctx.needs_input_grad[j] else None for j in (5, 6))
        if sn.shape[1]:
            reduced = not (g12 is None and gf is None and gs is None)
            check(_capi.lib().hf_projector_lighting_adjoint(*_ProjectorLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv),
                                                            C.byref(_p3(gn)), C.byref(_p3(gp)), _ptr(gw), _ptr(gd), _ptr(g12),
                                                            _ptr(gf), _ptr(gs), _ptr(_workspace(sn.device)) if reduced else None,
                                                            _stream_of(sn.device)))
        return (gn, gp, gw, gd, _tw_grad(g12, ctx.likes[0]), _scalar_grad(gf, ctx.likes[1]),
                _scalar_grad(gs, ctx.likes[2])) + (None,) * 7


def projector_lighting(shape, si, ray, projector, albedo=1.0, spp=1, weight=None, return_value=False,
                       return_visibility=False, return_uv=False):
    """Diffuse lighting under a ``Projector`` + box-filter film, the shadow ray towards the pinhole traced inside the
    lighting kernel (``hf_projector_lighting``): every sample that the frustum covers and that faces the projector reads
    the irradiance texture where the pinhole maps it (``uv``: the perspective sensor's ``sample_direction`` in units of
    the film), traces ``si.spawn_ray_to(projector origin)`` and, where nothing is in the way, gets
    ``weight * albedo * scale * I(uv) * <sh_n, c - p> / ref.z^3`` (``ref``: the point in the projector's frame).  Returns
    the [n // spp] image; with ``return_value`` also the [n] per-sample values, with ``return_visibility`` the [n] uint8 row
    (1: lit and unoccluded) and with ``return_uv`` the [2, n] texture positions in [0, 1]^2 units (zeros behind the
    projector; detached).  Differentiable with respect to ``si.sh_frame.n``, ``si.p``, ``weight`` ([n], optional), the
    irradiance texels and the projector's ``to_world``, ``fov`` and ``scale``, in reverse and forward mode; the
    visibility, the masks and the cell of the lookup are held.  Several projectors: one call each."""
    shape._check_ray(ray)
    image, value, vis, uv = _ProjectorLightingOp.apply(si.sh_frame.n, si.p, weight, projector.irradiance, projector.to_world,
                                                       projector.fov, projector.scale, shape, si.n, ray.d, si.t, projector,
                                                       float(albedo), int(spp))
    out = _value_outputs(image, value, vis, return_value, return_visibility)
    if return_uv:
        out = (out if isinstance(out, tuple) else (out,)) + (uv,)
    return out


def projector_rays(si, ray, projector):
    """The shadow ray of every sample of ``projector_lighting`` as a Ray3f (``hf_projector_rays``): what the fused kernel
    traces, bit for bit, ``maxt`` just short of the pinhole.  Lanes it does not trace (no hit, seen from behind, outside
    the frustum, facing away) get ``maxt = -1``, a miss."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        s = projector._struct(projector.to_world, projector.fov, projector.scale)
        check(_capi.lib().hf_projector_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                            tt.data_ptr(), C.byref(s), *projector.resolution, C.byref(_p3(r.o)),
                                            C.byref(_p3(r.d)), r.maxt.data_ptr(), _stream_of(pp.device)))
    return r

"""The homogeneous medium on top of the C ABI (include/hf.h): ``Medium`` is the reference's ``homogeneous``
medium (src/media/homogeneous.cpp) with the ``hg`` phase function (src/phase/hg.cpp) filling the half space below a top
plane; ``medium_lighting`` is the fused single-scattering row under a rig of up to 8 ``DirectionalLight``s
(``hf_medium_lighting``: one launch, one image per light, 1..32 points per primary ray, their shadow rays traced in the
kernel), ``medium_rays`` the shadow rays of one point towards one light, and ``medium_attenuation`` the factor the
surface term of the same picture is multiplied by.  ``sigma_t``, ``albedo`` and ``g`` may be tensors of the user's graph
or duals.  They are host-side parameters (hf_medium_t is host memory): expected as HOST tensors, read at every call.

torch is used for device memory, streams and autograd plumbing only; the arithmetic of the row happens in the HIP
kernels (``medium_attenuation`` is a closed form in plain torch ops and needs none)."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check
from .directional import MAX_LIGHTS, _host64, _rig
from .shape import _check_ray_index, _detached_f32, _empty_rays, _p3, _ptr, _stream_of, _value_outputs, _with_weight

_WORKSPACES = {}


def _workspace(device):
    """the adjoint's workspace (a row of sums per block): one per (device, stream), kept, as the directional row's"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_medium_workspace_floats(MAX_LIGHTS), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


def _vec3(v, what):
    v = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float64).reshape(-1)
    if v.size != 3 or not np.isfinite(v).all():
        raise ValueError("Medium: %s has 3 finite components (got %r)" % (what, v.tolist()))
    return v


class Medium:
    """The ``homogeneous`` medium (src/media/homogeneous.cpp:139-175: ``sigma_s = albedo * sigma_t``) with the ``hg``
    phase function of asymmetry ``g`` (src/phase/hg.cpp), filling the half space below the plane through ``top_origin``
    with the normal ``top_normal`` (out of the medium, any finite length > 0).  ``sigma_t`` (> 0), ``albedo`` and ``g``
    (|g| < 1) may be tensors of the user's graph or duals (host tensors, read at every call); the plane is constant.
    Out of scope: a heterogeneous medium, RGB, emission, multiple scattering."""

    def __init__(self, sigma_t, albedo=0.75, g=0.0, top_origin=(0.0, 0.0, 1.0), top_normal=(0.0, 0.0, 1.0)):
        self.sigma_t, self.albedo, self.g = sigma_t, albedo, g
        self.top_origin, self.top_normal = _vec3(top_origin, "top_origin"), _vec3(top_normal, "top_normal")
        length = float(np.sqrt((self.top_normal ** 2).sum()))
        if not (np.isfinite(length) and length > 0.0):
            raise ValueError("Medium: top_normal must have a finite length > 0 (got %r)" % (self.top_normal.tolist(),))
        s, gg = float(_host64(sigma_t).detach()), float(_host64(g).detach())
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError("Medium: sigma_t must be finite and > 0 (got %r)" % (s,))
        if not abs(gg) < 1.0:
            raise ValueError("Medium: g must lie in (-1, 1) (got %r)" % (gg,))

    @property
    def unit_normal(self):
        return self.top_normal / np.sqrt((self.top_normal ** 2).sum())


def _stacked(medium, lights):
    """the row's differentiable scalars as one [3 + J] float64 host tensor (sigma_t, albedo, g, then every light's
    irradiance), stacked with torch: autograd hands each its gradient (and forward mode its tangent)"""
    return torch.stack([_host64(x).reshape(()) for x in (medium.sigma_t, medium.albedo, medium.g)] +
                       [_host64(l.irradiance).reshape(()) for l in lights])


def _structs(par, geometry, to_lights):
    """(hf_medium_t, the hf_directional_light_t array) of the given (primal) parameters: host values"""
    q = par.detach().tolist()
    M = _capi.hf_medium_t((C.c_double * 3)(*geometry[0]), (C.c_double * 3)(*geometry[1]), q[0], q[1], q[2])
    L = (_capi.hf_directional_light_t * len(to_lights))()
    for j, v in enumerate(to_lights):
        L[j] = _capi.hf_directional_light_t((C.c_double * 3)(*v), q[_capi.HF_MEDIUM_PARAMS + j])
    return M, L


def _geometry(medium, lights):
    return ((tuple(medium.top_origin.tolist()), tuple(medium.top_normal.tolist())),
            tuple(tuple(_host64(l.to_light).detach().reshape(3).tolist()) for l in lights))


class _MediumLightingOp(torch.autograd.Function):
    """(images [J, n / spp], per-sample values [J, n], visibility words [J, n]) of hf_medium_lighting; backward =
    hf_medium_lighting_adjoint (gradients of weight, t and the 3 + J scalars), jvp = hf_medium_lighting_tangent.  Both
    draw the points again, read the words the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, oo, dd, tt, vis, *rest):
        """what hf_medium_lighting_adjoint / _tangent start with (rest: the weight if there is one)"""
        spp, (M, L), J, num_steps, seed, rid = ctx.misc
        ww = rest[-1] if ctx.weighted else None
        return (oo.shape[1], spp, C.byref(_p3(oo)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), C.byref(M), J, L, num_steps, seed,
                _ptr(rid), vis.data_ptr())

    @staticmethod
    def forward(ctx, weight, t, par, shape, o, d, geometry, to_lights, spp, num_steps, seed, ray_index):
        oo, dd, tt, ww = map(_detached_f32, (o, d, t, weight))
        n, device, J = oo.shape[1], oo.device, len(to_lights)
        M, L = _structs(par, geometry, to_lights)
        ctx.misc = (spp, (M, L), J, num_steps, seed, ray_index)
        image = torch.empty((J, n // max(spp, 1)), dtype=torch.float32, device=device)
        value = torch.empty((J, n), dtype=torch.float32, device=device)
        vis = torch.empty((J, n), dtype=torch.int32, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_medium_lighting(shape._h, n, spp, C.byref(_p3(oo)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww),
                                                 C.byref(M), J, L, num_steps, seed, _ptr(ray_index), image.data_ptr(),
                                                 value.data_ptr(), vis.data_ptr(), _stream_of(device)))
        saved = _with_weight(ctx, (oo, dd, tt, vis), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, value, vis

    @staticmethod
    def jvp(ctx, dweight, dt, dpar, *_):
        saved = ctx.saved_tensors
        oo, J = saved[0], ctx.misc[2]
        dw, dtt = _detached_f32(dweight if ctx.weighted else None), _detached_f32(dt)
        # (held until the call has been enqueued)
        dp = dpar.detach().to(device=oo.device, dtype=torch.float32).contiguous() if dpar is not None else None
        dimage = torch.empty((J, oo.shape[1] // max(ctx.misc[0], 1)), dtype=torch.float32, device=oo.device)
        dvalue = torch.empty((J, oo.shape[1]), dtype=torch.float32, device=oo.device)
        if oo.shape[1]:
            check(_capi.lib().hf_medium_lighting_tangent(*_MediumLightingOp._prefix(ctx, *saved), _ptr(dw), _ptr(dtt), _ptr(dp),
                                                         dimage.data_ptr(), dvalue.data_ptr(), _stream_of(oo.device)))
        return dimage, dvalue, None

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis):
        saved = ctx.saved_tensors
        oo, tt, J = saved[0], saved[2], ctx.misc[2]
        gi, gv = _detached_f32(grad_image), _detached_f32(grad_value)
        gw = torch.zeros_like(tt) if ctx.weighted and ctx.needs_input_grad[0] else None
        gt = torch.zeros_like(tt) if ctx.needs_input_grad[1] else None
        reduced = ctx.needs_input_grad[2]
        gp = torch.zeros(_capi.HF_MEDIUM_PARAMS + J, dtype=torch.float32, device=oo.device) if reduced else None
        if oo.shape[1]:
            check(_capi.lib().hf_medium_lighting_adjoint(*_MediumLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv), _ptr(gw),
                                                         _ptr(gt), _ptr(gp), _ptr(_workspace(oo.device)) if reduced else None,
                                                         _stream_of(oo.device)))
        gpar = gp.to(device="cpu", dtype=torch.float64) if reduced else None
        return (gw, gt, gpar) + (None,) * 9


def medium_lighting(shape, si, ray, lights, medium, spp=1, num_steps=4, seed=0, weight=None, ray_index=None,
                    return_value=False, return_visibility=False):
    """Single scattering in a homogeneous ``Medium`` under a rig of ``DirectionalLight``s + box-filter film, every shadow
    ray traced inside ONE kernel (``hf_medium_lighting``): on the part of every primary ray inside the medium, up to
    ``si.t`` (``inf`` for a sample that missed the terrain: it takes part), ``num_steps`` (1..32) points are drawn in
    proportion to the transmittance from the TEA stream of ``sky_lighting`` (``seed``, ``ray_index``); every point traces
    a shadow ray towards every light that shines into the medium and, where nothing is in the way, gathers
    ``weight * albedo * a * p_hg * irradiance * exp(-optical depth up to the top) / num_steps``.  ``lights``: one
    ``DirectionalLight``, a sequence of up to 8, or the [J, 4] tensor ``directional_lighting`` takes.  Returns the
    [J, n // spp] images; with ``return_value`` also the [J, n] per-sample values, with ``return_visibility`` the [J, n]
    int32 words (bit k: point k sees light j).  Differentiable with respect to ``weight`` ([n], optional), ``si.t``
    (through which the gradient reaches the heights and ``to_world``), the medium's ``sigma_t``, ``albedo`` and ``g`` and
    every light's ``irradiance``, in reverse and forward mode; the visibility and the branch of the segment are held
    (the silhouette part of a moving shadow is the reparameterisation's business).  Not differentiated: ``to_light``,
    the top plane, the primary ray."""
    shape._check_ray(ray)
    rig = _rig(lights)
    par = _stacked(medium, rig)
    image, value, vis = _MediumLightingOp.apply(weight, si.t, par, shape, ray.o, ray.d, *_geometry(medium, rig), int(spp),
                                                int(num_steps), int(seed), _check_ray_index(ray_index, ray))
    return _value_outputs(image, value, vis, return_value, return_visibility)


def medium_rays(si, ray, light, medium, k, seed=0, ray_index=None):
    """Shadow ray ``k`` of every sample towards one ``DirectionalLight`` as a Ray3f (``hf_medium_rays``): what the fused
    kernel traces for that point and light, bit for bit, ``maxt = inf``; it starts on the primary ray, in free space.
    Lanes it does not trace (no part of the ray inside the medium, or a light that does not shine in) get a zero origin
    and direction and ``maxt = -1``, a miss."""
    oo, dd, tt = map(_detached_f32, (ray.o, ray.d, si.t))
    n, r = oo.shape[1], _empty_rays(oo)
    if n:
        rig = _rig(light)
        M, L = _structs(_stacked(medium, rig), *_geometry(medium, rig))
        check(_capi.lib().hf_medium_rays(n, C.byref(_p3(oo)), C.byref(_p3(dd)), tt.data_ptr(), C.byref(M), L, int(k), int(seed),
                                         _ptr(_check_ray_index(ray_index, ray)), C.byref(_p3(r.o)), C.byref(_p3(r.d)),
                                         r.maxt.data_ptr(), _stream_of(oo.device)))
    return r


def medium_attenuation(si, ray, lights, medium):
    """The [J, n] factors ``exp(-sigma_t (S_i + depth(p_i) / nu_j))`` of the samples that hit the terrain, 0 elsewhere:
    the transmittance along the part ``S_i`` of the primary ray inside the medium times the one from the hit point up to
    the top plane towards light j (``nu_j = <l_j, N>``; a light with ``nu_j <= 0`` does not shine in: zeros).  It is what
    multiplies ``directional_lighting``'s ``value[j]`` so that the surface term of the same picture is attenuated.
    Plain torch ops: autograd differentiates it with respect to ``si.t`` and ``sigma_t``; no kernel."""
    rig = _rig(lights)
    t = si.t
    dev, dt = t.device, t.dtype
    N = torch.as_tensor(medium.unit_normal, dtype=dt, device=dev)
    top = torch.as_tensor(medium.top_origin, dtype=dt, device=dev)
    sigma = _host64(medium.sigma_t).to(device=dev, dtype=dt)
    o, d = ray.o.detach().to(dt), ray.d.detach().to(dt)
    h = ((o - top[:, None]) * N[:, None]).sum(0)
    c = (d * N[:, None]).sum(0)
    hit = torch.isfinite(t) & (t > 0)
    ts = torch.where(hit, t, torch.zeros_like(t))
    inf = torch.full_like(ts, float("inf"))
    down, inside = c < 0, h < 0
    u_in = torch.where(down, torch.clamp(h / torch.where(down, -c, torch.ones_like(c)), min=0.0), torch.zeros_like(c))
    u_top = torch.where(inside & (c > 0), -h / torch.where(c > 0, c, torch.ones_like(c)), inf)
    u_out = torch.where(down | inside, torch.minimum(ts, u_top), torch.zeros_like(ts))
    S = torch.clamp(u_out - u_in, min=0.0)
    depth = torch.clamp(-(h + ts * c), min=0.0)
    rows = []
    for l in rig:
        v = _host64(l.to_light).detach().reshape(3)
        nu = float((v / torch.linalg.vector_norm(v) * torch.as_tensor(medium.unit_normal)).sum())
        rows.append(torch.where(hit, torch.exp(-sigma * (S + depth / nu)), torch.zeros_like(ts)) if nu > 0.0
                    else torch.zeros_like(ts))
    return torch.stack(rows)

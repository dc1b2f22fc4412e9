"""The sensor on top of the C ABI (include/hf.h): PerspectiveCamera and OrthographicCamera produce the
primary wavefront (``hf_sensor_rays``) and, for the perspective type, the film position of a world point
(``hf_sensor_project``: Sensor::sample_direction); ThinLensCamera is the perspective sensor with an aperture
(``hf_thinlens_rays``, ``hf_thinlens_project``).  Names and argument meaning follow src/sensors/perspective.cpp and
src/sensors/orthographic.cpp; ``to_world`` and ``fov`` may be tensors of the user's graph or duals.  They are the
sensor's host-side parameters (hf_sensor_t is host memory): expected as HOST tensors, read at every call.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import ctypes as C

import numpy as np
import torch

from . import _capi, workload
from ._capi import check
from .shape import Ray3f, _detached_f32, _p3, _ptr, _ref, _row_ptrs, _stream_of, _tw_grad, _tw_like, _tw_tangent


def _scalar_tangent(x, device):
    """the tangent of fov as one float32 device value (None: zero)"""
    return None if x is None else torch.as_tensor(x, device=device).detach().to(torch.float32).reshape(1).contiguous()


def _scalar_grad(g, like):
    """the device float of dL/dfov as a gradient of the user's fov tensor; None (not wanted) stays None"""
    if g is None:
        return None
    shape, dtype, device = like
    return g.reshape(shape).to(device=device, dtype=dtype)


_WORKSPACES = {}


def _workspace(device):
    """the adjoints' workspace: one per (device, stream), kept -- launches on one stream are ordered, so the next adjoint
    on it may reuse the block"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = torch.empty(_capi.lib().hf_sensor_workspace_floats(), dtype=torch.float32, device=device)
    return _WORKSPACES[key]


def _reduced(ctx, device, i_to_world=0, i_fov=1):
    """backward: the zeroed accumulators of dL/d(to_world) [12] and dL/dfov [1] for the inputs that need a gradient"""
    g12 = torch.zeros(12, dtype=torch.float32, device=device) if ctx.needs_input_grad[i_to_world] else None
    gf = torch.zeros(1, dtype=torch.float32, device=device) if ctx.needs_input_grad[i_fov] else None
    return g12, gf


class _SensorRaysOp(torch.autograd.Function):
    """(o, d, maxt, pos) of hf_sensor_rays; backward = hf_sensor_rays_adjoint (gradients of to_world and fov, reduced on
    the device without atomics), jvp = hf_sensor_rays_tangent.  maxt, the jitter and the pixel are held."""

    @staticmethod
    def _prefix(ctx):
        s, n, start, spp, seed, ray_id, _ = ctx.misc
        return C.byref(s), n, start, spp, seed, _ptr(ray_id)

    @staticmethod
    def forward(ctx, to_world, fov, cam, n, start, spp, seed, ray_id, device):
        ctx.misc = (cam._struct(to_world, fov), n, start, spp, seed, ray_id, device)
        ctx.tw_like = _tw_like(to_world)
        ctx.fov_like = _tw_like(fov) if isinstance(fov, torch.Tensor) else None
        o, d = (torch.empty((3, n), dtype=torch.float32, device=device) for _ in range(2))
        maxt = torch.empty(n, dtype=torch.float32, device=device)
        pos = torch.empty((2, n), dtype=torch.float32, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_sensor_rays(*_SensorRaysOp._prefix(ctx), C.byref(_p3(o)), C.byref(_p3(d)), maxt.data_ptr(),
                                             _ref(_row_ptrs(pos)), _stream_of(device)))
        ctx.mark_non_differentiable(maxt, pos)
        return o, d, maxt, pos

    @staticmethod
    def jvp(ctx, dtw, dfov, *_):
        n, device = ctx.misc[1], ctx.misc[6]
        d12, df = _tw_tangent(dtw, device), _scalar_tangent(dfov, device)
        do, dd = (torch.zeros((3, n), dtype=torch.float32, device=device) for _ in range(2))
        if n:
            check(_capi.lib().hf_sensor_rays_tangent(*_SensorRaysOp._prefix(ctx), _ptr(d12), _ptr(df), C.byref(_p3(do)),
                                                     C.byref(_p3(dd)), _stream_of(device)))
        return do, dd, None, None

    @staticmethod
    def backward(ctx, grad_o, grad_d, _grad_maxt, _grad_pos):
        n, device = ctx.misc[1], ctx.misc[6]
        go, gd = _detached_f32(grad_o), _detached_f32(grad_d)
        g12, gf = _reduced(ctx, device)
        if n and (g12 is not None or gf is not None):
            check(_capi.lib().hf_sensor_rays_adjoint(*_SensorRaysOp._prefix(ctx), _ref(_row_ptrs(go)), _ref(_row_ptrs(gd)),
                                                     _ptr(g12), _ptr(gf), _workspace(device).data_ptr(), _stream_of(device)))
        return (_tw_grad(g12, ctx.tw_like), _scalar_grad(gf, ctx.fov_like)) + (None,) * 7


class _SensorProjectOp(torch.autograd.Function):
    """(uv, valid bytes, weight) of hf_sensor_project; backward = hf_sensor_project_adjoint (gradients of to_world, fov
    and p), jvp = hf_sensor_project_tangent.  The masks are held."""

    @staticmethod
    def _prefix(ctx, pp):
        s, active = ctx.misc
        return C.byref(s), pp.shape[1], C.byref(_p3(pp)), _ptr(active)

    @staticmethod
    def forward(ctx, to_world, fov, p, cam, active):
        pp = _detached_f32(p)
        n, device = pp.shape[1], pp.device
        ctx.misc = (cam._struct(to_world, fov), active)
        ctx.tw_like = _tw_like(to_world)
        ctx.fov_like = _tw_like(fov) if isinstance(fov, torch.Tensor) else None
        uv = torch.zeros((2, n), dtype=torch.float32, device=device)
        valid = torch.zeros(n, dtype=torch.uint8, device=device)
        weight = torch.zeros(n, dtype=torch.float32, device=device)
        if n:
            check(_capi.lib().hf_sensor_project(*_SensorProjectOp._prefix(ctx, pp), C.byref(_row_ptrs(uv)), valid.data_ptr(),
                                                weight.data_ptr(), _stream_of(device)))
        ctx.save_for_backward(pp)
        ctx.save_for_forward(pp)
        ctx.mark_non_differentiable(valid)
        return uv, valid, weight

    @staticmethod
    def jvp(ctx, dtw, dfov, dp, *_):
        pp, = ctx.saved_tensors
        d12, df, dq = _tw_tangent(dtw, pp.device), _scalar_tangent(dfov, pp.device), _detached_f32(dp)
        duv, dweight = torch.zeros((2, pp.shape[1]), dtype=torch.float32, device=pp.device), torch.zeros_like(pp[0])
        if pp.shape[1]:
            check(_capi.lib().hf_sensor_project_tangent(*_SensorProjectOp._prefix(ctx, pp), _ref(_row_ptrs(dq)), _ptr(d12),
                                                        _ptr(df), C.byref(_row_ptrs(duv)), dweight.data_ptr(),
                                                        _stream_of(pp.device)))
        return duv, None, dweight

    @staticmethod
    def backward(ctx, grad_uv, _grad_valid, grad_weight):
        pp, = ctx.saved_tensors
        guv, gw = _detached_f32(grad_uv), _detached_f32(grad_weight)
        g12, gf = _reduced(ctx, pp.device)
        gp = torch.zeros_like(pp) if ctx.needs_input_grad[2] else None
        if pp.shape[1] and not (g12 is None and gf is None and gp is None):
            check(_capi.lib().hf_sensor_project_adjoint(*_SensorProjectOp._prefix(ctx, pp), _ref(_row_ptrs(guv)), _ptr(gw),
                                                        _ref(_row_ptrs(gp)), _ptr(g12), _ptr(gf),
                                                        _workspace(pp.device).data_ptr(), _stream_of(pp.device)))
        return _tw_grad(g12, ctx.tw_like), _scalar_grad(gf, ctx.fov_like), gp, None, None


class _Camera:
    """what both sensors share: the film with its crop window, the clip range, to_world and the wavefront"""
    _type = None

    def __init__(self, to_world, fov, film, near_clip, far_clip, crop):
        self.to_world = to_world
        self.fov = fov
        self.film = (int(film[0]), int(film[1]))
        self.crop = (0, 0) + self.film if crop is None else tuple(int(v) for v in crop)
        assert len(self.crop) == 4, "crop = (x, y, width, height)"
        self.near_clip, self.far_clip = float(near_clip), float(far_clip)

    @property
    def to_world(self):
        return self._to_world

    @to_world.setter
    def to_world(self, m):
        """3x4 or 4x4 (the last row is not read); a tensor stays the user's (its graph, its dual), anything else
        becomes a float64 host tensor"""
        self._to_world = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m, np.float64))
        assert self._to_world.numel() in (12, 16), "to_world is 3x4 or 4x4"

    def _struct(self, to_world, fov):
        """the hf_sensor_t of the given (primal) to_world and fov: host values, in double.  Both are read on the HOST at every
        call: keep them host tensors (the default); a device tensor works but makes every call wait for the device"""
        m = to_world.detach().to(device="cpu", dtype=torch.float64).reshape(-1)[:12].tolist()
        f = 0.0 if fov is None else float(fov.detach()) if isinstance(fov, torch.Tensor) else float(fov)
        return _capi.hf_sensor_t(self._type, self.film[0], self.film[1], *self.crop, (C.c_double * 12)(*m), f,
                                 self.near_clip, self.far_clip)

    def sample_rays(self, spp, seed=0, start=0, count=None, pixels=None, device="cuda"):
        """Samples [start, start + count) of the crop_w * crop_h * spp wavefront: ``(Ray3f, pos [2, n], ray_index)`` --
        the rays, their film positions in pixels of the whole film (what a reconstruction filter other than the box
        needs) and their indices in the full wavefront (int32: the ``ray_index`` of ``reparameterize_ray`` and of the
        lighting rows).  With ``pixels`` (int64 tensor of pixel indices y * crop_w + x of the crop window, one rank's
        list from ``workload.partition_tiles`` for instance) the result is the spp samples of exactly those pixels,
        pixel after pixel: the same rays, bit for bit, as in the full wavefront.  Differentiable with respect to
        ``to_world`` and ``fov`` in reverse and forward mode; maxt, the jitter and the pixel are held."""
        cw, ch = self.crop[2], self.crop[3]
        if pixels is not None:
            ray_index = workload.ray_indices(cw, ch, spp, device, pixels)
            start, n, ray_id = 0, int(ray_index.numel()), ray_index
        else:
            n = cw * ch * spp - start if count is None else int(count)
            ray_index, ray_id = torch.arange(start, start + n, dtype=torch.int64, device=device).to(torch.int32), None
        o, d, maxt, pos = _SensorRaysOp.apply(self.to_world, self.fov, self, n, int(start), int(spp), int(seed), ray_id,
                                              torch.device(device))
        ray = Ray3f.__new__(Ray3f)  # (o and d stay attached: the constructor would not change them either)
        ray.o, ray.d, ray.maxt, ray.time, ray.wavelengths = o, d, maxt, 0.0, None
        return ray, pos, ray_index


class PerspectiveCamera(_Camera):
    """The ``perspective`` sensor (src/sensors/perspective.cpp): a pinhole at ``to_world``'s translation that looks along
    its z axis with the horizontal field of view ``fov`` (degrees).  ``to_world``'s linear part must not scale.  ``film``
    = (width, height) in pixels, ``crop`` = (x, y, width, height) or None.  Out of scope: principal point offset,
    sample_border, ray differentials, wavelengths and time (the thin lens is ThinLensCamera)."""
    _type = _capi.HF_SENSOR_PERSPECTIVE

    def __init__(self, to_world, fov, film=(256, 256), near_clip=1e-2, far_clip=1e4, crop=None):
        super().__init__(to_world, fov, film, near_clip, far_clip, crop)

    @classmethod
    def look_at(cls, origin, target, up, fov, **kw):
        return cls(workload.look_at(origin, target, up), fov, **kw)

    def sample_direction(self, p, active=True):
        """The way back (Sensor::sample_direction): ``(uv [2, n], valid [n] bool, weight [n])`` of the world points
        ``p`` [3, n] -- the film position in pixels of the whole film (the ``pos`` of ``sample_rays``), whether the point
        is inside the clip range and the crop window, and importance / dist^2.  uv is written for every point inside the
        clip range (zeros elsewhere), weight is zero unless valid.  Differentiable with respect to ``p``, ``to_world``
        and ``fov`` in reverse and forward mode; the masks are held."""
        n = p.shape[1]
        if active is True or active is None:
            act = None
        else:
            act = torch.as_tensor(active, device=p.device).to(dtype=torch.uint8).expand(n).contiguous()
        uv, valid, weight = _SensorProjectOp.apply(self.to_world, self.fov, p, self, act)
        return uv, valid.bool(), weight


_LENS_WORKSPACES = {}


def _lens_workspace(device):
    """the thin lens's adjoints reduce 15 numbers where the sensor's reduce 13: a block of their own, kept as _workspace's"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _LENS_WORKSPACES:
        _LENS_WORKSPACES[key] = torch.empty(_capi.lib().hf_thinlens_workspace_floats(), dtype=torch.float32, device=device)
    return _LENS_WORKSPACES[key]


def _scalar_like(x):
    return _tw_like(x) if isinstance(x, torch.Tensor) else None


def _lens_reduced(ctx, device):
    """backward: the zeroed accumulators of dL/d(to_world) [12], dL/dfov, dL/dradius, dL/dfocus [1 each] for inputs 0..3
    that need a gradient"""
    g12 = torch.zeros(12, dtype=torch.float32, device=device) if ctx.needs_input_grad[0] else None
    return (g12,) + tuple(torch.zeros(1, dtype=torch.float32, device=device) if ctx.needs_input_grad[j] else None
                          for j in (1, 2, 3))


class _ThinLensRaysOp(torch.autograd.Function):
    """(o, d, maxt, pos) of hf_thinlens_rays; backward = hf_thinlens_rays_adjoint (gradients of to_world, fov,
    aperture_radius and focus_distance, reduced on the device without atomics), jvp = hf_thinlens_rays_tangent.  maxt, the
    jitter, the pixel and the disk point are held."""

    @staticmethod
    def _prefix(ctx):
        s, n, start, spp, seed, ray_id, _ = ctx.misc
        return C.byref(s), n, start, spp, seed, _ptr(ray_id)

    @staticmethod
    def forward(ctx, to_world, fov, radius, focus, cam, n, start, spp, seed, ray_id, device):
        ctx.misc = (cam._lens_struct(to_world, fov, radius, focus), n, start, spp, seed, ray_id, device)
        ctx.likes = (_tw_like(to_world), _scalar_like(fov), _scalar_like(radius), _scalar_like(focus))
        o, d = (torch.empty((3, n), dtype=torch.float32, device=device) for _ in range(2))
        maxt = torch.empty(n, dtype=torch.float32, device=device)
        pos = torch.empty((2, n), dtype=torch.float32, device=device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_thinlens_rays(*_ThinLensRaysOp._prefix(ctx), C.byref(_p3(o)), C.byref(_p3(d)), maxt.data_ptr(),
                                               _ref(_row_ptrs(pos)), _stream_of(device)))
        ctx.mark_non_differentiable(maxt, pos)
        return o, d, maxt, pos

    @staticmethod
    def jvp(ctx, dtw, dfov, dradius, dfocus, *_):
        n, device = ctx.misc[1], ctx.misc[6]
        d12 = _tw_tangent(dtw, device)
        df, dr, dfo = (_scalar_tangent(x, device) for x in (dfov, dradius, dfocus))
        do, dd = (torch.zeros((3, n), dtype=torch.float32, device=device) for _ in range(2))
        if n:
            check(_capi.lib().hf_thinlens_rays_tangent(*_ThinLensRaysOp._prefix(ctx), _ptr(d12), _ptr(df), _ptr(dr), _ptr(dfo),
                                                       C.byref(_p3(do)), C.byref(_p3(dd)), _stream_of(device)))
        return do, dd, None, None

    @staticmethod
    def backward(ctx, grad_o, grad_d, _grad_maxt, _grad_pos):
        n, device = ctx.misc[1], ctx.misc[6]
        go, gd = _detached_f32(grad_o), _detached_f32(grad_d)
        g = _lens_reduced(ctx, device)
        if n and any(x is not None for x in g):
            check(_capi.lib().hf_thinlens_rays_adjoint(*_ThinLensRaysOp._prefix(ctx), _ref(_row_ptrs(go)), _ref(_row_ptrs(gd)),
                                                       *(_ptr(x) for x in g), _lens_workspace(device).data_ptr(),
                                                       _stream_of(device)))
        return (_tw_grad(g[0], ctx.likes[0]),) + tuple(_scalar_grad(g[j], ctx.likes[j]) for j in (1, 2, 3)) + (None,) * 7


class _ThinLensProjectOp(torch.autograd.Function):
    """(uv, valid bytes, weight) of hf_thinlens_project; backward = hf_thinlens_project_adjoint (gradients of to_world,
    fov, aperture_radius, focus_distance and p), jvp = hf_thinlens_project_tangent.  The masks and the disk point are
    held."""

    @staticmethod
    def _prefix(ctx, pp):
        s, start, seed, ray_id, active = ctx.misc
        return C.byref(s), pp.shape[1], start, seed, _ptr(ray_id), C.byref(_p3(pp)), _ptr(active)

    @staticmethod
    def forward(ctx, to_world, fov, radius, focus, p, cam, start, seed, ray_id, active):
        pp = _detached_f32(p)
        n, device = pp.shape[1], pp.device
        ctx.misc = (cam._lens_struct(to_world, fov, radius, focus), start, seed, ray_id, active)
        ctx.likes = (_tw_like(to_world), _scalar_like(fov), _scalar_like(radius), _scalar_like(focus))
        uv = torch.zeros((2, n), dtype=torch.float32, device=device)
        valid = torch.zeros(n, dtype=torch.uint8, device=device)
        weight = torch.zeros(n, dtype=torch.float32, device=device)
        if n:
            check(_capi.lib().hf_thinlens_project(*_ThinLensProjectOp._prefix(ctx, pp), C.byref(_row_ptrs(uv)), valid.data_ptr(),
                                                  weight.data_ptr(), _stream_of(device)))
        ctx.save_for_backward(pp)
        ctx.save_for_forward(pp)
        ctx.mark_non_differentiable(valid)
        return uv, valid, weight

    @staticmethod
    def jvp(ctx, dtw, dfov, dradius, dfocus, dp, *_):
        pp, = ctx.saved_tensors
        d12, dq = _tw_tangent(dtw, pp.device), _detached_f32(dp)
        df, dr, dfo = (_scalar_tangent(x, pp.device) for x in (dfov, dradius, dfocus))
        duv, dweight = torch.zeros((2, pp.shape[1]), dtype=torch.float32, device=pp.device), torch.zeros_like(pp[0])
        if pp.shape[1]:
            check(_capi.lib().hf_thinlens_project_tangent(*_ThinLensProjectOp._prefix(ctx, pp), _ref(_row_ptrs(dq)), _ptr(d12),
                                                          _ptr(df), _ptr(dr), _ptr(dfo), C.byref(_row_ptrs(duv)),
                                                          dweight.data_ptr(), _stream_of(pp.device)))
        return duv, None, dweight

    @staticmethod
    def backward(ctx, grad_uv, _grad_valid, grad_weight):
        pp, = ctx.saved_tensors
        guv, gw = _detached_f32(grad_uv), _detached_f32(grad_weight)
        g = _lens_reduced(ctx, pp.device)
        gp = torch.zeros_like(pp) if ctx.needs_input_grad[4] else None
        if pp.shape[1] and not (gp is None and all(x is None for x in g)):
            check(_capi.lib().hf_thinlens_project_adjoint(*_ThinLensProjectOp._prefix(ctx, pp), _ref(_row_ptrs(guv)), _ptr(gw),
                                                          _ref(_row_ptrs(gp)), *(_ptr(x) for x in g),
                                                          _lens_workspace(pp.device).data_ptr(), _stream_of(pp.device)))
        return (_tw_grad(g[0], ctx.likes[0]),) + tuple(_scalar_grad(g[j], ctx.likes[j]) for j in (1, 2, 3)) + (gp,) + (None,) * 5


def _host_float(x):
    return float(x.detach()) if isinstance(x, torch.Tensor) else float(x)


class ThinLensCamera(_Camera):
    """The ``thinlens`` sensor (src/sensors/thinlens.cpp): the perspective sensor with an aperture of radius
    ``aperture_radius`` focused at ``focus_distance`` along its z axis -- depth of field.  ``aperture_radius = 0`` is the
    pinhole (the reference replaces 0 by an epsilon).  ``to_world``, ``fov``, ``aperture_radius`` and ``focus_distance``
    may be tensors of the user's graph or duals (host tensors, read at every call); the derivatives in the last two are
    an extension: the reference marks the thin lens's parameters NonDifferentiable.  Out of scope: ds.p / ds.d / ds.dist
    and the aperture pdf of sample_direction, ray differentials, wavelengths and time."""
    _type = _capi.HF_SENSOR_PERSPECTIVE

    def __init__(self, to_world, fov, aperture_radius, focus_distance, film=(256, 256), near_clip=1e-2, far_clip=1e4, crop=None):
        super().__init__(to_world, fov, film, near_clip, far_clip, crop)
        self.aperture_radius, self.focus_distance = aperture_radius, focus_distance

    @classmethod
    def look_at(cls, origin, target, up, fov, aperture_radius, focus_distance, **kw):
        return cls(workload.look_at(origin, target, up), fov, aperture_radius, focus_distance, **kw)

    def _lens_struct(self, to_world, fov, radius, focus):
        """the hf_thinlens_t of the given (primal) parameters: host values, in double"""
        return _capi.hf_thinlens_t(self._struct(to_world, fov), _host_float(radius), _host_float(focus))

    def sample_rays(self, spp, seed=0, start=0, count=None, pixels=None, device="cuda"):
        """As ``_Camera.sample_rays``: ``(Ray3f, pos [2, n], ray_index)``, the film positions those of the perspective
        sensor, every ray through its own point of the aperture (a second draw of the same seed).  Differentiable with
        respect to ``to_world``, ``fov``, ``aperture_radius`` and ``focus_distance`` in reverse and forward mode; maxt, the
        jitter, the pixel and the aperture point are held."""
        cw, ch = self.crop[2], self.crop[3]
        if pixels is not None:
            ray_index = workload.ray_indices(cw, ch, spp, device, pixels)
            start, n, ray_id = 0, int(ray_index.numel()), ray_index
        else:
            n = cw * ch * spp - start if count is None else int(count)
            ray_index, ray_id = torch.arange(start, start + n, dtype=torch.int64, device=device).to(torch.int32), None
        o, d, maxt, pos = _ThinLensRaysOp.apply(self.to_world, self.fov, self.aperture_radius, self.focus_distance, self, n,
                                                int(start), int(spp), int(seed), ray_id, torch.device(device))
        ray = Ray3f.__new__(Ray3f)  # (o and d stay attached: the constructor would not change them either)
        ray.o, ray.d, ray.maxt, ray.time, ray.wavelengths = o, d, maxt, 0.0, None
        return ray, pos, ray_index

    def sample_direction(self, p, ray_index=None, seed=0, start=0, active=True):
        """The way back (Sensor::sample_direction): ``(uv [2, n], valid [n] bool, weight [n])`` of the world points ``p``
        [3, n].  Point i is seen through the aperture point of the wavefront sample ``ray_index[i]`` (int32, as
        ``sample_rays`` returns it; None: ``start + i``) of ``seed``, so a point of sample i's ray projects to its
        ``pos``.  Differentiable with respect to ``p`` and the four parameters; the masks and the aperture point are held."""
        n = p.shape[1]
        if active is True or active is None:
            act = None
        else:
            act = torch.as_tensor(active, device=p.device).to(dtype=torch.uint8).expand(n).contiguous()
        rid = None if ray_index is None else ray_index.to(device=p.device, dtype=torch.int32).contiguous()
        uv, valid, weight = _ThinLensProjectOp.apply(self.to_world, self.fov, self.aperture_radius, self.focus_distance, p, self,
                                                     int(start), int(seed), rid, act)
        return uv, valid.bool(), weight


class OrthographicCamera(_Camera):
    """The ``orthographic`` sensor (src/sensors/orthographic.cpp): parallel rays along ``to_world``'s z axis from the
    image of [-1, 1] x [-1 / aspect, 1 / aspect] under ``to_world`` (whose scale sets the size of the view).  It has no
    ``sample_direction``: the reference has none, and a point names no film position of a sensor whose pixel integral is
    over the ray origins."""
    _type = _capi.HF_SENSOR_ORTHOGRAPHIC

    def __init__(self, to_world, film=(256, 256), near_clip=1e-2, far_clip=1e4, crop=None):
        super().__init__(to_world, None, film, near_clip, far_clip, crop)

    @classmethod
    def look_at(cls, origin, target, up, scale=(1.0, 1.0, 1.0), **kw):
        """look_at(origin, target, up) times scale(scale): the sensor of ``workload.ortho_rays``"""
        return cls(workload.look_at(origin, target, up) @ np.diag([scale[0], scale[1], scale[2], 1.0]), **kw)

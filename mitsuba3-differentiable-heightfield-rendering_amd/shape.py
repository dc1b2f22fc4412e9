"""Host-side mirror of the reference's Shape plugin interface for the heightfield
hot path, on top of the C ABI (include/hf.h).  Names, argument meaning and error
behaviour follow include/mitsuba/render/shape.h:137-183 and its Python surface
src/render/python/shape_v.cpp:51-102; the data types follow
include/mitsuba/core/ray.h:24-82 and include/mitsuba/render/interaction.h.

torch is used for device memory, streams and autograd plumbing only; all
arithmetic happens in the HIP kernels of libhf.so.  There is no CPU fallback.
"""
import ctypes as C
import enum
import math

import torch
import torch.autograd.forward_ad as fwAD

from . import _capi
from ._capi import check, hf_desc_t, hf_pi_t, hf_position_sample_t, hf_rays_t, hf_si_grad_t, hf_si_t, hf_si_tangent_t


class RayFlags(enum.IntFlag):
    """include/mitsuba/render/interaction.h:19-69"""
    Empty = 0x0
    Minimal = 0x1
    UV = 0x2
    dPdUV = 0x4
    ShadingFrame = 0x8
    dNGdUV = 0x10
    dNSdUV = 0x20
    BoundaryTest = 0x40
    FollowShape = 0x80
    DetachShape = 0x100
    All = 0x2 | 0x4 | 0x8
    AllNonDifferentiable = 0x2 | 0x4 | 0x8 | 0x100
    # libhf extension (include/hf.h HF_RAY_BOUNDARY_ALL_EDGES): boundary_test over all three triangle edges (the
    # reference Mesh's semantics) instead of the silhouette edges only
    BoundaryAllEdges = 0x10000


class ParamFlags(enum.IntFlag):
    """include/mitsuba/render/fwd / object.h ParamFlags"""
    Differentiable = 0x0
    NonDifferentiable = 0x1
    Discontinuous = 0x2


def _as_f32(x, device):
    t = torch.as_tensor(x, dtype=torch.float32, device=device)
    return t.contiguous()


# ---- marshalling: what every call into libhf builds its arguments with -------------------------------------------------
def _ptr(x):
    """address of a device tensor or a host (numpy) array; None stays None (a NULL argument)"""
    if x is None:
        return None
    return x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data


def _ref(c):
    """C.byref of a ctypes array or struct; None stays None"""
    return None if c is None else C.byref(c)


def _row_addrs(x):
    """addresses of the rows of a [k, n] array: a device tensor, a row or column slice of one (row slices of
    [3, n] tensors are rows of m floats: no copies), or a host (numpy) array"""
    if isinstance(x, torch.Tensor):
        # (an empty tensor has the address 0, and so have its rows)
        base, step = x.data_ptr(), x.stride(0) * x.element_size() if x.numel() else 0
    else:
        base, step = x.ctypes.data, x.strides[0]
    return [base + step * k for k in range(x.shape[0])]


def _row_ptrs(x, k=None):
    """ctypes array of the row pointers of a [k, n] array (see _row_addrs), NULL-padded to k entries; None stays None"""
    if x is None:
        return None
    addrs = _row_addrs(x)
    return (C.c_void_p * (k or len(addrs)))(*addrs)


def _rows(buf, n):
    """device addresses of the rows of a contiguous [k, n] float32 tensor"""
    return _row_addrs(buf)


def _p3(x):
    """ctypes array of the 3 row pointers of a [3, n] tensor"""
    return _row_ptrs(x)


def _f3(x):
    """[3, n] float32 device tensor -> (keepalive, ctypes array of 3 row pointers)"""
    x = x.to(dtype=torch.float32).contiguous()
    return x, _p3(x)


def _fill(struct, layout, addrs):
    """set the pointer fields of a ctypes struct, named by layout = [(field, rows), ...], to consecutive addresses"""
    k = 0
    for name, c in layout:
        if c == 1:
            setattr(struct, name, addrs[k])
        else:
            arr = getattr(struct, name)
            for j in range(c):
                arr[j] = addrs[k + j]
        k += c
    return struct


def _stream_of(device):
    """the current stream of `device` as the hf_stream_t of the C ABI"""
    return torch.cuda.current_stream(device).cuda_stream


def _tangent(x, shape, device, what, exc=AssertionError):
    """a tangent or an upstream gradient as a contiguous float32 device tensor of `shape`; None (zero) stays None.
    A wrong number of values raises `exc`: AssertionError from the Heightfield methods, ValueError from the
    reparameterisation entries."""
    if x is None:
        return None
    x = torch.as_tensor(x, device=device).detach().to(torch.float32).contiguous()
    if x.numel() != math.prod(shape):
        raise exc(f"{what}: expected {math.prod(shape)} values, got {x.numel()}")
    return x.reshape(shape)


def _tw_tangent(dtw, device=None, exc=AssertionError):
    """a 3x4 / 4x4 (last row dropped) / 12-value tangent of to_world as the 12 contiguous float32 device values of the
    C ABI (None: zero)"""
    if dtw is None:
        return None
    dtw = torch.as_tensor(dtw, device=device).detach().reshape(-1)
    return _tangent(dtw[:12] if dtw.numel() == 16 else dtw, (12,), dtw.device, "d_to_world", exc)


def _tw_like(to_world):
    """(shape, dtype, device) of a to_world input, None without one"""
    return None if to_world is None else (tuple(to_world.shape), to_world.dtype, to_world.device)


def _tw_grad(grad12, like):
    """the 12 floats of dL/d(to_world) as a gradient of the user's 3x4 / 4x4 tensor (a 4x4's last row gets zeros);
    None (not wanted) stays None"""
    if grad12 is None:
        return None
    shape, dtype, device = like
    g = grad12.reshape(3, 4)
    if shape[0] == 4:
        g = torch.cat([g, torch.zeros((1, 4), dtype=g.dtype, device=g.device)])
    return g.reshape(shape).to(device=device, dtype=dtype)


def _grad12(grad_tw):
    """a caller's dL/d(to_world) accumulator as the C ABI takes it: 12 contiguous float32 device values (or None)"""
    assert grad_tw is None or (grad_tw.numel() == 12 and grad_tw.dtype == torch.float32 and grad_tw.is_contiguous())
    return grad_tw


def _has_tangent(x):
    """a forward-mode AD tangent is attached to x (torch.autograd.forward_ad; False outside a dual level)"""
    return isinstance(x, torch.Tensor) and fwAD.unpack_dual(x).tangent is not None


# ---- what the height / to_world differentiable ops share: each op below states its inputs, C calls and return tuple ----
_STALE = {"jvp": "heightfield parameters changed between the primal and the tangent pass",
          "backward": "heightfield parameters changed between forward and backward"}


def _op_save(ctx, shape, tensors, to_world=None):
    """forward: keep `tensors` for both derivative passes, stamp the parameter version, remember to_world's layout"""
    ctx.shape = shape
    ctx.save_for_backward(*tensors)
    ctx.save_for_forward(*tensors)
    ctx.h_version = shape._param_version()
    ctx.tw_like = _tw_like(to_world)


def _op_saved(ctx, which):
    """jvp / backward: (shape, saved tensors), refused when the parameters changed since the primal pass"""
    if ctx.h_version != ctx.shape._param_version():
        raise RuntimeError(_STALE[which])
    return ctx.shape, ctx.saved_tensors


def _op_grads(ctx, i_heights, i_to_world):
    """backward: zeroed accumulators (dL/dheight [H, W], dL/d(to_world) [12]) for the inputs that need a gradient"""
    shape = ctx.shape
    grad_h = shape._zero_heights() if ctx.needs_input_grad[i_heights] else None
    grad_tw = torch.zeros(12, dtype=torch.float32, device=shape.device) if ctx.needs_input_grad[i_to_world] else None
    return grad_h, grad_tw


class Ray3f:
    """SoA ray wavefront: o, d as [3, n] float32 tensors, maxt [n] (default +inf,
    i.e. dr::Largest, ray.h:37).  time / wavelengths are carried but unused."""

    def __init__(self, o, d, maxt=None, time=0.0, wavelengths=None):
        dev = o.device if isinstance(o, torch.Tensor) else (d.device if isinstance(d, torch.Tensor) else "cuda")
        self.o = _as_f32(o, dev)
        self.d = _as_f32(d, dev)
        if self.o.dim() == 1:
            self.o = self.o.reshape(3, 1)
        if self.d.dim() == 1:
            self.d = self.d.reshape(3, 1)
        n = max(self.o.shape[1], self.d.shape[1])
        if self.o.shape[1] != n:
            self.o = self.o.expand(3, n).contiguous()
        if self.d.shape[1] != n:
            self.d = self.d.expand(3, n).contiguous()
        assert self.o.shape == (3, n) and self.d.shape == (3, n), "Ray3f expects [3, n] SoA tensors"
        if maxt is None:
            self.maxt = torch.full((n,), math.inf, dtype=torch.float32, device=self.o.device)
        else:
            self.maxt = _as_f32(maxt, self.o.device).reshape(-1)
            if self.maxt.numel() == 1 and n != 1:
                self.maxt = self.maxt.expand(n).contiguous()
        self.time = time
        self.wavelengths = wavelengths

    def __len__(self):
        return self.o.shape[1]

    def __call__(self, t):
        """ray(t) = fmadd(d, t, o), ray.h:57"""
        return torch.addcmul(self.o, self.d, t)

    @property
    def device(self):
        return self.o.device


class Frame3f:
    def __init__(self, s, t, n):
        self.s, self.t, self.n = s, t, n

    def to_local(self, v):
        return torch.stack([(v * self.s).sum(0), (v * self.t).sum(0), (v * self.n).sum(0)])


class PreliminaryIntersection3f:
    """interaction.h:587-691"""

    def __init__(self, t, prim_uv, prim_index, shape):
        self.t = t
        self.prim_uv = prim_uv
        self.prim_index = prim_index
        # (uint32_t) -1 for a non-instanced shape (rectangle.cpp:222)
        self.shape_index = torch.full_like(prim_index, -1)
        self.shape = shape
        self.instance = None

    def is_valid(self):
        return self.t != math.inf

    def compute_surface_interaction(self, ray, ray_flags=RayFlags.All, active=True):
        """interaction.h:658-684: shape->compute_surface_interaction + finalize."""
        return self.shape.compute_surface_interaction(ray, self, ray_flags, 0, active)


class SurfaceInteraction3f:
    """interaction.h:175-507 (fields of DRJIT_STRUCT :504-506 that a static shape fills)"""

    def __init__(self):
        self.t = self.p = self.n = self.uv = None
        self.sh_frame = None
        self.dp_du = self.dp_dv = self.dn_du = self.dn_dv = None
        self.duv_dx = self.duv_dy = None
        self.wi = None
        self.prim_index = None
        self.boundary_test = None
        self.shape = None
        self.instance = None
        self.time = 0.0
        self.wavelengths = None
        self.ray_flags = None        # the RayFlags the record was computed with (None: not known)

    def is_valid(self):
        return self.t != math.inf

    def spawn_ray(self, d):
        """Semi-infinite ray from the interaction towards ``d`` ([3] or [3, n]); the origin is offset along
        the detached normal by (1 + max|p|) * RayEpsilon, signed by <n, d> (interaction.h:134-136, 161-165;
        RayEpsilon = 1500 * eps/2, math.h:18-22)."""
        d = torch.as_tensor(d, dtype=torch.float32, device=self.p.device)
        if d.dim() == 1:
            d = d[:, None].expand(3, self.p.shape[1])
        p, n = self.p.detach(), self.n.detach()
        mag = (1.0 + p.abs().max(0).values) * (1500.0 * 5.9604644775390625e-08)
        mag = torch.where((n * d).sum(0) < 0, -mag, mag)
        o = torch.addcmul(p, mag[None, :], n)
        maxt = torch.full((p.shape[1],), math.inf, dtype=torch.float32, device=p.device)
        return Ray3f(o.contiguous(), d.contiguous(), maxt)


def _device_copy(dst, src, nbytes):
    """synchronous device-to-device copy through the HIP runtime libhf is linked against (test accessors only)"""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    if hip.hipMemcpy(dst, src, nbytes, 3) != 0:   # hipMemcpyDeviceToDevice
        raise RuntimeError("hipMemcpy failed")


class PositionSample3f:
    """include/mitsuba/render/records.h PositionSample: p, n ([3, n]), uv ([2, n]), time, pdf ([n]), delta.  The
    heightfield also records the sampled triangle (prim_index) and its barycentrics b ([2, n]: b1, b2)."""

    def __init__(self, p, n, uv, time, pdf, delta=False):
        self.p, self.n, self.uv, self.time, self.pdf, self.delta = p, n, uv, time, pdf, delta
        self.prim_index = self.b = None


class DirectionSample3f(PositionSample3f):
    """records.h DirectionSample: a PositionSample plus the unit direction d from the reference point and the
    distance dist"""

    def __init__(self, ps, d, dist):
        super().__init__(ps.p, ps.n, ps.uv, ps.time, ps.pdf, ps.delta)
        self.prim_index, self.b = ps.prim_index, ps.b
        self.d, self.dist = d, dist


class _SamplePositionOp(torch.autograd.Function):
    """Differentiable [6, n] block (p, n) of sample_position; backward = hf_sample_position_adjoint (atomic scatter of
    dL/dheight), jvp = hf_sample_position_tangent.  The sampled triangle and b are frozen (detached, as build_pmf).
    to_world (differentiable_to_world shapes, else None): hf_sample_position_adjoint_transform / _tangent_transform."""

    @staticmethod
    def forward(ctx, shape, heights, prim, b, active, block, to_world=None):
        _op_save(ctx, shape, (prim, b), to_world)
        ctx.active = active
        return block

    @staticmethod
    def jvp(ctx, _shape, dh, _prim, _b, _active, _block, dtw=None):
        shape, (prim, b) = _op_saved(ctx, "jvp")
        return shape._sample_tangent_raw(prim, b, ctx.active, dh, dtw)

    @staticmethod
    def backward(ctx, g):
        shape, (prim, b) = _op_saved(ctx, "backward")
        grad_h, grad_tw = _op_grads(ctx, 1, 6)
        if grad_h is not None or grad_tw is not None:
            shape._sample_adjoint_raw(prim, b, ctx.active, g.contiguous().to(torch.float32), grad_h, grad_tw)
        return None, grad_h, None, None, None, None, _tw_grad(grad_tw, ctx.tw_like)


class _AttributeOp(torch.autograd.Function):
    """Differentiable value [size, n] of eval_attribute*; backward = hf_eval_attribute_adjoint (atomic scatter into the
    attribute buffer and the heights, dL/dp per lane), jvp = hf_eval_attribute_tangent.  Inputs: the attribute buffer,
    si.p (vertex attributes; the gradient of p then reaches hf_adjoint through _SurfaceInteractionOp) and the heights."""

    @staticmethod
    def forward(ctx, shape, name, attr, p, heights, prim, t, active, value):
        p = p.detach().contiguous() if p is not None else None
        _op_save(ctx, shape, (attr.detach(), p, prim, t))
        ctx.name, ctx.active = name, active
        return value

    @staticmethod
    def jvp(ctx, _shape, _name, dattr, dp, dh, *_):
        shape, (attr, p, prim, t) = _op_saved(ctx, "jvp")
        return shape._attr_tangent_raw(ctx.name, attr, p, prim, t, ctx.active, dattr, dp, dh)

    @staticmethod
    def backward(ctx, g):
        shape, (attr, p, prim, t) = _op_saved(ctx, "backward")
        need_a, need_p, need_h = ctx.needs_input_grad[2], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        ga, gp, gh = shape._attr_adjoint_raw(ctx.name, attr, p, prim, t, ctx.active, g.contiguous().to(torch.float32),
                                             need_a, need_p, need_h)
        return None, None, ga, gp, gh, None, None, None, None


# order of the differentiable SI block handed to autograd: 18 rows
_DIFF_ROWS = [("t", 1), ("p", 3), ("n", 3), ("uv", 2), ("sh_n", 3), ("dp_du", 3), ("dp_dv", 3)]
_AUX_ROWS = [("boundary_test", 1), ("sh_s", 3), ("sh_t", 3), ("wi", 3)]
# the pointer fields of hf_rays_t, hf_pi_t and hf_position_sample_t, in the order _fill takes their addresses
_RAY_ROWS = [("o", 3), ("d", 3), ("maxt", 1)]
_PI_ROWS = [("t", 1), ("prim_uv", 2), ("prim_index", 1)]
_SAMPLE_ROWS = [("p", 3), ("n", 3), ("uv", 2), ("pdf", 1), ("prim_index", 1), ("b", 2)]


class _SurfaceInteractionOp(torch.autograd.Function):
    """Differentiable SI block [18, n]; backward = hf_adjoint (atomic scatter of dL/dheight), jvp = hf_tangent.
    to_world (differentiable_to_world shapes, else None): hf_adjoint_transform / hf_tangent_transform."""

    @staticmethod
    def forward(ctx, shape, heights, o, d, maxt, t, uv, prim, flags, active, diff_block, to_world=None):
        _op_save(ctx, shape, (o, d, maxt, t, uv, prim), to_world)
        ctx.flags, ctx.active = flags, active
        return diff_block

    @staticmethod
    def jvp(ctx, _shape, dh, do, dd, _maxt, _t, _uv, _prim, _flags, _active, _diff, dtw=None):
        shape, saved = _op_saved(ctx, "jvp")
        return shape._tangent_raw(*saved, ctx.flags, ctx.active, dh, do, dd, dtw)

    @staticmethod
    def backward(ctx, g):
        shape, saved = _op_saved(ctx, "backward")
        n = saved[0].shape[1]
        need_o, need_d = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        grad_h, grad_tw = _op_grads(ctx, 1, 11)
        grad_od = torch.empty((6, n), dtype=torch.float32, device=shape.device) if (need_o or need_d) else None
        shape._adjoint_raw(*saved, ctx.flags, ctx.active, g.contiguous().to(torch.float32), grad_h, grad_od,
                           grad_tw=grad_tw)
        go = grad_od[0:3] if need_o else None
        gd = grad_od[3:6] if need_d else None
        return None, grad_h, go, gd, None, None, None, None, None, None, None, _tw_grad(grad_tw, ctx.tw_like)


class _ParameterizationOp(torch.autograd.Function):
    """Differentiable SI block [18, n] of eval_parameterization; backward = hf_eval_parameterization_adjoint (atomic
    scatter of dL/dheight), jvp = hf_eval_parameterization_tangent.  The triangle and its barycentrics are recomputed
    from uv by the derivative entries and frozen; the t and uv rows carry no derivative.  to_world
    (differentiable_to_world shapes, else None): dL/d(to_world) through the same entries."""

    @staticmethod
    def forward(ctx, shape, heights, uv, flags, active, diff_block, to_world=None):
        _op_save(ctx, shape, (uv,), to_world)
        ctx.flags, ctx.active = flags, active
        return diff_block

    @staticmethod
    def jvp(ctx, _shape, dh, _uv, _flags, _active, _diff, dtw=None):
        shape, (uv,) = _op_saved(ctx, "jvp")
        return shape._param_tangent_raw(uv, ctx.flags, ctx.active, dh, dtw)

    @staticmethod
    def backward(ctx, g):
        shape, (uv,) = _op_saved(ctx, "backward")
        grad_h, grad_tw = _op_grads(ctx, 1, 6)
        if grad_h is not None or grad_tw is not None:
            shape._param_adjoint_raw(uv, ctx.flags, ctx.active, g.contiguous().to(torch.float32), grad_h, grad_tw)
        return None, grad_h, None, None, None, None, _tw_grad(grad_tw, ctx.tw_like)


class Heightfield:
    """`heightfield` shape plugin mirror.

    Properties (build decision, SURVEY.md section 8a -- the reference snapshot has no
    heightfield plugin): `heightfield` ([H, W] or [H, W, 1] tensor, row 0 at object
    y = -1; cf. TensorXf(data, 3, {H,W,C}) in src/textures/bitmap.cpp:262),
    `max_height`, `to_world` (3x4 / 4x4 affine), `flip_normals`, `face_normals`.
    `face_normals` is Mesh's property (src/render/mesh.cpp:30) but defaults to True (flat shading), where Mesh's
    defaults to False: a heightfield shades flat unless smooth shading is asked for (hf_set_face_normals).
    Object space is Rectangle's: x,y in [-1,1], +Z up (src/shapes/rectangle.cpp:47-48).
    Properties named `vertex_*` ([H, W, C] or [H, W] tensor) or `face_*` ([2 (H-1)(W-1), C] tensor) become shape
    attributes (add_attribute).
    """

    def __init__(self, props=None, **kw):
        props = dict(props or {}, **kw)
        props.pop("type", None)
        hfield = props.pop("heightfield")
        self.max_height = float(props.pop("max_height", 1.0))
        to_world = props.pop("to_world", None)
        self.flip_normals = bool(props.pop("flip_normals", False))
        face_normals = bool(props.pop("face_normals", True))
        # to_world Differentiable | Discontinuous (rectangle.cpp:128) instead of NonDifferentiable; off by default
        self.differentiable_to_world = bool(props.pop("differentiable_to_world", False))
        device = props.pop("device", None)
        attr_props = [(k, props.pop(k)) for k in sorted(props) if k.startswith(("vertex_", "face_"))]
        if props:
            raise RuntimeError(f"Unreferenced properties: {sorted(props)}")  # Properties semantics
        if not torch.cuda.is_available():
            raise RuntimeError("Heightfield: no HIP device available (libhf has no CPU fallback)")
        if device is None:
            device = hfield.device if isinstance(hfield, torch.Tensor) and hfield.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        h = torch.as_tensor(hfield, dtype=torch.float32)
        if h.dim() == 3 and h.shape[2] == 1:
            h = h[:, :, 0]
        if h.dim() != 2:
            raise RuntimeError("heightfield: expected a [H, W] or [H, W, 1] tensor")
        self.height, self.width = int(h.shape[0]), int(h.shape[1])
        tw = torch.eye(4, dtype=torch.float64)[:3] if to_world is None else torch.as_tensor(to_world, dtype=torch.float64).cpu()
        tw = tw.reshape(-1)[:12].reshape(3, 4)
        self.to_world = tw.to(torch.float32)
        self._to_world_in, self._to_world_version = self.to_world, 0
        desc = hf_desc_t()
        desc.width, desc.height = self.width, self.height
        desc.max_height = self.max_height
        for k, v in enumerate(self.to_world.reshape(-1).tolist()):
            desc.to_world[k] = v
        desc.has_to_object = 0
        desc.flip_normals = int(self.flip_normals)
        desc.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        handle = C.c_void_p()
        check(_capi.lib().hf_create(C.byref(desc), C.byref(handle)))  # HF_EINVAL if H or W < 2
        self._h = handle
        self._dirty = True
        self._heights_version = 0
        # the differentiable parameter (put_parameter("heightfield", ..., Differentiable|Discontinuous))
        self.heightfield = h.to(self.device).contiguous().clone()
        self.parameters_changed(["heightfield"])
        self.face_normals = True
        self.set_face_normals(face_normals)
        # shape attributes (Mesh::m_mesh_attributes): name -> flat float32 buffer [count * size] (interleaved), and
        # name -> (HF_ATTR_VERTEX / HF_ATTR_FACE, size)
        self.attributes, self._attr_meta = {}, {}
        for name, data in attr_props:
            data = torch.as_tensor(data, dtype=torch.float32)
            if name.startswith("vertex_"):
                size = 1 if data.dim() == 2 else int(data.shape[-1])
                if tuple(data.shape[:2]) != (self.height, self.width):
                    raise RuntimeError(f"{name}: expected a [{self.height}, {self.width}, C] tensor, got {tuple(data.shape)}")
            else:
                size = 1 if data.dim() == 1 else int(data.shape[-1])
            self.add_attribute(name, size, data)

    # ---- lifetime ---------------------------------------------------------------------
    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _capi.lib().hf_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- parameter plumbing (shape.cpp:536-570, rectangle.cpp:126-142) ---------------
    def traverse(self, callback):
        callback.put_parameter("heightfield", self.heightfield, ParamFlags.Differentiable | ParamFlags.Discontinuous)
        callback.put_parameter("max_height", self.max_height, ParamFlags.NonDifferentiable)
        callback.put_parameter("to_world", self.to_world, ParamFlags.Differentiable | ParamFlags.Discontinuous
                               if self.differentiable_to_world else ParamFlags.NonDifferentiable)
        for name, buf in self.attributes.items():   # mesh.cpp:74-76: every attribute is shown as differentiable
            callback.put_parameter(name, buf, ParamFlags.Differentiable)

    def parameters_changed(self, keys=()):
        keys = list(keys)
        for name, (type_, size) in getattr(self, "_attr_meta", {}).items():   # every attribute, whatever the keys
            expected = size * self._attr_count(type_)
            buf = self.attributes[name]
            if buf.numel() != expected:   # mesh.cpp:103-110: an attribute of the wrong size is reset to zeros
                self.attributes[name] = torch.zeros(expected, dtype=torch.float32, device=self.device)
            elif buf.dtype != torch.float32 or buf.device != self.device or not buf.is_contiguous() or buf.dim() != 1:
                self.attributes[name] = buf.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if not keys or "heightfield" in keys:
            h = self.heightfield
            if h.dim() == 3 and h.shape[2] == 1:
                h = h[:, :, 0]
            if tuple(h.shape) != (self.height, self.width):
                # bitmap.cpp:272-286: resolution may not change / must stay >= 2
                raise RuntimeError(f"heightfield: tensor shape {tuple(h.shape)} != ({self.height}, {self.width})")
            hd = h.detach().to(device=self.device, dtype=torch.float32).contiguous()
            check(_capi.lib().hf_set_heights(self._h, hd.data_ptr(), self._stream()))
            self._heights_keepalive = hd
            self._heights_version += 1
        if not keys or "to_world" in keys:
            tw = (C.c_float * 12)(*self.to_world.detach().reshape(-1)[:12].tolist())
            check(_capi.lib().hf_set_transform(self._h, tw, None))
            # the tensor the kernels now use: the autograd input of every differentiable op until the next change
            self._to_world_in = self.to_world
            self._to_world_version += 1
        self.mark_dirty()

    def _param_version(self):
        """what a differentiable op checks between its primal and its derivative pass: the heights' version and, for
        differentiable_to_world shapes, the transform's"""
        return (self._heights_version, self._to_world_version if self.differentiable_to_world else 0)

    def _to_world_live(self, detach=False):
        """the to_world tensor the ops take as an input when a derivative is wanted with respect to it, else None"""
        if not self.differentiable_to_world or detach:
            return None
        tw = self._to_world_in
        if not isinstance(tw, torch.Tensor):
            return None
        if _has_tangent(tw) or (torch.is_grad_enabled() and tw.requires_grad):
            return tw
        return None

    def _wants_derivative(self, *tensors, detach=False):
        """a derivative is wanted with respect to one of `tensors`, the heights or to_world: a forward-mode tangent
        (torch.autograd.forward_ad, whatever the grad mode) or requires_grad with grad mode on.  detach
        (RayFlags.DetachShape): the heights and to_world do not count, `tensors` (the rays) still do."""
        live = tensors if detach else (*tensors, self.heightfield)
        if any(_has_tangent(x) or (torch.is_grad_enabled() and x.requires_grad) for x in live):
            return True
        return self._to_world_live(detach) is not None

    def _zero_heights(self):
        """a zeroed dL/dheight accumulator [H, W]"""
        return torch.zeros((self.height, self.width), dtype=torch.float32, device=self.device)

    def _dheights(self, dh, exc=AssertionError):
        """a tangent of the heights for the C ABI: one float32 per height (None: zero)"""
        return _tangent(dh, (self.height, self.width), self.device, "dheights", exc)

    def set_face_normals(self, face_normals):
        """Flat (True) or smooth (False) shading.  Smooth: angle-weighted vertex normals, rebuilt with every
        parameters_changed, interpolated into sh_frame.n and differentiated through (hf_set_face_normals)."""
        check(_capi.lib().hf_set_face_normals(self._h, 1 if face_normals else 0, self._stream()))
        self.face_normals = bool(face_normals)
        self.mark_dirty()

    def shading_derivatives(self, pi, active=True):
        """dn_du, dn_dv ([3, n] each) of the hits of `pi`: the derivatives of the shading normal with respect to the
        barycentrics (mesh.cpp:818-829, RayFlags.dNSdUV); zero for misses and with flat shading.  Not differentiable."""
        n = pi.t.shape[0]
        keep, _ = self._mask(active, n)
        out = torch.empty((6, n), dtype=torch.float32, device=self.device)
        pis = self._pi_struct(pi.t.detach().contiguous(), pi.prim_uv.detach().contiguous(), pi.prim_index.contiguous())
        check(_capi.lib().hf_shading_derivatives(self._h, n, C.byref(pis), _ptr(keep), C.byref(_p3(out[0:3])),
                                                 C.byref(_p3(out[3:6])), self._stream()))
        return out[0:3], out[3:6]

    # ---- area sampling (Mesh::build_pmf / sample_position / pdf_position, mesh.cpp:401-432, 552-642) ----------------
    def ensure_pmf_built(self):
        """mesh.cpp ensure_pmf_built: the area table is enabled on first use (hf_set_area_sampling); from then on every
        parameters_changed / Adam step rebuilds it with the heights"""
        if not getattr(self, "_area_enabled", False):
            check(_capi.lib().hf_set_area_sampling(self._h, 1, self._stream()))
            self._area_enabled = True

    def _area_scalars(self):
        self.ensure_pmf_built()
        area, norm = C.c_float(), C.c_float()
        check(_capi.lib().hf_surface_area(self._h, C.byref(area), C.byref(norm)))
        return area.value, norm.value

    def surface_area(self):
        """mesh.cpp:552-555: the sum of the triangle areas (m_area_pmf.sum(), float32)"""
        return self._area_scalars()[0]

    def area_cdf(self):
        """the area table's float32 CDF ([2 (W-1) (H-1)] device tensor, a copy; hf_area_cdf)"""
        self.ensure_pmf_built()
        ptr, cnt = C.c_void_p(), C.c_size_t()
        check(_capi.lib().hf_area_cdf(self._h, C.byref(ptr), C.byref(cnt)))
        out = torch.empty(cnt.value, dtype=torch.float32, device=self.device)
        if cnt.value:
            torch.cuda.current_stream(self.device).synchronize()   # the last rebuild, on this stream
            _device_copy(out.data_ptr(), ptr.value, 4 * cnt.value)
        return out

    def sample_position(self, time, sample, active=True):
        """mesh.cpp:557-610 (hf_sample_position): sample [2, n] in [0, 1).  p and n are differentiable in the
        heightfield (hf_sample_position_adjoint / _tangent); uv, pdf and the choice of triangle are not."""
        self.ensure_pmf_built()
        sample = _as_f32(sample, self.device).reshape(2, -1)
        n = sample.shape[1]
        keep, ap = self._mask(active, n)
        block = torch.empty((6, n), dtype=torch.float32, device=self.device)   # p, n
        rest = torch.empty((5, n), dtype=torch.float32, device=self.device)    # uv, pdf, b
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        more = _row_addrs(rest)
        out = _fill(hf_position_sample_t(), _SAMPLE_ROWS, _row_addrs(block) + more[0:3] + [prim.data_ptr()] + more[3:5])
        check(_capi.lib().hf_sample_position(self._h, n, C.byref(_row_ptrs(sample)), ap, C.byref(out), self._stream()))
        if self._wants_derivative():
            block = _SamplePositionOp.apply(self, self.heightfield, prim, rest[3:5], keep, block, self._to_world_live())
        ps = PositionSample3f(block[0:3], block[3:6], rest[0:2], time, rest[2], False)
        ps.prim_index, ps.b = prim, rest[3:5]
        return ps

    def pdf_position(self, ps, active=True):
        """mesh.cpp:637-640: m_area_pmf.normalization() = (float) (1 / sum) for every active lane"""
        norm = self._area_scalars()[1]
        n = ps.p.shape[1]
        pdf = torch.full((n,), norm, dtype=torch.float32, device=self.device)
        keep, _ = self._mask(active, n)
        return pdf if keep is None else torch.where(keep.bool(), pdf, torch.zeros_like(pdf))

    def sample_direction(self, it, sample, active=True):
        """Shape::sample_direction (shape.cpp:363-382) on sample_position: differentiable in the heightfield and in it.p"""
        ps = self.sample_position(it.time, sample, active)
        d = ps.p - it.p
        dist_squared = (d * d).sum(0)
        dist = torch.sqrt(dist_squared)
        d = d / dist
        dp = (d * ps.n).sum(0).abs()
        x = dist_squared / dp
        pdf = ps.pdf * torch.where(torch.isfinite(x), x, torch.zeros_like(x))
        ps.pdf = pdf
        return DirectionSample3f(ps, d, dist)

    def pdf_direction(self, it, ds, active=True):
        """Shape::pdf_direction (shape.cpp:385-395)"""
        pdf = self.pdf_position(ds, active)
        dp = (ds.d * ds.n).sum(0).abs()
        return pdf * torch.where(dp != 0, (ds.dist * ds.dist) / dp, torch.zeros_like(dp))

    def _sample_adjoint_raw(self, prim, b, active_u8, g, grad_h, grad_tw=None):
        b = b.contiguous()
        check(_capi.lib().hf_sample_position_adjoint_transform(
            self._h, prim.shape[0], prim.data_ptr(), C.byref(_row_ptrs(b)), _ptr(active_u8), C.byref(_p3(g[0:3])),
            C.byref(_p3(g[3:6])), _ptr(grad_h), _ptr(_grad12(grad_tw)), self._stream()))

    def _sample_tangent_raw(self, prim, b, active_u8, dh, dtw=None):
        n = prim.shape[0]
        out = torch.zeros((6, n), dtype=torch.float32, device=self.device)
        if dh is None and dtw is None:
            return out
        dh, dtw, b = self._dheights(dh), _tw_tangent(dtw, self.device), b.contiguous()
        check(_capi.lib().hf_sample_position_tangent_transform(
            self._h, n, prim.data_ptr(), C.byref(_row_ptrs(b)), _ptr(active_u8), _ptr(dh), _ptr(dtw),
            C.byref(_p3(out[0:3])), C.byref(_p3(out[3:6])), self._stream()))
        return out

    def sample_position_adjoint(self, ps, grad_p=None, grad_n=None, active=True, grad_heightfield=None,
                                grad_to_world=None):
        """Explicit adjoint of sample_position for the samples of `ps`: accumulates dL/dheight for the upstream
        gradients grad_p / grad_n ([3, n], None = zero) into grad_heightfield ([H, W]).  grad_to_world (12 contiguous
        float32 device values, row-major 3x4, optional): dL/d(to_world) is accumulated into it as well
        (hf_sample_position_adjoint_transform)."""
        n = ps.prim_index.shape[0]
        if grad_heightfield is None:
            grad_heightfield = self._zero_heights()
        z = torch.zeros((3, n), dtype=torch.float32, device=self.device)
        g = torch.cat([z if grad_p is None else _as_f32(grad_p, self.device).reshape(3, n),
                       z if grad_n is None else _as_f32(grad_n, self.device).reshape(3, n)]).contiguous()
        keep, _ = self._mask(active, n)
        self._sample_adjoint_raw(ps.prim_index, ps.b, keep, g, grad_heightfield, grad_to_world)
        return grad_heightfield

    def sample_position_tangent(self, ps, dheights, active=True, d_to_world=None):
        """Explicit forward mode of sample_position: (dp, dn) ([3, n] each) for the height tangent dheights ([H, W])
        and the tangent d_to_world (3x4 / 4x4 / 12 values) of to_world; either may be None (zero)"""
        keep, _ = self._mask(active, ps.prim_index.shape[0])
        out = self._sample_tangent_raw(ps.prim_index, ps.b, keep, dheights, d_to_world)
        return out[0:3], out[3:6]

    # ---- eval_parameterization (Shape::eval_parameterization, shape.h:361; Mesh: mesh.cpp:503-545, 614-635) ----------
    def eval_parameterization(self, uv, ray_flags=RayFlags.All, active=True):
        """The surface interaction at texture coordinates uv ([2, n]; hf_eval_parameterization): the record of Mesh's
        UV-space ray o = (u, v, -1), d = (0, 0, 1) (t = 1, wi = sh_frame.to_local((0, 0, -1))).  Lanes outside
        [0, 1]^2, NaN and inactive lanes are misses (is_valid() False, wi = 0).  si.prim_index is the triangle.
        p, n, sh_frame (and wi), dp_du, dp_dv are differentiable in the heightfield -- and in to_world for
        differentiable_to_world shapes -- with the triangle and its barycentrics frozen; uv and t are not."""
        ray_flags = int(ray_flags)
        if (ray_flags & RayFlags.DetachShape) and (ray_flags & RayFlags.FollowShape):
            raise _capi.HfError(_capi.HF_EFLAGS, "Invalid combination of RayFlags: DetachShape | FollowShape")
        uv = _as_f32(uv.detach() if isinstance(uv, torch.Tensor) else uv, self.device).reshape(2, -1)
        n = uv.shape[1]
        diff, aux, out = self._si_blocks(n)
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        keep, ap = self._mask(active, n)
        check(_capi.lib().hf_eval_parameterization(self._h, n, C.byref(_row_ptrs(uv)), ray_flags, ap, C.byref(out),
                                                   prim.data_ptr(), self._stream()))
        detach = bool(ray_flags & RayFlags.DetachShape)
        if self._wants_derivative(detach=detach):
            diff = _ParameterizationOp.apply(self, self.heightfield, uv, ray_flags, keep, diff, self._to_world_live(detach))
        o = torch.stack([uv[0], uv[1], torch.full_like(uv[0], -1.0)])
        d = torch.zeros((3, n), dtype=torch.float32, device=self.device)
        d[2] = 1.0
        ray = Ray3f(o, d, torch.ones(n, dtype=torch.float32, device=self.device))
        return self._package_si(ray, prim, diff, aux, ray_flags)

    def _param_adjoint_raw(self, uv, ray_flags, active_u8, g, grad_h, grad_tw=None):
        gs = _fill(hf_si_grad_t(), _DIFF_ROWS, _row_addrs(g))
        check(_capi.lib().hf_eval_parameterization_adjoint(
            self._h, uv.shape[1], C.byref(_row_ptrs(uv)), int(ray_flags), _ptr(active_u8), C.byref(gs), _ptr(grad_h),
            _ptr(_grad12(grad_tw)), self._stream()))

    def _param_tangent_raw(self, uv, ray_flags, active_u8, dh, dtw=None):
        n = uv.shape[1]
        out = torch.zeros((18, n), dtype=torch.float32, device=self.device)
        if dh is None and dtw is None:
            return out
        dh, dtw = self._dheights(dh), _tw_tangent(dtw, self.device)
        ts = _fill(hf_si_tangent_t(), _DIFF_ROWS, _row_addrs(out))
        check(_capi.lib().hf_eval_parameterization_tangent(
            self._h, n, C.byref(_row_ptrs(uv)), int(ray_flags), _ptr(active_u8), _ptr(dh), _ptr(dtw), C.byref(ts),
            self._stream()))
        return out

    def eval_parameterization_adjoint(self, uv, grad_si, ray_flags=RayFlags.All, active=True, grad_heightfield=None,
                                      grad_to_world=None):
        """Explicit adjoint of eval_parameterization: accumulates dL/dheight for the upstream gradients grad_si ([18, n]:
        t, p, n, uv, sh_frame.n, dp_du, dp_dv; the t and uv rows are ignored) into grad_heightfield ([H, W]) and, when
        given (12 contiguous float32 device values), dL/d(to_world) into grad_to_world"""
        uv = _as_f32(uv.detach() if isinstance(uv, torch.Tensor) else uv, self.device).reshape(2, -1)
        n = uv.shape[1]
        g = _as_f32(grad_si, self.device)
        assert g.shape == (18, n)
        if grad_heightfield is None:
            grad_heightfield = self._zero_heights()
        keep, _ = self._mask(active, n)
        self._param_adjoint_raw(uv, ray_flags, keep, g, grad_heightfield, grad_to_world)
        return grad_heightfield

    def eval_parameterization_tangent(self, uv, dheights=None, ray_flags=RayFlags.All, active=True, d_to_world=None):
        """Explicit forward mode of eval_parameterization: the tangent [18, n] for dheights ([H, W]) and d_to_world
        (3x4 / 4x4 / 12 values), either None (zero); the t and uv rows are 0"""
        uv = _as_f32(uv.detach() if isinstance(uv, torch.Tensor) else uv, self.device).reshape(2, -1)
        keep, _ = self._mask(active, uv.shape[1])
        return self._param_tangent_raw(uv, ray_flags, keep, dheights, d_to_world)

    # ---- shape attributes (Mesh::add_attribute / has_attribute / eval_attribute*, mesh.cpp:905-1004) -------------------
    def _attr_count(self, type_):
        return self.width * self.height if type_ == _capi.HF_ATTR_VERTEX else 2 * (self.width - 1) * (self.height - 1)

    def add_attribute(self, name, size, data):
        """mesh.cpp:905-936: `vertex_*` holds one value of `size` floats per grid vertex (row-major, vertex (i, j) =
        i W + j), `face_*` one per triangle (prim_index order); data is read as count * size interleaved floats"""
        if name in self.attributes:
            raise RuntimeError(f"add_attribute(): attribute {name} already exists.")
        if name.startswith("vertex_"):
            type_ = _capi.HF_ATTR_VERTEX
        elif name.startswith("face_"):
            type_ = _capi.HF_ATTR_FACE
        else:
            raise RuntimeError('add_attribute(): attribute name must start with either "vertex_" of "face_".')
        size = int(size)
        count = self._attr_count(type_)
        buf = torch.as_tensor(data, dtype=torch.float32).detach().to(self.device).reshape(-1).contiguous().clone()
        if buf.numel() != count * size:
            raise RuntimeError(f"add_attribute(): attribute {name}: expected {count} x {size} values, got {buf.numel()}")
        self.attributes[name] = buf
        self._attr_meta[name] = (type_, size)

    def has_attribute(self, name, active=True):
        """mesh.cpp:938-944; Shape::has_attribute (shape.cpp:457-463) is false for any other name"""
        return name in self.attributes

    def _attr_lookup(self, fn, name, sizes):
        if name not in self.attributes:   # Shape::eval_attribute* (shape.cpp:465-505)
            raise RuntimeError(f"Invalid attribute requested {name}.")
        type_, size = self._attr_meta[name]
        if size not in sizes:
            raise RuntimeError(f'{fn}(): Attribute "{name}" requested but had size {size}.')
        return type_, size

    def eval_attribute(self, name, si, active=True):
        """mesh.cpp:946-967 in an RGB variant: [3, n]; a size-1 attribute is broadcast to the three channels"""
        _, size = self._attr_lookup("eval_attribute", name, (1, 3))
        v = self._eval_attr(name, si, active)
        return v.expand(3, -1) if size == 1 else v

    def eval_attribute_1(self, name, si, active=True):
        """mesh.cpp:969-985: [n]"""
        self._attr_lookup("eval_attribute_1", name, (1,))
        return self._eval_attr(name, si, active)[0]

    def eval_attribute_3(self, name, si, active=True):
        """mesh.cpp:987-1004: [3, n]"""
        self._attr_lookup("eval_attribute_3", name, (3,))
        return self._eval_attr(name, si, active)

    def _attr_inputs(self, name, attr, p, prim, t, active_u8):
        """(type, size, attr address, prim address, p rows (byref or None), t address, active address)"""
        type_, size = self._attr_meta[name]
        if attr.numel() != size * self._attr_count(type_) or not attr.is_contiguous() or attr.dtype != torch.float32:
            # the kernels gather count * size floats: a buffer assigned behind parameters_changed's back is refused
            raise RuntimeError(f"attribute {name}: expected a contiguous float32 buffer of {self._attr_count(type_)} x "
                               f"{size} values, got {tuple(attr.shape)} {attr.dtype}")
        vertex = type_ == _capi.HF_ATTR_VERTEX
        assert not vertex or (p.is_contiguous() and p.dtype == torch.float32)
        return type_, size, prim.data_ptr(), _ref(_p3(p) if vertex else None), _ptr(t), _ptr(active_u8)

    def _eval_attr(self, name, si, active):
        vertex = self._attr_meta[name][0] == _capi.HF_ATTR_VERTEX
        n = si.prim_index.shape[0]
        keep, _ = self._mask(active, n)
        prim = si.prim_index.contiguous()
        t = si.t.detach().contiguous() if si.t is not None else None
        p = si.p.detach().to(torch.float32).contiguous() if vertex else None
        buf = self.attributes[name]
        value = self._attr_forward_raw(name, buf.detach(), p, prim, t, keep)
        if vertex and self._to_world_live() is not None:
            raise NotImplementedError(
                f"eval_attribute({name!r}): the derivative of a vertex attribute with respect to to_world is not "
                "implemented; evaluate it under torch.no_grad() or with a to_world that does not require a gradient")
        # a face attribute depends on its buffer alone; a vertex attribute on si.p and the heights as well
        if self._wants_derivative(buf, si.p) if vertex else self._wants_derivative(buf, detach=True):
            value = _AttributeOp.apply(self, name, buf, si.p if vertex else None, self.heightfield if vertex else None,
                                       prim, t, keep, value)
        return value

    def _attr_forward_raw(self, name, attr, p, prim, t, active_u8):
        n = prim.shape[0]
        type_, size, pr, pp, tp, ap = self._attr_inputs(name, attr, p, prim, t, active_u8)
        out = torch.empty((size, n), dtype=torch.float32, device=self.device)
        check(_capi.lib().hf_eval_attribute(self._h, n, type_, size, attr.data_ptr(), pr, pp, tp, ap,
                                            C.byref(_row_ptrs(out, 3)), self._stream()))
        return out

    def _attr_adjoint_raw(self, name, attr, p, prim, t, active_u8, g, need_attr=True, need_p=True, need_h=True,
                          grad_attr=None, grad_h=None):
        """(dL/dattr [count * size], dL/dp [3, n], dL/dheight [H, W]) for g [size, n]; None where not needed"""
        n = prim.shape[0]
        type_, size, pr, pp, tp, ap = self._attr_inputs(name, attr, p, prim, t, active_u8)
        vertex = type_ == _capi.HF_ATTR_VERTEX
        need_p, need_h = need_p and vertex, need_h and vertex
        if need_attr and grad_attr is None:
            grad_attr = torch.zeros(attr.numel(), dtype=torch.float32, device=self.device)
        if need_h and grad_h is None:
            grad_h = self._zero_heights()
        gp = torch.empty((3, n), dtype=torch.float32, device=self.device) if need_p else None
        check(_capi.lib().hf_eval_attribute_adjoint(self._h, n, type_, size, attr.data_ptr(), pr, pp, tp, ap,
                                                    C.byref(_row_ptrs(g, 3)), _ptr(grad_attr if need_attr else None),
                                                    _ref(_row_ptrs(gp)), _ptr(grad_h if need_h else None),
                                                    self._stream()))
        return (grad_attr if need_attr else None), gp, (grad_h if need_h else None)

    def _attr_tangent_raw(self, name, attr, p, prim, t, active_u8, dattr=None, dp=None, dh=None):
        n = prim.shape[0]
        type_, size, pr, pp, tp, ap = self._attr_inputs(name, attr, p, prim, t, active_u8)
        out = torch.empty((size, n), dtype=torch.float32, device=self.device)
        dattr, dh = _tangent(dattr, (attr.numel(),), self.device, "dattr"), self._dheights(dh)
        dp = _tangent(dp, (3, n), self.device, "dp") if type_ == _capi.HF_ATTR_VERTEX else None
        check(_capi.lib().hf_eval_attribute_tangent(self._h, n, type_, size, attr.data_ptr(), pr, pp, tp, ap, _ptr(dattr),
                                                    _ref(_row_ptrs(dp)), _ptr(dh), C.byref(_row_ptrs(out, 3)),
                                                    self._stream()))
        return out

    def _attr_si(self, si):
        prim = si.prim_index.contiguous()
        t = si.t.detach().contiguous() if si.t is not None else None
        p = si.p.detach().to(torch.float32).contiguous() if si.p is not None else None
        return p, prim, t

    def eval_attribute_adjoint(self, name, si, grad, active=True, grad_attr=None, grad_heightfield=None):
        """Explicit reverse mode of eval_attribute* (no autograd): for dL/dvalue grad ([size, n]) returns
        (dL/dattr [count * size], accumulated into grad_attr if given; dL/dp [3, n]; dL/dheight [H, W], accumulated into
        grad_heightfield if given).  Face attributes: dL/dp and dL/dheight are None."""
        p, prim, t = self._attr_si(si)
        keep, _ = self._mask(active, prim.shape[0])
        g = _as_f32(grad, self.device).reshape(self._attr_meta[name][1], -1).contiguous()
        return self._attr_adjoint_raw(name, self.attributes[name].detach(), p, prim, t, keep, g,
                                      grad_attr=grad_attr, grad_h=grad_heightfield)

    def eval_attribute_tangent(self, name, si, dattr=None, dp=None, dheights=None, active=True):
        """Explicit forward mode of eval_attribute*: the tangent [size, n] for the tangents dattr ([count * size]), dp
        ([3, n], of si.p) and dheights ([H, W]); any of them may be None (zero)"""
        p, prim, t = self._attr_si(si)
        keep, _ = self._mask(active, prim.shape[0])
        return self._attr_tangent_raw(name, self.attributes[name].detach(), p, prim, t, keep, dattr, dp, dheights)

    def parameters_grad_enabled(self):
        tw = self.to_world
        tw_grad = self.differentiable_to_world and isinstance(tw, torch.Tensor) and tw.requires_grad
        return bool(self.heightfield.requires_grad or tw_grad)

    def mark_dirty(self):
        self._dirty = True

    def dirty(self):
        return self._dirty

    def primitive_count(self):
        """one kd-tree primitive (shape.cpp:526-529); the cells are internal"""
        return 1

    def effective_primitive_count(self):
        return 2 * (self.width - 1) * (self.height - 1)

    def is_mesh(self):
        return False

    def bbox(self):
        out = (C.c_float * 6)()
        check(_capi.lib().hf_bbox(self._h, out))
        return torch.tensor(list(out), dtype=torch.float32).reshape(2, 3)

    def num_levels(self):
        return _capi.lib().hf_num_levels(self._h)

    def mip(self, level):
        w, h = C.c_uint32(), C.c_uint32()
        check(_capi.lib().hf_get_mip(self._h, level, None, C.byref(w), C.byref(h)))
        out = torch.empty((h.value, w.value, 2), dtype=torch.float32)
        check(_capi.lib().hf_get_mip(self._h, level, out.data_ptr(), C.byref(w), C.byref(h)))
        return out

    def node_level(self, level):
        """the acceleration data of level `level` as stored, padded slots included: (records [side, side, 12] =
        (a, b, c, f, lo0, hi0, .., lo3, hi3) per node, minmax [side, side, 2]), side = 2^(num_levels - level)"""
        side = C.c_uint32()
        check(_capi.lib().hf_get_node_level(self._h, level, None, None, C.byref(side)))
        rec = torch.empty((side.value, side.value, 12), dtype=torch.float32)
        mm = torch.empty((side.value, side.value, 2), dtype=torch.float32)
        check(_capi.lib().hf_get_node_level(self._h, level, rec.data_ptr(), mm.data_ptr(), C.byref(side)))
        return rec, mm

    # ---- helpers -------------------------------------------------------------------------
    def _stream(self):
        return _stream_of(self.device)

    def _check_ray(self, ray):
        if not isinstance(ray, Ray3f):
            raise TypeError("expected a Ray3f")
        if ray.device != self.device:
            raise RuntimeError(f"ray lives on {ray.device}, shape on {self.device}")

    @staticmethod
    def _rays_struct(o, d, maxt):
        return _fill(hf_rays_t(), _RAY_ROWS, _row_addrs(o)[:3] + _row_addrs(d)[:3] + [maxt.data_ptr()])

    def _mask(self, active, n):
        if active is True or active is None:
            return None, None
        if active is False:
            active = torch.zeros(n, dtype=torch.bool, device=self.device)
        a = torch.as_tensor(active, device=self.device).to(torch.uint8).contiguous()
        if a.numel() == 1 and n != 1:
            a = a.expand(n).contiguous()
        assert a.shape == (n,)
        return a, a.data_ptr()

    @staticmethod
    def _pi_struct(t, uv, prim):
        return _fill(hf_pi_t(), _PI_ROWS, [t.data_ptr()] + _row_addrs(uv)[:2] + [prim.data_ptr()])

    # ---- the hot path ---------------------------------------------------------------------
    # ---- the `coherent` hint of Scene::ray_intersect / ray_test / ray_intersect_preliminary (scene.h:117-146) ----------
    COHERENCE_AUTO, COHERENCE_INCOHERENT, COHERENCE_COHERENT = 0, 1, 2

    def set_ray_coherence(self, mode):
        """``hf_set_ray_coherence``: which kernels the trace launches that follow take -- ``COHERENCE_AUTO`` (default:
        every 64-ray batch decides for itself), ``COHERENCE_INCOHERENT`` (= ``coherent=False``: bounce rays, auxiliary
        rays; kernels without the beam sweep at 6-7 waves per SIMD) or ``COHERENCE_COHERENT``.  Results never depend on it."""
        check(_capi.lib().hf_set_ray_coherence(self._h, int(mode)))

    def ray_coherence(self):
        return int(_capi.lib().hf_get_ray_coherence(self._h))

    class _Coherence:
        """``with shape._coherent(flag):`` -- the hint for the launches inside (None: the handle's mode as it is)"""
        def __init__(self, shape, flag):
            self.shape, self.flag = shape, flag
        def __enter__(self):
            if self.flag is not None:
                self.old = self.shape.ray_coherence()
                self.shape.set_ray_coherence(Heightfield.COHERENCE_COHERENT if self.flag else Heightfield.COHERENCE_INCOHERENT)
        def __exit__(self, *exc):
            if self.flag is not None:
                self.shape.set_ray_coherence(self.old)
            return False

    def _coherent(self, flag):
        return Heightfield._Coherence(self, flag)

    def ray_intersect_preliminary(self, ray, active=True, coherent=None):
        """shape.h:137-138; ``coherent``: the hint of Scene::ray_intersect_preliminary (scene.h:237-259), None = the handle's mode"""
        self._check_ray(ray)
        n = len(ray)
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        uv = torch.empty((2, n), dtype=torch.float32, device=self.device)
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        keep, ap = self._mask(active, n)
        rays = self._rays_struct(ray.o, ray.d, ray.maxt)
        pi = self._pi_struct(t, uv, prim)
        with self._coherent(coherent):
            check(_capi.lib().hf_ray_intersect_preliminary(self._h, n, C.byref(rays), ap, C.byref(pi), self._stream()))
        return PreliminaryIntersection3f(t, uv, prim, self)

    def ray_test(self, ray, active=True, coherent=None):
        """shape.h:153; ``coherent``: scene.h:188-207"""
        self._check_ray(ray)
        n = len(ray)
        hit = torch.empty(n, dtype=torch.uint8, device=self.device)
        keep, ap = self._mask(active, n)
        rays = self._rays_struct(ray.o, ray.d, ray.maxt)
        with self._coherent(coherent):
            check(_capi.lib().hf_ray_test(self._h, n, C.byref(rays), ap, hit.data_ptr(), self._stream()))
        return hit.bool()

    # ---- scalar / packet forms (shape.h:220-240): host arrays in, host arrays out -------------------
    def ray_intersect_preliminary_packet(self, o, d, maxt=None, active=None):
        """``ray_intersect_preliminary_packet`` / ``_scalar`` (shape.h:220-240, the per-kd-leaf call of
        kdtree.h:2490-2520): up to 16 rays held in HOST memory (numpy / CPU tensors, [3, n] or [3]).  Returns
        host arrays ``(t, prim_uv [2, n], prim_index)``.  Same kernel and arithmetic as the wavefront entry,
        one synchronous launch per call (``hf_ray_intersect_preliminary_packet``)."""
        import numpy as np
        o, d, maxt, act, n = self._host_packet(o, d, maxt, active)
        t = np.empty(n, np.float32); uv = np.empty((2, n), np.float32); prim = np.empty(n, np.uint32)
        check(_capi.lib().hf_ray_intersect_preliminary_packet(self._h, n, C.byref(_row_ptrs(o)), C.byref(_row_ptrs(d)),
                                                              _ptr(maxt), _ptr(act), _ptr(t), C.byref(_row_ptrs(uv)),
                                                              _ptr(prim)))
        return t, uv, prim

    def ray_intersect_preliminary_scalar(self, o, d, maxt=math.inf):
        t, uv, prim = self.ray_intersect_preliminary_packet(o, d, maxt)
        return float(t[0]), (float(uv[0, 0]), float(uv[1, 0])), int(prim[0])

    def ray_test_packet(self, o, d, maxt=None, active=None):
        import numpy as np
        o, d, maxt, act, n = self._host_packet(o, d, maxt, active)
        hit = np.empty(n, np.uint8)
        check(_capi.lib().hf_ray_test_packet(self._h, n, C.byref(_row_ptrs(o)), C.byref(_row_ptrs(d)), _ptr(maxt),
                                             _ptr(act), _ptr(hit)))
        return hit.astype(bool)

    def ray_test_scalar(self, o, d, maxt=math.inf):
        return bool(self.ray_test_packet(o, d, maxt)[0])

    @staticmethod
    def _host_packet(o, d, maxt, active):
        import numpy as np
        o = np.ascontiguousarray(np.asarray(o, np.float32).reshape(3, -1))
        d = np.ascontiguousarray(np.asarray(d, np.float32).reshape(3, -1))
        n = max(o.shape[1], d.shape[1])
        o = np.ascontiguousarray(np.broadcast_to(o, (3, n))); d = np.ascontiguousarray(np.broadcast_to(d, (3, n)))
        maxt = np.full(n, math.inf, np.float32) if maxt is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(maxt, np.float32).reshape(-1), (n,)))
        act = None if active is None else np.ascontiguousarray(np.broadcast_to(np.asarray(active).astype(np.uint8).reshape(-1), (n,)))
        return o, d, maxt, act, n

    def _si_blocks(self, n):
        """the two blocks of an SI record, [18, n] (_DIFF_ROWS: what autograd sees) and [10, n] (_AUX_ROWS), and the
        hf_si_t over their rows"""
        diff = torch.empty((18, n), dtype=torch.float32, device=self.device)
        aux = torch.empty((10, n), dtype=torch.float32, device=self.device)
        return diff, aux, _fill(hf_si_t(), _DIFF_ROWS + _AUX_ROWS, _row_addrs(diff) + _row_addrs(aux))

    def _attach_si(self, ray, t, uv, prim, ray_flags, keep, diff):
        """the differentiable block as the output of _SurfaceInteractionOp when a derivative is wanted.  DetachShape:
        the heights and to_world are detached, the rays are not."""
        detach = bool(ray_flags & RayFlags.DetachShape)
        if self._wants_derivative(ray.o, ray.d, detach=detach):
            diff = _SurfaceInteractionOp.apply(self, self.heightfield, ray.o, ray.d, ray.maxt, t, uv, prim, ray_flags, keep,
                                               diff, self._to_world_live(detach))
        return diff

    def _package_si(self, ray, pi_prim, diff, aux, ray_flags):
        n = len(ray)
        si = SurfaceInteraction3f()
        si.t = diff[0]
        si.p, si.n, si.uv = diff[1:4], diff[4:7], diff[7:9]
        sh_n = diff[9:12]
        si.dp_du, si.dp_dv = diff[12:15], diff[15:18]
        si.boundary_test = aux[0] if (ray_flags & RayFlags.BoundaryTest) else torch.zeros(n, device=self.device)
        sh_s, sh_t, wi = aux[1:4], aux[4:7], aux[7:10]
        if (diff.requires_grad or _has_tangent(diff)) and (ray_flags & RayFlags.ShadingFrame):
            # finalize_surface_interaction is AD-attached in the reference (interaction.h:257-267, 476-499):
            # sh_frame.s = normalize(dp_du - n <n, dp_du>), t = cross(n, s), wi = to_local(-d).  The kernel's rows are
            # plain outputs, so when gradients are wanted these three are rebuilt here from the differentiable rows
            # (sh_frame.n, dp_du, ray.d): a BSDF that reads cos_theta = wi.z then back-propagates to the heights.
            dp_du = si.dp_du
            s_un = dp_du - sh_n * (sh_n * dp_du).sum(0, keepdim=True)
            nrm = torch.linalg.norm(s_un, dim=0, keepdim=True)
            ok = (nrm > 0) & torch.isfinite(diff[0])[None, :]
            s_at = s_un / torch.where(ok, nrm, torch.ones_like(nrm))
            sh_s = torch.where(ok, s_at, aux[1:4])           # degenerate dp_du / misses: the kernel's (detached) rows
            sh_t = torch.where(ok, torch.linalg.cross(sh_n, sh_s, dim=0), aux[4:7])
            md = -ray.d
            wi = torch.where(ok, torch.stack([(md * sh_s).sum(0), (md * sh_t).sum(0), (md * sh_n).sum(0)]), aux[7:10])
        si.sh_frame = Frame3f(sh_s, sh_t, sh_n)
        si.wi = wi
        zeros3 = torch.zeros((3, n), dtype=torch.float32, device=self.device)
        si.dn_du, si.dn_dv = zeros3, zeros3          # flat shading
        si.duv_dx = si.duv_dy = torch.zeros((2, n), dtype=torch.float32, device=self.device)
        si.prim_index = pi_prim                       # interaction.h:486
        si.shape = self
        si.time, si.wavelengths = ray.time, ray.wavelengths
        si.ray_flags = int(ray_flags)
        return si

    def compute_surface_interaction(self, ray, pi, ray_flags=RayFlags.All, recursion_depth=0, active=True):
        """shape.h:179-183 + finalize_surface_interaction (interaction.h:476-499)"""
        self._check_ray(ray)
        ray_flags = int(ray_flags)
        n = len(ray)
        diff, aux, out = self._si_blocks(n)
        if recursion_depth > 0:   # mesh.cpp:680-682: early exit, zero-initialised record
            diff.zero_(); aux.zero_()
            return self._package_si(ray, pi.prim_index, diff, aux, ray_flags)
        keep, ap = self._mask(active, n)
        rays = self._rays_struct(ray.o, ray.d, ray.maxt)
        pis = self._pi_struct(pi.t, pi.prim_uv, pi.prim_index)
        check(_capi.lib().hf_compute_surface_interaction(self._h, n, C.byref(rays), C.byref(pis), ray_flags, ap,
                                                         C.byref(out), self._stream()))
        diff = self._attach_si(ray, pi.t, pi.prim_uv, pi.prim_index, ray_flags, keep, diff)
        return self._package_si(ray, pi.prim_index, diff, aux, ray_flags)

    def ray_intersect(self, ray, ray_flags=RayFlags.All, active=True, coherent=None):
        """shape.cpp:436-446: preliminary intersection + surface interaction, one fused kernel; ``coherent``: scene.h:117-146"""
        self._check_ray(ray)
        ray_flags = int(ray_flags)
        n = len(ray)
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        uv = torch.empty((2, n), dtype=torch.float32, device=self.device)
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        diff, aux, out = self._si_blocks(n)
        keep, ap = self._mask(active, n)
        rays = self._rays_struct(ray.o, ray.d, ray.maxt)
        pis = self._pi_struct(t, uv, prim)
        with self._coherent(coherent):
            check(_capi.lib().hf_ray_intersect(self._h, n, C.byref(rays), ray_flags, ap, C.byref(pis), C.byref(out),
                                               self._stream()))
        diff = self._attach_si(ray, t, uv, prim, ray_flags, keep, diff)
        si = self._package_si(ray, prim, diff, aux, ray_flags)
        si.prim_uv = uv
        return si

    # ---- adjoint ------------------------------------------------------------------------------
    def _adjoint_raw(self, o, d, maxt, t, uv, prim, ray_flags, active_u8, g, grad_h, grad_od, row_band=None, grad_tw=None):
        rays = self._rays_struct(o, d, maxt)
        pis = self._pi_struct(t, uv, prim)
        gs = _fill(hf_si_grad_t(), _DIFF_ROWS, _row_addrs(g))
        go, gd = (None, None) if grad_od is None else (_p3(grad_od[0:3]), _p3(grad_od[3:6]))
        # (without grad_tw this is hf_adjoint_rows: the entry forwards to it)
        check(_capi.lib().hf_adjoint_transform(self._h, o.shape[1], C.byref(rays), C.byref(pis), int(ray_flags),
                                               _ptr(active_u8), C.byref(gs), _ptr(grad_h), _ref(go), _ref(gd),
                                               _ptr(row_band), _ptr(_grad12(grad_tw)), self._stream()))

    # ---- tangent (forward mode) ------------------------------------------------------------------
    def _tangent_raw(self, o, d, maxt, t, uv, prim, ray_flags, active_u8, dh, do, dd, dtw=None):
        n = o.shape[1]
        out = torch.empty((18, n), dtype=torch.float32, device=self.device)
        ts = _fill(hf_si_tangent_t(), _DIFF_ROWS, _row_addrs(out))
        dh, dtw = self._dheights(dh), _tw_tangent(dtw, self.device)
        do, dd = _tangent(do, (3, n), self.device, "d_o"), _tangent(dd, (3, n), self.device, "d_d")
        rays = self._rays_struct(o, d, maxt)
        pis = self._pi_struct(t, uv, prim)
        check(_capi.lib().hf_tangent_transform(self._h, n, C.byref(rays), C.byref(pis), int(ray_flags), _ptr(active_u8),
                                               _ptr(dh), _ref(_row_ptrs(do)), _ref(_row_ptrs(dd)), _ptr(dtw), C.byref(ts),
                                               self._stream()))
        return out

    def tangent(self, ray, pi, dheights=None, d_o=None, d_d=None, ray_flags=RayFlags.All, active=True, d_to_world=None):
        """Explicit forward mode (``hf_tangent``), the mirror of ``adjoint``: the tangent [18, n] (t, p, n, uv,
        sh_frame.n, dp_du, dp_dv) of the surface interaction for a perturbation ``dheights`` ([H, W]) of the heights,
        ``d_o`` / ``d_d`` ([3, n]) of the rays and ``d_to_world`` (3x4 / 4x4 / 12 values, ``hf_tangent_transform``) of
        to_world; any of them may be None (zero).  Missed and inactive lanes: 0."""
        self._check_ray(ray)
        keep, _ = self._mask(active, len(ray))
        return self._tangent_raw(ray.o.detach(), ray.d.detach(), ray.maxt, pi.t, pi.prim_uv, pi.prim_index, ray_flags, keep,
                                 dheights, d_o, d_d, d_to_world)

    def new_row_band(self):
        """{height, 0} as int32[2] on the device: the initial value of hf_adjoint_rows' row band."""
        return torch.tensor([self.height, 0], dtype=torch.int32, device=self.device)

    def adjoint(self, ray, pi, grad_si, ray_flags=RayFlags.All, active=True, grad_heightfield=None,
                ray_grads=False, row_band=None, grad_to_world=None):
        """Explicit adjoint: accumulate dL/dheight for upstream gradients `grad_si`
        ([18, n]: t, p, n, uv, sh_frame.n, dp_du, dp_dv) into `grad_heightfield` ([H, W]).
        row_band (int32[2] device tensor from new_row_band(), optional): updated to {lowest texture row that
        received a contribution, highest + 1} (hf_adjoint_rows): what a multi-GPU host needs to all-reduce.
        grad_to_world (12 contiguous float32 device values, row-major 3x4, optional): dL/d(to_world) is accumulated
        into it as well (hf_adjoint_transform)."""
        self._check_ray(ray)
        n = len(ray)
        g = _as_f32(grad_si, self.device)
        assert g.shape == (18, n)
        if grad_heightfield is None:
            grad_heightfield = self._zero_heights()
        keep, _ = self._mask(active, n)
        grad_od = torch.empty((6, n), dtype=torch.float32, device=self.device) if ray_grads else None
        self._adjoint_raw(ray.o, ray.d, ray.maxt, pi.t, pi.prim_uv, pi.prim_index, ray_flags, keep, g,
                          grad_heightfield, grad_od, row_band, grad_to_world)
        if ray_grads:
            return grad_heightfield, grad_od[0:3], grad_od[3:6]
        return grad_heightfield


def allreduce_gradient(grad, group=None):
    """Sum the per-GPU dL/dheight textures (one RCCL all-reduce over xGMI; rays are
    sharded over ranks, heights are replicated -- SURVEY.md section 8e)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group)
    return grad


class Adam:
    """Adam on the heightfield parameter of one shape, the mirror of ``mitsuba.ad.Adam``
    (src/python/python/ad/optimizers.py:204-310) + ``params.update()`` (util.py:185-232):
    ``step()`` runs ``hf_adam_step`` -- the update of the parameter tensor in place and the rebuild
    of the shape's acceleration data -- in one call on the current stream.  State (m, v, t) lives here,
    like ``Optimizer.state`` / ``Adam.t``.  ``uniform``: the 'UniformAdam' variant (optimizers.py:259, 290-291)."""

    def __init__(self, shape, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-8, mask_updates=False, uniform=False):
        assert 0 <= beta_1 < 1 and 0 <= beta_2 < 1 and lr > 0 and epsilon > 0  # optimizers.py:248-249
        self.shape, self.lr, self.beta_1, self.beta_2, self.epsilon = shape, lr, beta_1, beta_2, epsilon
        self.mask_updates, self.uniform = mask_updates, uniform
        self.reset()

    def reset(self):
        """zero-initialise the optimiser state (optimizers.py:303-309)"""
        h = self.shape.heightfield
        self.state = (torch.zeros_like(h, requires_grad=False), torch.zeros_like(h, requires_grad=False))
        self.t = 0

    def set_learning_rate(self, lr):
        self.lr = lr

    def zero_grad(self):
        self.shape.heightfield.grad = None

    def step(self):
        h = self.shape.heightfield
        g = h.grad
        if g is None:  # optimizers.py:274-275: nothing to do without a gradient
            return
        if not (h.is_cuda and h.dtype == torch.float32 and h.is_contiguous()):
            raise RuntimeError("Adam: the heightfield parameter must be a contiguous float32 device tensor")
        g = g.to(dtype=torch.float32).contiguous()
        self.t += 1
        m, v = self.state
        check(_capi.lib().hf_adam_step(self.shape._h, h.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                       self.lr, self.beta_1, self.beta_2, self.epsilon, self.t,
                                       (1 if self.mask_updates else 0) | (2 if self.uniform else 0),
                                       self.shape._stream()))
        self.shape._heights_keepalive = h
        self.shape._heights_version += 1
        self.shape.mark_dirty()


# ---- what the lighting Functions (direct, sky, envmap, bounce) marshal alike -------------------------------------------
def _detached_f32(x):
    """a wavefront row (sh_n, p, n, d, t, weight of a lighting row) as a detached contiguous float32 tensor; None stays None"""
    return x.detach().to(dtype=torch.float32).contiguous() if x is not None else None


def _dir_lights(lights):
    """the [K, 4] lights as (hf_dir_light_t array of at least one entry, K); hf_point_light_t has its packing: position, intensity"""
    L = (_capi.hf_dir_light_t * max(lights.shape[0], 1))()
    for k, row in enumerate(lights.detach().cpu().tolist()):
        L[k].to_light[0], L[k].to_light[1], L[k].to_light[2], L[k].irradiance = row
    return L, lights.shape[0]


def _with_weight(ctx, saved, ww):
    """forward: the tensors to save, the optional per-sample weight last; ctx.weighted tells jvp and backward that it is there"""
    ctx.weighted = ww is not None
    return saved + (ww,) if ctx.weighted else saved


def _weighted_tangents(ctx, dsh_n, dweight):
    """jvp: the tangents of sh_n and weight as float32 (None: zero, or no weight was given)"""
    return _detached_f32(dsh_n), _detached_f32(dweight if ctx.weighted else None)


def _weighted_grads(ctx, sn, grad_image):
    """backward: grad_image as float32, the gradient outputs of sh_n and of weight (None: no weight was given)"""
    return _detached_f32(grad_image), torch.empty_like(sn), torch.empty_like(sn[0]) if ctx.weighted else None


def _texel_tangent(dfull):
    """jvp: the tangent of a map's texels as contiguous float32 (None: zero)"""
    return dfull.to(dtype=torch.float32).contiguous() if dfull is not None else None


def _texel_grad(ctx, i, dat):
    """backward: the zeroed grad_data an adjoint accumulates into, or None if input ``i`` (the texels) wants no gradient"""
    return torch.zeros_like(dat) if ctx.needs_input_grad[i] else None


def _empty_rays(pp):
    """the outputs of a *_rays entry: a Ray3f of the wavefront's size"""
    return Ray3f(torch.empty_like(pp), torch.empty_like(pp), torch.empty(pp.shape[1], dtype=torch.float32, device=pp.device))


def _lighting_inputs(sh_n, d, t, lights, vis):
    """what both direct lighting Functions pass to libhf: the sh_n, d and t rows as float32, the lights and the vis row pointers"""
    vis = vis.to(dtype=torch.uint8).contiguous() if vis is not None else None
    return (*(x.to(dtype=torch.float32).contiguous() for x in (sh_n, d, t)), *_dir_lights(lights), vis, _row_ptrs(vis))


class _DirectLightingOp(torch.autograd.Function):
    @staticmethod
    def _prefix(ctx, sn, dd, tt, ww=None):
        """what every hf_direct_lighting_weighted* entry starts with"""
        K, spp, L, albedo, vis, vis_p = ctx.misc
        return sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), K, L, albedo, vis_p

    @staticmethod
    def forward(ctx, sh_n, d, t, lights, albedo, spp, vis, weight):
        sn, dd, tt, L, K, vis, vis_p = _lighting_inputs(sh_n, d, t, lights, vis)
        saved = _with_weight(ctx, (sn, dd, tt), _detached_f32(weight))
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.misc = (K, spp, L, albedo, vis, vis_p)
        image = torch.empty((K, sn.shape[1] // spp), dtype=torch.float32, device=sh_n.device)
        check(_capi.lib().hf_direct_lighting_weighted(*_DirectLightingOp._prefix(ctx, *saved), image.data_ptr(),
                                                      _stream_of(sh_n.device)))
        return image

    @staticmethod
    def jvp(ctx, dsh_n, _dd, _dt, _dl, _da, _ds, _dv, dweight):
        saved = ctx.saved_tensors
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        K, spp, sn = ctx.misc[0], ctx.misc[1], saved[0]
        dimage = torch.empty((K, sn.shape[1] // spp), dtype=torch.float32, device=sn.device)
        check(_capi.lib().hf_direct_lighting_weighted_tangent(*_DirectLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                              _ptr(dw), dimage.data_ptr(), _stream_of(sn.device)))
        return dimage

    @staticmethod
    def backward(ctx, grad_image):
        saved = ctx.saved_tensors
        sn = saved[0]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        check(_capi.lib().hf_direct_lighting_weighted_adjoint(*_DirectLightingOp._prefix(ctx, *saved), gi.data_ptr(),
                                                              C.byref(_p3(gn)), _ptr(gw), _stream_of(sn.device)))
        return gn, None, None, None, None, None, None, gw


def direct_lighting(si, ray, lights, albedo=1.0, spp=1, vis=None, weight=None):
    """Diffuse direct lighting under directional lights + box-filter film, on the wavefront
    (``hf_direct_lighting``; the emitter-sampling term of direct_reparam.py:149-175 with diffuse.cpp:135-140).
    ``lights``: [K, 4] tensor of (unit direction towards the light, irradiance); ``vis``: optional [K, n] uint8,
    0 = shadowed (``~shape.ray_test(shadow ray)``); ``weight``: optional [n] per-sample factor -- the determinant of a
    reparameterised camera ray (direct_reparam.py:164-180), differentiable.  Returns the [K, n // spp] images;
    differentiable with respect to ``si.sh_frame.n`` (``hf_direct_lighting_adjoint``), which carries the gradient on
    to ``hf_adjoint`` and the heights, and to ``weight``."""
    lights = torch.as_tensor(lights, dtype=torch.float32)
    return _DirectLightingOp.apply(si.sh_frame.n, ray.d, si.t, lights, float(albedo), int(spp), vis, weight)


class _PointLightingOp(torch.autograd.Function):
    @staticmethod
    def _prefix(ctx, sn, pp, dd, tt):
        """what every hf_point_lighting* entry starts with"""
        K, spp, L, albedo, vis, vis_p = ctx.misc
        return (sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), C.byref(_p3(pp)), K, L, albedo,
                vis_p)

    @staticmethod
    def forward(ctx, sh_n, p, d, t, lights, albedo, spp, vis):
        sn, dd, tt, L, K, vis, vis_p = _lighting_inputs(sh_n, d, t, lights, vis)
        saved = (sn, p.to(dtype=torch.float32).contiguous(), dd, tt)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.misc = (K, spp, L, albedo, vis, vis_p)
        image = torch.empty((K, sn.shape[1] // spp), dtype=torch.float32, device=sh_n.device)
        check(_capi.lib().hf_point_lighting(*_PointLightingOp._prefix(ctx, *saved), image.data_ptr(),
                                            _stream_of(sh_n.device)))
        return image

    @staticmethod
    def jvp(ctx, dsh_n, dp, *_):
        sn = ctx.saved_tensors[0]
        dn, dq = _detached_f32(dsh_n), _detached_f32(dp)
        dimage = torch.empty((ctx.misc[0], sn.shape[1] // ctx.misc[1]), dtype=torch.float32, device=sn.device)
        check(_capi.lib().hf_point_lighting_tangent(*_PointLightingOp._prefix(ctx, *ctx.saved_tensors), _ref(_row_ptrs(dn)),
                                                    _ref(_row_ptrs(dq)), dimage.data_ptr(), _stream_of(sn.device)))
        return dimage

    @staticmethod
    def backward(ctx, grad_image):
        sn, pp = ctx.saved_tensors[:2]
        gi = grad_image.to(dtype=torch.float32).contiguous()
        gn = torch.empty_like(sn); gp = torch.empty_like(pp)
        check(_capi.lib().hf_point_lighting_adjoint(*_PointLightingOp._prefix(ctx, *ctx.saved_tensors), gi.data_ptr(),
                                                    C.byref(_p3(gn)), C.byref(_p3(gp)), _stream_of(sn.device)))
        return gn, gp, None, None, None, None, None, None


def point_lighting(si, ray, lights, albedo=1.0, spp=1, vis=None):
    """``direct_lighting`` under POINT lights (``hf_point_lighting``; src/emitters/point.cpp): ``lights`` is a [K, 4]
    tensor of (position, radiant intensity).  Differentiable with respect to ``si.sh_frame.n`` and ``si.p``."""
    lights = torch.as_tensor(lights, dtype=torch.float32)
    return _PointLightingOp.apply(si.sh_frame.n, si.p, ray.d, si.t, lights, float(albedo), int(spp), vis)


class _SkyLightingOp(torch.autograd.Function):
    """(image, visibility words) of hf_sky_lighting; backward = hf_sky_lighting_adjoint (gradients of sh_n and weight),
    jvp = hf_sky_lighting_tangent.  Both read the visibility word the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, dd, tt, vis, ww=None):
        """what hf_sky_lighting_adjoint / _tangent start with"""
        spp, num_rays, seed, rid, radiance, albedo = ctx.misc
        return (sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(rid),
                radiance, albedo, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, weight, shape, p, nrm, d, t, radiance, albedo, spp, num_rays, seed, ray_index):
        sn, pp, gn, dd, tt, ww = map(_detached_f32, (sh_n, p, nrm, d, t, weight))
        n = sn.shape[1]
        ctx.misc = (spp, num_rays, seed, ray_index, radiance, albedo)
        image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=sn.device)
        vis = torch.empty(n, dtype=torch.int32, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_sky_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                              C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(ray_index),
                                              radiance, albedo, image.data_ptr(), vis.data_ptr(), _stream_of(sn.device)))
        saved = _with_weight(ctx, (sn, dd, tt, vis), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, vis

    @staticmethod
    def jvp(ctx, dsh_n, dweight, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dimage = torch.empty(sn.shape[1] // ctx.misc[0], dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_sky_lighting_tangent(*_SkyLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)), _ptr(dw),
                                                      dimage.data_ptr(), _stream_of(sn.device)))
        return dimage, None

    @staticmethod
    def backward(ctx, grad_image, _grad_vis):
        saved = ctx.saved_tensors
        sn = saved[0]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        if sn.shape[1]:
            check(_capi.lib().hf_sky_lighting_adjoint(*_SkyLightingOp._prefix(ctx, *saved), gi.data_ptr(), C.byref(_p3(gn)),
                                                      _ptr(gw), _stream_of(sn.device)))
        return (gn, gw) + (None,) * 11


def sky_lighting(shape, si, ray, radiance=1.0, albedo=1.0, spp=1, num_rays=8, seed=0, weight=None, ray_index=None,
                 return_visibility=False):
    """Diffuse lighting under a constant environment of scalar ``radiance`` (the reference's ``constant`` emitter) +
    box-filter film, the shadow rays traced inside the lighting kernel (``hf_sky_lighting``): every sample draws
    ``num_rays`` (1..32) uniform sphere directions from the TEA stream of ``reparameterize_ray`` (``seed``,
    ``ray_index``), traces ``si.spawn_ray(direction)`` for those above its shading hemisphere and averages
    ``albedo/pi * cos * radiance / pdf`` over the unoccluded ones.  Returns the [n // spp] image; with
    ``return_visibility`` also the [n] int32 visibility words (bit k: direction k was traced and reached the sky).
    Differentiable with respect to ``si.sh_frame.n`` and ``weight`` ([n], optional); visibility is piecewise constant."""
    shape._check_ray(ray)
    image, vis = _SkyLightingOp.apply(si.sh_frame.n, weight, shape, si.p, si.n, ray.d, si.t, float(radiance), float(albedo),
                                      int(spp), int(num_rays), int(seed), _check_ray_index(ray_index, ray))
    return (image, vis) if return_visibility else image


def sky_rays(si, ray, k, seed=0, ray_index=None):
    """Shadow ray ``k`` of every sample of ``sky_lighting`` as a Ray3f (``hf_sky_rays``): what the fused kernel traces
    for that direction, bit for bit.  Lanes it does not trace (no hit, seen from behind, direction below the shading
    hemisphere) get ``maxt = -1``, a miss."""
    rid = _check_ray_index(ray_index, ray)
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        check(_capi.lib().hf_sky_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                      tt.data_ptr(), int(k), int(seed), _ptr(rid), C.byref(_p3(r.o)), C.byref(_p3(r.d)),
                                      r.maxt.data_ptr(), _stream_of(pp.device)))
    return r


class Receiver:
    """The plane a caustic lands on (``hf_receiver_t``): the world point ``origin`` at film position (0, 0) and the two
    orthogonal vectors ``ex``, ``ey`` with film x = <X - origin, ex>, y = <X - origin, ey> in pixels."""

    def __init__(self, origin, ex, ey):
        self.origin, self.ex, self.ey = (tuple(float(c) for c in v) for v in (origin, ex, ey))
        assert all(len(v) == 3 for v in (self.origin, self.ex, self.ey)), "origin, ex, ey: three components each"

    @staticmethod
    def plane_z(z, x_range, y_range, width, height):
        """the horizontal plane at height ``z`` whose rectangle x_range x y_range is a film of width x height pixels
        (pixel (0, 0) at the corner (x_range[0], y_range[0]))"""
        sx, sy = width / (x_range[1] - x_range[0]), height / (y_range[1] - y_range[0])
        return Receiver((x_range[0], y_range[0], z), (sx, 0.0, 0.0), (0.0, sy, 0.0))

    def _struct(self):
        return _capi.hf_receiver_t((C.c_float * 3)(*self.origin), (C.c_float * 3)(*self.ex), (C.c_float * 3)(*self.ey))


class _CausticLightingOp(torch.autograd.Function):
    """(pos, value, visibility bytes) of hf_caustic_lighting; backward = hf_caustic_adjoint (gradients of sh_n, p and
    weight), jvp = hf_caustic_tangent.  Both read the visibility byte the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, pp, gn, dd, tt, vis, ww=None):
        """what hf_caustic_adjoint / _tangent start with"""
        eta, power, rcv, act = ctx.misc
        return (sn.shape[1], C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(act),
                _ptr(ww), eta, power, C.byref(rcv), vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, p, weight, shape, nrm, d, t, active, eta, power, receiver):
        sn, pp, gn, dd, tt, ww = map(_detached_f32, (sh_n, p, nrm, d, t, weight))
        n = sn.shape[1]
        ctx.misc = (eta, power, receiver._struct(), active)
        pos = torch.empty((2, n), dtype=torch.float32, device=sn.device)
        value = torch.empty(n, dtype=torch.float32, device=sn.device)
        vis = torch.empty(n, dtype=torch.uint8, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_caustic_lighting(shape._h, n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                  C.byref(_p3(dd)), tt.data_ptr(), _ptr(active), _ptr(ww), eta, power,
                                                  C.byref(ctx.misc[2]), _ref(_row_ptrs(pos)), value.data_ptr(),
                                                  vis.data_ptr(), _stream_of(sn.device)))
        saved = _with_weight(ctx, (sn, pp, gn, dd, tt, vis), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return pos, value, vis

    @staticmethod
    def jvp(ctx, dsh_n, dp, dweight, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dq = _detached_f32(dp)
        dpos, dvalue = torch.empty((2, sn.shape[1]), dtype=torch.float32, device=sn.device), torch.empty_like(sn[0])
        if sn.shape[1]:
            check(_capi.lib().hf_caustic_tangent(*_CausticLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                 _ref(_row_ptrs(dq)), _ptr(dw), _ref(_row_ptrs(dpos)), dvalue.data_ptr(),
                                                 _stream_of(sn.device)))
        return dpos, dvalue, None

    @staticmethod
    def backward(ctx, grad_pos, grad_value, _grad_vis):
        saved = ctx.saved_tensors
        sn = saved[0]
        gq, gv = _detached_f32(grad_pos), _detached_f32(grad_value)
        gn, gp = torch.empty_like(sn), torch.empty_like(sn)
        gw = torch.empty_like(sn[0]) if ctx.weighted else None
        if sn.shape[1]:
            check(_capi.lib().hf_caustic_adjoint(*_CausticLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(gq)), _ptr(gv),
                                                 C.byref(_p3(gn)), C.byref(_p3(gp)), _ptr(gw), _stream_of(sn.device)))
        return (gn, gp, gw) + (None,) * 8


def _caustic_active(active, n, device):
    """``active`` as the [n] uint8 row of the hf_caustic_* entries; True = None: every lane"""
    if active is True or active is None:
        return None
    a = torch.as_tensor(active, device=device)
    return a.to(dtype=torch.uint8).expand(n).contiguous()


def caustic_lighting(shape, si, ray, receiver, eta=1.33, power=1.0, weight=None, active=True, return_visibility=False):
    """Light tracing through the surface (``hf_caustic_lighting``): every sample of the wavefront is a light sample
    that arrives along ``ray.d`` at ``si``, is refracted at ``si.sh_frame.n`` with the relative index ``eta`` (as the
    reference's ``fresnel()`` defines it; the ``dielectric`` BSDF's transmission lobe in importance mode), walked
    against the same terrain up to the ``receiver`` (a ``Receiver``) and, where nothing is in the way, lands there.
    Returns ``(pos [2, n], value [n])``: the landing position in the receiver's film coordinates and the flux
    ``weight * power * (1 - F)``; a sample that deposits nothing has value 0 and pos (-16, -16), outside every film.  With
    ``return_visibility`` also the [n] uint8 row (1: deposited).  Differentiable with respect to ``si.sh_frame.n``,
    ``si.p`` and ``weight`` ([n], optional), in reverse and forward mode; the masks and the occlusion are piecewise
    constant.  Splat the result with ``caustic_film``."""
    shape._check_ray(ray)
    n = len(ray)
    pos, value, vis = _CausticLightingOp.apply(si.sh_frame.n, si.p, weight, shape, si.n, ray.d, si.t,
                                               _caustic_active(active, n, ray.d.device), float(eta), float(power), receiver)
    return (pos, value, vis) if return_visibility else (pos, value)


def caustic_rays(si, ray, receiver, eta=1.33, active=True):
    """The refracted ray of every sample of ``caustic_lighting`` as a Ray3f (``hf_caustic_rays``): what the fused kernel
    walks, bit for bit; ``maxt`` is the distance to the receiver.  Lanes it does not trace (no hit, the normals disagree
    on the side, total internal reflection, a receiver behind the ray) get ``maxt = -1``, a miss, and a zero ray."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        rcv = receiver._struct()
        check(_capi.lib().hf_caustic_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                          tt.data_ptr(), _ptr(_caustic_active(active, n, pp.device)), float(eta),
                                          C.byref(rcv), C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(),
                                          _stream_of(pp.device)))
    return r


def caustic_filter_mass(stddev=0.5):
    """The integral of the film's filter over its window, squared: w(x) = exp(-x^2 / (2 stddev^2)) - exp(-8) on
    |x| <= 4 stddev (src/rfilters/gaussian.cpp), so int w = stddev (sqrt(2 pi) erf(2 sqrt(2)) - 8 exp(-8))."""
    return (stddev * (math.sqrt(2.0 * math.pi) * math.erf(2.0 * math.sqrt(2.0)) - 8.0 * math.exp(-8.0))) ** 2


def caustic_film(pos, value, width, height, stddev=0.5):
    """The film of a light tracer: the ACCUMULATED image plane of ``hf_film_splat_weighted`` for the samples of
    ``caustic_lighting``, [height * width] -- a sum, not an average, so it is not divided by the weight plane.  It is
    divided by the filter's mass ``caustic_filter_mass(stddev)``, a closed-form constant (0.6248 pixel^2 for stddev 0.5),
    which makes a pixel hold the flux that lands on it: sum(film) = sum(value) for samples well inside the film, to
    within the lattice ripple of the filter (2 exp(-2 pi^2 stddev^2) per axis and sample: 1.4 % for stddev 0.5).
    Differentiable with respect to ``pos`` and ``value``."""
    image, _ = _FilmMotionOp.apply(value[None], pos, None, int(width), int(height), float(stddev))
    return image[0] / caustic_filter_mass(float(stddev))


class _EnvmapEvalOp(torch.autograd.Function):
    """hf_envmap_eval of the map `full` ([H, W], the seam column included) for world directions; linear in the texels:
    backward = hf_envmap_eval_adjoint, jvp = hf_envmap_eval of the texels' tangent."""

    @staticmethod
    def _eval(dat, dd, act, rot):
        out = torch.empty(dd.shape[1], dtype=torch.float32, device=dd.device)
        if dd.shape[1]:
            check(_capi.lib().hf_envmap_eval(dd.shape[1], C.byref(_p3(dd)), _ptr(act), dat.shape[1], dat.shape[0],
                                             dat.data_ptr(), C.byref(rot), out.data_ptr(), _stream_of(dd.device)))
        return out

    @staticmethod
    def forward(ctx, full, d, active, rot):
        dat = full.detach().to(dtype=torch.float32).contiguous()
        dd = d.detach().to(dtype=torch.float32).contiguous()
        act = active.to(dtype=torch.uint8).contiguous() if active is not None else None
        ctx.misc = (act, rot, tuple(dat.shape))
        ctx.save_for_backward(dd)
        ctx.save_for_forward(dd)
        return _EnvmapEvalOp._eval(dat, dd, act, rot)

    @staticmethod
    def jvp(ctx, dfull, *_):
        act, rot, shape = ctx.misc
        dd, = ctx.saved_tensors
        if dfull is None:
            return torch.zeros(dd.shape[1], dtype=torch.float32, device=dd.device)
        return _EnvmapEvalOp._eval(_texel_tangent(dfull), dd, act, rot)

    @staticmethod
    def backward(ctx, grad_out):
        act, rot, (H, W) = ctx.misc
        dd, = ctx.saved_tensors
        gd = torch.zeros((H, W), dtype=torch.float32, device=dd.device)
        if dd.shape[1]:
            go = grad_out.to(dtype=torch.float32).contiguous()
            check(_capi.lib().hf_envmap_eval_adjoint(dd.shape[1], C.byref(_p3(dd)), _ptr(act), W, H, C.byref(rot),
                                                     go.data_ptr(), gd.data_ptr(), _stream_of(dd.device)))
        return gd, None, None, None


class Envmap:
    """The reference's ``envmap`` emitter (src/emitters/envmap.cpp) for one channel: a latitude-longitude map of scalar
    radiance, row 0 the north pole (the map's +Y).  ``data``: [H, W0] float32 device tensor (W0 >= 1, H >= 2), kept by
    reference -- it may require grad; the seam column (a copy of column 0, envmap.cpp:147, 249-258) is appended with
    ``torch.cat`` at every use, so autograd folds its gradient back onto column 0.  ``to_world``: 3 x 3 rotation from the
    map's space to world, default the one that takes the map's +Y to world +Z (Rectangle's object space is Z-up);
    detached.  ``defensive``: the fraction u in [0, 1] of the sampling distribution that is spread evenly over the cells
    (include/hf.h); 0 samples in proportion to luminance, a positive value keeps dark texels reachable while the texels
    are optimised.  The object owns the sampling table (``hf_envmap_build_table``) and rebuilds it when ``data`` has been
    written to (its version counter) and in ``parameters_changed()``."""

    def __init__(self, data, to_world=None, defensive=0.0):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32:
            data = torch.as_tensor(data, dtype=torch.float32)
        if data.dim() != 2 or data.shape[0] < 2 or data.shape[1] < 1:
            raise ValueError("Envmap: data must be [H >= 2, W0 >= 1]")
        if not 0.0 <= float(defensive) <= 1.0:
            raise ValueError("Envmap: defensive must lie in [0, 1]")
        self.data = data
        self.defensive = float(defensive)
        tw = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) if to_world is None else \
            torch.as_tensor(to_world, dtype=torch.float32).detach().cpu().reshape(3, 3)
        self.to_world = tw
        self._rot = (C.c_float * 9)(*[float(v) for v in tw.reshape(-1)])
        self._table = None
        self._key = None

    @property
    def resolution(self):
        """(W, H) of the map the kernels read: the seam column included"""
        return self.data.shape[1] + 1, self.data.shape[0]

    def parameters_changed(self, keys=()):
        self._key = None

    def full(self):
        """[H, W0 + 1]: data with its seam column, attached to ``data``"""
        return torch.cat([self.data, self.data[:, :1]], 1)

    def table(self):
        """the sampling table of the current texels (a new tensor whenever it is rebuilt: an earlier one stays valid for
        the backward pass of the call that used it)"""
        key = (self.data._version, self.data.data_ptr(), tuple(self.data.shape), self.defensive)
        if self._table is None or key != self._key:
            W, H = self.resolution
            dat = self.full().detach().contiguous()
            table = torch.empty(_capi.lib().hf_envmap_table_floats(W, H), dtype=torch.float32, device=dat.device)
            check(_capi.lib().hf_envmap_build_table(W, H, dat.data_ptr(), self.defensive, table.data_ptr(),
                                                    _stream_of(dat.device)))
            self._table, self._key = table, key
        return self._table

    def eval(self, d, active=True):
        """radiance seen along the world directions ``d`` [3, n] (Emitter::eval); differentiable in ``data``"""
        act = None if active is True else torch.as_tensor(active, device=d.device).expand(d.shape[1])
        return _EnvmapEvalOp.apply(self.full(), d, act, self._rot)

    def sample_direction(self, sample):
        """Emitter::sample_direction for ``sample`` [2, n] in [0, 1): (ds, weight) with ds.d the world direction, ds.pdf
        the density per solid angle (0 for an invalid draw), ds.cell the index cy (W - 1) + cx of the drawn cell, ds.frac
        ([2, n]) the position in it and weight = radiance / pdf.  The distribution is detached; so are the returned values."""
        W, H = self.resolution
        s = sample.detach().to(dtype=torch.float32).contiguous()
        n = s.shape[1]
        dat, table = self.full().detach().contiguous(), self.table()
        d = torch.empty((3, n), dtype=torch.float32, device=s.device)
        weight, pdf = torch.empty_like(s[0]), torch.empty_like(s[0])
        cell = torch.empty(n, dtype=torch.int32, device=s.device)
        frac = torch.empty_like(s)
        if n:
            check(_capi.lib().hf_envmap_sample_direction(n, C.byref(_row_ptrs(s)), W, H, dat.data_ptr(), table.data_ptr(),
                                                         C.byref(self._rot), C.byref(_p3(d)), weight.data_ptr(),
                                                         pdf.data_ptr(), cell.data_ptr(), C.byref(_row_ptrs(frac)),
                                                         _stream_of(s.device)))
        ds = DirectionSample3f(PositionSample3f(None, -d, None, None, pdf, False), d, math.inf)
        ds.cell, ds.frac = cell, frac
        return ds, weight

    def pdf_direction(self, d):
        """density per solid angle with which ``sample_direction`` draws the world directions ``d`` [3, n]: plain torch
        over the table's header and the texels (not a hot path)"""
        W, H = self.resolution
        dat, table = self.full().detach(), self.table()
        sigma, mbar, u = table[0], table[1], table[2]
        # (the lookup in double, as hf_envmap_eval does it: near a pole it amplifies an input error by 1 / theta)
        v = torch.nan_to_num(self.to_world.to(device=d.device, dtype=torch.float64).T @ d.detach().to(dtype=torch.float64))
        ux = torch.atan2(v[0], -v[2]) / (2.0 * math.pi) - 0.5 / (W - 1)
        uy = torch.acos(v[1].clamp(-1.0, 1.0)) / math.pi
        ux = (ux - torch.floor(ux)) * (W - 1); uy = (uy - torch.floor(uy)) * (H - 1)
        cx = ux.long().clamp(0, W - 2); cy = uy.long().clamp(0, H - 2)
        p = dat.clamp(min=0.0)
        mc = 0.25 * ((p[cy, cx] + p[cy, cx + 1]) + (p[cy + 1, cx] + p[cy + 1, cx + 1]))
        wc = torch.sin(math.pi * (cy + 0.5) / (H - 1)) * ((1.0 - u) * mc + u * mbar)
        st = torch.sqrt(v[0] * v[0] + v[2] * v[2]).clamp(min=1e-12)   # sin theta as envmap.cpp:403-415 takes it: well conditioned at the poles
        pdf = (wc * ((W - 1) * (H - 1)) / sigma / (2.0 * math.pi ** 2 * st)).to(torch.float32)
        return torch.where((sigma > 0) & (wc > 0), pdf, torch.zeros_like(pdf))


class _EnvmapLightingOp(torch.autograd.Function):
    """(image, visibility words) of hf_envmap_lighting; backward = hf_envmap_lighting_adjoint (gradients of sh_n, weight and
    the texels), jvp = hf_envmap_lighting_tangent.  Both read the visibility word and the table the forward saved and
    trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, dd, tt, vis, dat, table, ww=None):
        """what hf_envmap_lighting_adjoint / _tangent start with"""
        spp, num_rays, seed, rid, rot, albedo = ctx.misc
        return (sn.shape[1], spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(rid),
                dat.shape[1], dat.shape[0], dat.data_ptr(), table.data_ptr(), C.byref(rot), albedo, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, weight, full, shape, p, nrm, d, t, table, rot, albedo, spp, num_rays, seed, ray_index):
        sn, pp, gn, dd, tt, ww, dat = map(_detached_f32, (sh_n, p, nrm, d, t, weight, full))
        n = sn.shape[1]
        ctx.misc = (spp, num_rays, seed, ray_index, rot, albedo)
        image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=sn.device)
        vis = torch.empty(n, dtype=torch.int32, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_envmap_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                 C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(ray_index),
                                                 dat.shape[1], dat.shape[0], dat.data_ptr(), table.data_ptr(), C.byref(rot),
                                                 albedo, image.data_ptr(), vis.data_ptr(), _stream_of(sn.device)))
        saved = _with_weight(ctx, (sn, dd, tt, vis, dat, table), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, vis

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dfull, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        df = _texel_tangent(dfull)
        dimage = torch.empty(sn.shape[1] // ctx.misc[0], dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_envmap_lighting_tangent(*_EnvmapLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                         _ptr(dw), _ptr(df), dimage.data_ptr(), _stream_of(sn.device)))
        return dimage, None

    @staticmethod
    def backward(ctx, grad_image, _grad_vis):
        saved = ctx.saved_tensors
        sn, dat = saved[0], saved[4]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gd = _texel_grad(ctx, 2, dat)
        if sn.shape[1]:
            check(_capi.lib().hf_envmap_lighting_adjoint(*_EnvmapLightingOp._prefix(ctx, *saved), gi.data_ptr(),
                                                         C.byref(_p3(gn)), _ptr(gw), _ptr(gd), _stream_of(sn.device)))
        return (gn, gw, gd) + (None,) * 12


def envmap_lighting(shape, si, ray, envmap, albedo=1.0, spp=1, num_rays=8, seed=0, weight=None, ray_index=None,
                    return_visibility=False):
    """Diffuse lighting under an environment map (``Envmap``; the reference's ``envmap`` emitter) + box-filter film, the
    shadow rays traced inside the lighting kernel (``hf_envmap_lighting``): every sample draws ``num_rays`` (1..32)
    directions by importance sampling of the map from the TEA stream of ``sky_lighting`` (``seed``, ``ray_index``), traces
    ``si.spawn_ray(direction)`` for those above its shading hemisphere and averages ``albedo/pi * cos * radiance / pdf``
    over the unoccluded ones.  Returns the [n // spp] image; with ``return_visibility`` also the [n] int32 visibility
    words.  Differentiable with respect to ``si.sh_frame.n``, ``weight`` ([n], optional) and ``envmap.data``; visibility
    and the sampling distribution are detached."""
    shape._check_ray(ray)
    image, vis = _EnvmapLightingOp.apply(si.sh_frame.n, weight, envmap.full(), shape, si.p, si.n, ray.d, si.t, envmap.table(),
                                         envmap._rot, float(albedo), int(spp), int(num_rays), int(seed),
                                         _check_ray_index(ray_index, ray))
    return (image, vis) if return_visibility else image


def envmap_rays(si, ray, envmap, k, seed=0, ray_index=None, return_weight=False):
    """Shadow ray ``k`` of every sample of ``envmap_lighting`` as a Ray3f (``hf_envmap_rays``): what the fused kernel
    traces for that direction, bit for bit.  Lanes it does not trace (no hit, seen from behind, an invalid draw,
    direction below the shading hemisphere) get ``maxt = -1``, a miss.  ``return_weight``: also the emitter weights
    ``radiance / pdf`` of the draws ([n])."""
    rid = _check_ray_index(ray_index, ray)
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    W, H = envmap.resolution
    dat, table = envmap.full().detach().contiguous(), envmap.table()
    wgt = torch.empty(n, dtype=torch.float32, device=pp.device) if return_weight else None
    if n:
        check(_capi.lib().hf_envmap_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                         tt.data_ptr(), int(k), int(seed), _ptr(rid), W, H, dat.data_ptr(), table.data_ptr(),
                                         C.byref(envmap._rot), C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(),
                                         _ptr(wgt), _stream_of(pp.device)))
    return (r, wgt) if return_weight else r


# ---- what the two reflection Functions (reflect, glossy) are made of.  `entry`: the C entry's name; `mid(ctx, dat, ww,
# *extra)`: the row's C arguments between t and its outputs (derivatives: its visibility row); `extra`: the row's further
# differentiable rows (glossy: alpha), which follow sh_n and weight among the inputs, the tangents and the gradients ----
def _reflection_forward(ctx, entry, mid, vis_dtype, shape, sh_n, p, nrm, d, t, weight, full, *extra):
    """(image, value, vis) of a forward entry; saves (sn, dd, tt, vis, dat, *extra[, weight]).  ctx.misc[0] is spp"""
    sn, pp, gn, dd, tt, ww, dat = map(_detached_f32, (sh_n, p, nrm, d, t, weight, full))
    extra = tuple(map(_detached_f32, extra))
    n, spp = sn.shape[1], ctx.misc[0]
    image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=sn.device)
    value = torch.empty(n, dtype=torch.float32, device=sn.device)
    vis = torch.empty(n, dtype=vis_dtype, device=sn.device)
    if n:  # (an empty wavefront has no rows to point to)
        check(getattr(_capi.lib(), entry)(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                          C.byref(_p3(dd)), tt.data_ptr(), *mid(ctx, dat, ww, *extra), image.data_ptr(),
                                          value.data_ptr(), vis.data_ptr(), _stream_of(sn.device)))
    saved = _with_weight(ctx, (sn, dd, tt, vis, dat) + extra, ww)
    ctx.save_for_backward(*saved)
    ctx.save_for_forward(*saved)
    ctx.mark_non_differentiable(vis)
    return image, value, vis


def _reflection_prefix(ctx, mid):
    """what a row's _adjoint / _tangent entries start with"""
    sn, dd, tt, vis, dat, *extra = ctx.saved_tensors
    ww = extra.pop() if ctx.weighted else None
    return (sn.shape[1], ctx.misc[0], C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), *mid(ctx, dat, ww, *extra),
            vis.data_ptr())


def _reflection_jvp(ctx, entry, mid, dsh_n, dweight, dfull, *dextra):
    sn = ctx.saved_tensors[0]
    dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
    dx, df = tuple(map(_detached_f32, dextra)), _texel_tangent(dfull)   # (held until the call has been enqueued)
    dimage = torch.empty(sn.shape[1] // max(ctx.misc[0], 1), dtype=torch.float32, device=sn.device)
    dvalue = torch.empty_like(sn[0])
    if sn.shape[1]:
        check(getattr(_capi.lib(), entry)(*_reflection_prefix(ctx, mid), _ref(_row_ptrs(dn)), _ptr(dw), *map(_ptr, dx),
                                          _ptr(df), dimage.data_ptr(), dvalue.data_ptr(), _stream_of(sn.device)))
    return dimage, dvalue, None


def _reflection_backward(ctx, entry, mid, grad_image, grad_value, n_extra=0):
    """the gradients of sh_n, weight, the `n_extra` further rows and the texels (inputs 0, 1, 2 .. and 2 + n_extra)"""
    sn, dat = ctx.saved_tensors[0], ctx.saved_tensors[4]
    gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
    gv = _detached_f32(grad_value)
    gx = tuple(torch.empty_like(sn[0]) if ctx.needs_input_grad[2 + j] else None for j in range(n_extra))
    gd = _texel_grad(ctx, 2 + n_extra, dat)
    if sn.shape[1]:
        check(getattr(_capi.lib(), entry)(*_reflection_prefix(ctx, mid), _ptr(gi), _ptr(gv), C.byref(_p3(gn)), _ptr(gw),
                                          *map(_ptr, gx), _ptr(gd), _stream_of(sn.device)))
    return (gn, gw) + gx + (gd,)


def _value_outputs(image, value, vis, return_value, return_visibility):
    """what reflection_lighting and glossy_lighting return: the image, then what was asked for of value and visibility"""
    out = (image,) + ((value,) if return_value else ()) + ((vis,) if return_visibility else ())
    return out if len(out) > 1 else image


class _ReflectionLightingOp(torch.autograd.Function):
    """(image, per-sample value, visibility bytes) of hf_reflect_lighting; backward = hf_reflect_lighting_adjoint (gradients
    of sh_n, weight and the texels), jvp = hf_reflect_lighting_tangent.  Both read the visibility byte the forward saved
    and trace nothing."""

    @staticmethod
    def _mid(ctx, dat, ww):
        spp, eta, rot, act = ctx.misc
        return (_ptr(act), _ptr(ww), eta, dat.shape[1], dat.shape[0], dat.data_ptr(), C.byref(rot))

    @staticmethod
    def forward(ctx, sh_n, weight, full, shape, p, nrm, d, t, active, rot, eta, spp):
        ctx.misc = (spp, eta, rot, active)
        return _reflection_forward(ctx, "hf_reflect_lighting", _ReflectionLightingOp._mid, torch.uint8, shape, sh_n, p, nrm,
                                   d, t, weight, full)

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dfull, *_):
        return _reflection_jvp(ctx, "hf_reflect_lighting_tangent", _ReflectionLightingOp._mid, dsh_n, dweight, dfull)

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis):
        return _reflection_backward(ctx, "hf_reflect_lighting_adjoint", _ReflectionLightingOp._mid, grad_image,
                                    grad_value) + (None,) * 9


def reflection_lighting(shape, si, ray, envmap, eta=0.0, spp=1, weight=None, active=True, return_value=False,
                        return_visibility=False):
    """Specular reflection of an environment map (``Envmap``) + box-filter film, the mirror ray traced inside the lighting
    kernel (``hf_reflect_lighting``): every sample is reflected at ``si.sh_frame.n`` (``reflect(wi, m)``), the ray
    ``si.spawn_ray(wr)`` is walked against the terrain and, where it escapes, the sample's value is ``weight * F *
    envmap.eval(wr)`` with ``F`` the Fresnel reflectance of the relative index ``eta`` (``fresnel()``; ``eta = 0``: an ideal
    mirror, F = 1).  A reflected ray that hits the terrain contributes 0 (no second vertex).  Returns the [n // spp] image;
    with ``return_value`` also the [n] per-sample values (what ``film_gaussian(..., weight=)`` consumes) and with
    ``return_visibility`` the [n] uint8 row (1: the mirror ray escapes).  Differentiable with respect to
    ``si.sh_frame.n``, ``weight`` ([n], optional: the specular reflectance) and ``envmap.data``, in reverse and forward
    mode; the masks, the visibility and the cell of the lookup are piecewise constant."""
    shape._check_ray(ray)
    image, value, vis = _ReflectionLightingOp.apply(si.sh_frame.n, weight, envmap.full(), shape, si.p, si.n, ray.d, si.t,
                                                    _caustic_active(active, len(ray), ray.d.device), envmap._rot, float(eta),
                                                    int(spp))
    return _value_outputs(image, value, vis, return_value, return_visibility)


def reflection_rays(si, ray, active=True):
    """The reflected ray of every sample of ``reflection_lighting`` as a Ray3f (``hf_reflect_rays``): what the fused
    kernel walks, bit for bit.  Lanes it does not trace (no hit, seen from behind, a mirror direction below the true
    surface) get ``maxt = -1``, a miss, and a zero ray."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        check(_capi.lib().hf_reflect_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                          tt.data_ptr(), _ptr(_caustic_active(active, n, pp.device)), C.byref(_p3(r.o)),
                                          C.byref(_p3(r.d)), r.maxt.data_ptr(), _stream_of(pp.device)))
    return r


class _GlossyLightingOp(torch.autograd.Function):
    """(image, per-sample value, visibility words) of hf_glossy_lighting; backward = hf_glossy_lighting_adjoint (gradients
    of sh_n, weight, alpha and the texels), jvp = hf_glossy_lighting_tangent.  Both read the visibility word the forward
    saved, draw the microfacet normals again and trace nothing."""

    @staticmethod
    def _mid(ctx, dat, ww, al):
        spp, eta, num_rays, seed, rid, rot, act = ctx.misc
        return (_ptr(act), _ptr(ww), al.data_ptr(), eta, num_rays, seed, _ptr(rid), dat.shape[1], dat.shape[0], dat.data_ptr(),
                C.byref(rot))

    @staticmethod
    def forward(ctx, sh_n, weight, alpha, full, shape, p, nrm, d, t, active, rot, eta, spp, num_rays, seed, ray_index):
        ctx.misc = (spp, eta, num_rays, seed, ray_index, rot, active)
        return _reflection_forward(ctx, "hf_glossy_lighting", _GlossyLightingOp._mid, torch.int32, shape, sh_n, p, nrm, d, t,
                                   weight, full, alpha)

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dalpha, dfull, *_):
        return _reflection_jvp(ctx, "hf_glossy_lighting_tangent", _GlossyLightingOp._mid, dsh_n, dweight, dfull, dalpha)

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis):
        return _reflection_backward(ctx, "hf_glossy_lighting_adjoint", _GlossyLightingOp._mid, grad_image, grad_value,
                                    n_extra=1) + (None,) * 12


def _glossy_alpha(alpha, n, device):
    """``alpha`` (a float, or a tensor of 1 or n elements) as the [n] float32 row of the hf_glossy_* entries; a scalar is
    broadcast here, so its gradient is the sum torch forms"""
    a = torch.as_tensor(alpha, dtype=torch.float32, device=device).reshape(-1)
    if a.numel() not in (1, n):
        raise ValueError("alpha must be a float or a tensor of 1 or %d elements (got %d)" % (n, a.numel()))
    return a.expand(n)


def glossy_lighting(shape, si, ray, envmap, alpha, eta=0.0, spp=1, num_rays=4, seed=0, weight=None, ray_index=None,
                    active=True, return_value=False, return_visibility=False):
    """Glossy reflection of an environment map (``Envmap``) + box-filter film (``hf_glossy_lighting``): the reflection
    lobe of a rough conductor or dielectric with an isotropic GGX distribution of roughness ``alpha`` (a float, or a
    tensor of 1 or n elements, e.g. a roughness texture read through ``eval_attribute``).  Every sample draws
    ``num_rays`` (1..32) microfacet normals about ``si.sh_frame.n`` by visible-normal sampling from the TEA stream of
    ``sky_lighting`` (``seed``, ``ray_index``), mirrors ``wi`` at each, walks ``si.spawn_ray(wo)`` against the terrain
    inside the kernel and averages ``weight * F * G1(wo) * envmap.eval(wo)`` over the rays that escape (``F``: the
    Fresnel reflectance of the relative index ``eta``; ``eta = 0``: F = 1).  A reflected ray that hits the terrain
    contributes 0.  Returns the [n // spp] image; with ``return_value`` also the [n] per-sample values and with
    ``return_visibility`` the [n] int32 words (bit k: mirror ray k escapes).  Differentiable with respect to
    ``si.sh_frame.n``, ``weight`` ([n], optional: the specular reflectance), ``alpha`` and ``envmap.data``, in reverse and
    forward mode, with the drawn directions held (detached sampling, attached evaluation).  The variance of the estimator
    grows as ``alpha`` falls: a near-mirror belongs to ``reflection_lighting``."""
    shape._check_ray(ray)
    n = len(ray)
    image, value, vis = _GlossyLightingOp.apply(si.sh_frame.n, weight, _glossy_alpha(alpha, n, ray.d.device), envmap.full(),
                                                shape, si.p, si.n, ray.d, si.t, _caustic_active(active, n, ray.d.device),
                                                envmap._rot, float(eta), int(spp), int(num_rays), int(seed),
                                                _check_ray_index(ray_index, ray))
    return _value_outputs(image, value, vis, return_value, return_visibility)


def glossy_rays(si, ray, alpha, k, seed=0, ray_index=None, active=True, return_normal=False):
    """Mirror ray ``k`` of every sample of ``glossy_lighting`` as a Ray3f (``hf_glossy_rays``): what the fused kernel walks
    for that direction, bit for bit.  Lanes it does not trace get ``maxt = -1``, a miss, and a zero ray.  With
    ``return_normal`` also the [3, n] microfacet normals (zero for an invalid draw)."""
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    h = torch.empty_like(pp) if return_normal else None
    al = _glossy_alpha(alpha, n, pp.device).detach().contiguous()
    rid = _check_ray_index(ray_index, ray)
    if n:
        check(_capi.lib().hf_glossy_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                         tt.data_ptr(), _ptr(_caustic_active(active, n, pp.device)), al.data_ptr(), int(k),
                                         int(seed), _ptr(rid), C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(),
                                         _ref(_row_ptrs(h)), _stream_of(pp.device)))
    return (r, h) if return_normal else r


_WRAPS = {"clamp": _capi.HF_WRAP_CLAMP, "repeat": _capi.HF_WRAP_REPEAT}


def _bitmap_in(dat, wrap):
    """the texture's C arguments: TW, TH, tex, wrap"""
    return dat.shape[1], dat.shape[0], dat.data_ptr(), wrap


class _BitmapEvalOp(torch.autograd.Function):
    """hf_bitmap_eval of the texture `data` ([TH, TW]) at film positions; backward = hf_bitmap_eval_adjoint (gradients of
    the texels and of the positions, the cell held), jvp = hf_bitmap_eval of the texels' tangent + (Lx, Ly) . dpos."""

    @staticmethod
    def _eval(dat, pp, act, wrap, slopes=False):
        n = pp.shape[1]
        out = torch.empty(n, dtype=torch.float32, device=pp.device)
        grad = torch.empty((2, n), dtype=torch.float32, device=pp.device) if slopes else None
        if n:
            check(_capi.lib().hf_bitmap_eval(n, _ref(_row_ptrs(pp)), _ptr(act), *_bitmap_in(dat, wrap), out.data_ptr(),
                                             _ref(_row_ptrs(grad)), _stream_of(pp.device)))
        return (out, grad) if slopes else out

    @staticmethod
    def forward(ctx, data, pos, active, wrap):
        dat, pp = _detached_f32(data), _detached_f32(pos)
        ctx.misc = (active, wrap)
        ctx.save_for_backward(dat, pp)
        ctx.save_for_forward(dat, pp)
        return _BitmapEvalOp._eval(dat, pp, active, wrap)

    @staticmethod
    def jvp(ctx, ddata, dpos, *_):
        act, wrap = ctx.misc
        dat, pp = ctx.saved_tensors
        out = torch.zeros(pp.shape[1], dtype=torch.float32, device=pp.device)
        if ddata is not None:
            out = _BitmapEvalOp._eval(_texel_tangent(ddata), pp, act, wrap)
        if dpos is not None:
            _, slopes = _BitmapEvalOp._eval(dat, pp, act, wrap, slopes=True)
            out = out + (slopes * dpos.to(dtype=torch.float32)).sum(0)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        act, wrap = ctx.misc
        dat, pp = ctx.saved_tensors
        gd = _texel_grad(ctx, 0, dat)
        gp = torch.zeros_like(pp) if ctx.needs_input_grad[1] else None
        if pp.shape[1] and (gd is not None or gp is not None):
            go = _detached_f32(grad_out)
            check(_capi.lib().hf_bitmap_eval_adjoint(pp.shape[1], _ref(_row_ptrs(pp)), _ptr(act), *_bitmap_in(dat, wrap),
                                                     go.data_ptr(), _ref(_row_ptrs(gp)), _ptr(gd), _stream_of(pp.device)))
        return gd, gp, None, None


class Bitmap:
    """The reference's ``bitmap`` texture (src/textures/bitmap.cpp) for one channel with the bilinear filter, laid on a
    ``Receiver``: a film position of the receiver is a texel coordinate, texel (ix, iy) has its centre at
    ``(ix + 0.5, iy + 0.5)``.  ``data``: [TH, TW] float32 device tensor, kept by reference -- it may require grad.
    ``wrap``: ``"clamp"`` or ``"repeat"``."""

    def __init__(self, data, wrap="clamp"):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32:
            data = torch.as_tensor(data, dtype=torch.float32)
        if data.dim() != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError("Bitmap: data must be [TH >= 1, TW >= 1]")
        if wrap not in _WRAPS:
            raise ValueError("Bitmap: wrap must be 'clamp' or 'repeat' (got %r)" % (wrap,))
        self.data = data
        self.wrap = wrap

    @property
    def resolution(self):
        """(TW, TH)"""
        return self.data.shape[1], self.data.shape[0]

    def eval(self, pos, active=True):
        """the texture at the film positions ``pos`` [2, n] (``hf_bitmap_eval``), 0 on inactive lanes; differentiable in
        ``pos`` (with the cell held) and in ``data``, in reverse and forward mode"""
        return _BitmapEvalOp.apply(self.data, pos, _caustic_active(active, pos.shape[1], pos.device), _WRAPS[self.wrap])


class _RefractionLightingOp(torch.autograd.Function):
    """(image, per-sample value, visibility bytes, landing positions) of hf_refract_lighting; backward =
    hf_refract_lighting_adjoint (gradients of sh_n, p, weight and the texels), jvp = hf_refract_lighting_tangent.  Both
    read the visibility byte the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, pp, gn, dd, tt, vis, dat, ww=None):
        """what hf_refract_lighting_adjoint / _tangent start with"""
        spp, eta, sigma_t, rcv, wrap, act = ctx.misc
        return (sn.shape[1], spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(),
                _ptr(act), _ptr(ww), eta, sigma_t, C.byref(rcv), *_bitmap_in(dat, wrap), vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, p, weight, data, shape, nrm, d, t, active, eta, sigma_t, receiver, wrap, spp):
        sn, pp, gn, dd, tt, ww, dat = map(_detached_f32, (sh_n, p, nrm, d, t, weight, data))
        n = sn.shape[1]
        ctx.misc = (spp, eta, sigma_t, receiver._struct(), wrap, active)
        image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=sn.device)
        value = torch.empty(n, dtype=torch.float32, device=sn.device)
        vis = torch.empty(n, dtype=torch.uint8, device=sn.device)
        pos = torch.empty((2, n), dtype=torch.float32, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_refract_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                  C.byref(_p3(dd)), tt.data_ptr(), _ptr(active), _ptr(ww), eta, sigma_t,
                                                  C.byref(ctx.misc[3]), *_bitmap_in(dat, wrap), image.data_ptr(),
                                                  value.data_ptr(), vis.data_ptr(), _ref(_row_ptrs(pos)),
                                                  _stream_of(sn.device)))
        saved = _with_weight(ctx, (sn, pp, gn, dd, tt, vis, dat), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis, pos)
        return image, value, vis, pos

    @staticmethod
    def jvp(ctx, dsh_n, dp, dweight, ddata, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dq, df = _detached_f32(dp), _texel_tangent(ddata)   # (held until the call has been enqueued)
        dimage = torch.empty(sn.shape[1] // max(ctx.misc[0], 1), dtype=torch.float32, device=sn.device)
        dvalue = torch.empty_like(sn[0])
        if sn.shape[1]:
            check(_capi.lib().hf_refract_lighting_tangent(*_RefractionLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                          _ref(_row_ptrs(dq)), _ptr(dw), _ptr(df), dimage.data_ptr(),
                                                          dvalue.data_ptr(), _stream_of(sn.device)))
        return dimage, dvalue, None, None

    @staticmethod
    def backward(ctx, grad_image, grad_value, _grad_vis, _grad_pos):
        saved = ctx.saved_tensors
        sn, dat = saved[0], saved[6]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gv, gp, gd = _detached_f32(grad_value), torch.empty_like(sn), _texel_grad(ctx, 3, dat)
        if sn.shape[1]:
            check(_capi.lib().hf_refract_lighting_adjoint(*_RefractionLightingOp._prefix(ctx, *saved), _ptr(gi), _ptr(gv),
                                                          C.byref(_p3(gn)), C.byref(_p3(gp)), _ptr(gw), _ptr(gd),
                                                          _stream_of(sn.device)))
        return (gn, gp, gw, gd) + (None,) * 10


def refraction_lighting(shape, si, ray, receiver, bitmap, eta=1.33, sigma_t=0.0, spp=1, weight=None, active=True,
                        return_value=False, return_visibility=False, return_position=False):
    """The refraction view + box-filter film (``hf_refract_lighting``): every sample of the wavefront looks along
    ``ray.d``, is refracted at ``si.sh_frame.n`` with the relative index ``eta`` (the ``dielectric`` BSDF's transmission
    lobe in radiance mode), walked against the same terrain up to the ``receiver`` (a ``Receiver``) and, where nothing is
    in the way, sees the ``bitmap`` (a ``Bitmap`` laid on the receiver) where it lands: the sample's value is
    ``weight * (1 - F) * eta_ti^2 * exp(-sigma_t * s) * bitmap.eval(pos)`` with ``s`` the length of the transmitted
    segment.  A transmitted ray that hits the terrain contributes 0 (no second vertex).  Returns the [n // spp] image;
    with ``return_value`` also the [n] per-sample values, with ``return_visibility`` the [n] uint8 row (1: the receiver
    is seen) and with ``return_position`` the [2, n] landing positions ((-16, -16) where nothing is seen; detached: their
    derivatives are ``caustic_lighting``'s).  Differentiable with respect to ``si.sh_frame.n``, ``si.p``, ``weight`` ([n],
    optional) and ``bitmap.data``, in reverse and forward mode; the masks, the visibility and the cell of the lookup are
    piecewise constant, ``sigma_t`` is a constant."""
    shape._check_ray(ray)
    image, value, vis, pos = _RefractionLightingOp.apply(si.sh_frame.n, si.p, weight, bitmap.data, shape, si.n, ray.d, si.t,
                                                         _caustic_active(active, len(ray), ray.d.device), float(eta),
                                                         float(sigma_t), receiver, _WRAPS[bitmap.wrap], int(spp))
    out = _value_outputs(image, value, vis, return_value, return_visibility)
    if return_position:
        out = (out if isinstance(out, tuple) else (out,)) + (pos,)
    return out


def dielectric_lighting(shape, si, ray, envmap, receiver, bitmap, eta=1.33, sigma_t=0.0, spp=1, weight=None, active=True):
    """Both lobes of a smooth dielectric interface seen from the camera, [n // spp]: ``reflection_lighting(eta)`` (the
    environment map mirrored at the surface, weighted by F) + ``refraction_lighting(eta)`` (the textured receiver seen
    through it, weighted by (1 - F) eta_ti^2).  A plain sum of the two rows: no kernel of its own."""
    return reflection_lighting(shape, si, ray, envmap, eta=eta, spp=spp, weight=weight, active=active) + \
        refraction_lighting(shape, si, ray, receiver, bitmap, eta=eta, sigma_t=sigma_t, spp=spp, weight=weight, active=active)


class RectLight:
    """A one-sided ``area`` emitter on a ``rectangle`` (``hf_rect_light_t``): the rectangle [-1, 1]^2 under a to_world
    whose translation is ``center`` and whose images of (1, 0, 0) and (0, 1, 0) are ``ex`` and ``ey``; it emits the scalar
    ``radiance`` on the side of ``normalize(ex x ey)``.  ``texture``: a ``Bitmap`` or a [TH, TW] float32 device tensor
    that multiplies the radiance (bilinear, clamped; texel (0, 0) at the corner ``center - ex - ey``), kept by reference
    -- it may require grad."""

    def __init__(self, center, ex, ey, radiance=1.0, texture=None):
        self.center, self.ex, self.ey = (tuple(float(c) for c in v) for v in (center, ex, ey))
        assert all(len(v) == 3 for v in (self.center, self.ex, self.ey)), "center, ex, ey: three components each"
        self.radiance = float(radiance)
        if isinstance(texture, Bitmap):
            if texture.wrap != "clamp":
                raise ValueError("RectLight: the texture of a lamp is clamped")
            texture = texture.data
        if texture is not None and (not isinstance(texture, torch.Tensor) or texture.dtype != torch.float32 or
                                    texture.dim() != 2 or texture.shape[0] < 1 or texture.shape[1] < 1):
            raise ValueError("RectLight: texture must be a Bitmap or a float32 tensor [TH >= 1, TW >= 1]")
        self.texture = texture

    @staticmethod
    def from_to_world(M, radiance=1.0, texture=None):
        """the lamp of a rectangle with the 3 x 4 (or 4 x 4) to_world ``M``"""
        M = torch.as_tensor(M, dtype=torch.float64).cpu()
        return RectLight(M[:3, 3].tolist(), M[:3, 0].tolist(), M[:3, 1].tolist(), radiance, texture)

    def _struct(self):
        return _capi.hf_rect_light_t((C.c_float * 3)(*self.center), (C.c_float * 3)(*self.ex), (C.c_float * 3)(*self.ey),
                                     self.radiance)

    def geometry(self):
        """(area, unit normal) as the entries form them (``hf_rect_light_geometry``)"""
        area, nl = C.c_float(), (C.c_float * 3)()
        check(_capi.lib().hf_rect_light_geometry(C.byref(self._struct()), C.byref(area), C.byref(nl)))
        return area.value, tuple(nl)


def _rect_tex(dat):
    """the texture's C arguments: TW, TH, tex (no texture: 0, 0, NULL)"""
    return (dat.shape[1], dat.shape[0], dat.data_ptr()) if dat is not None else (0, 0, None)


class _RectLightingOp(torch.autograd.Function):
    """(image, visibility words) of hf_rect_lighting; backward = hf_rect_lighting_adjoint (gradients of sh_n, p, weight
    and the texels), jvp = hf_rect_lighting_tangent.  Both read the visibility word the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, sn, pp, dd, tt, vis, *rest):
        """what hf_rect_lighting_adjoint / _tangent start with (rest: the texels if the lamp has them, then the weight)"""
        spp, num_rays, seed, rid, lamp, albedo = ctx.misc
        dat = rest[0] if ctx.textured else None
        ww = rest[-1] if ctx.weighted else None
        return (sn.shape[1], spp, C.byref(_p3(pp)), C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed,
                _ptr(rid), C.byref(lamp), *_rect_tex(dat), albedo, vis.data_ptr())

    @staticmethod
    def forward(ctx, sh_n, p, weight, texture, shape, nrm, d, t, lamp, albedo, spp, num_rays, seed, ray_index):
        sn, pp, gn, dd, tt, ww, dat = map(_detached_f32, (sh_n, p, nrm, d, t, weight, texture))
        n = sn.shape[1]
        ctx.misc = (spp, num_rays, seed, ray_index, lamp, albedo)
        ctx.textured = dat is not None
        image = torch.empty(n // max(spp, 1), dtype=torch.float32, device=sn.device)
        vis = torch.empty(n, dtype=torch.int32, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_rect_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                               C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(ray_index),
                                               C.byref(lamp), *_rect_tex(dat), albedo, image.data_ptr(), vis.data_ptr(),
                                               _stream_of(sn.device)))
        saved = _with_weight(ctx, (sn, pp, dd, tt, vis) + ((dat,) if ctx.textured else ()), ww)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.mark_non_differentiable(vis)
        return image, vis

    @staticmethod
    def jvp(ctx, dsh_n, dp, dweight, dtexture, *_):
        saved = ctx.saved_tensors
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dq, df = _detached_f32(dp), _texel_tangent(dtexture if ctx.textured else None)  # (held until the call has been enqueued)
        dimage = torch.empty(sn.shape[1] // max(ctx.misc[0], 1), dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_rect_lighting_tangent(*_RectLightingOp._prefix(ctx, *saved), _ref(_row_ptrs(dn)),
                                                       _ref(_row_ptrs(dq)), _ptr(dw), _ptr(df), dimage.data_ptr(),
                                                       _stream_of(sn.device)))
        return dimage, None

    @staticmethod
    def backward(ctx, grad_image, _grad_vis):
        saved = ctx.saved_tensors
        sn = saved[0]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gp = torch.empty_like(sn)
        gd = _texel_grad(ctx, 3, saved[5]) if ctx.textured else None
        if sn.shape[1]:
            check(_capi.lib().hf_rect_lighting_adjoint(*_RectLightingOp._prefix(ctx, *saved), gi.data_ptr(), C.byref(_p3(gn)),
                                                       C.byref(_p3(gp)), _ptr(gw), _ptr(gd), _stream_of(sn.device)))
        return (gn, gp, gw, gd) + (None,) * 10


def rect_lighting(shape, si, ray, light, albedo=1.0, spp=1, num_rays=8, seed=0, weight=None, ray_index=None,
                  return_visibility=False):
    """Diffuse lighting under a rectangle lamp (``RectLight``; the reference's ``area`` emitter on a ``rectangle``) +
    box-filter film, soft shadows traced inside the lighting kernel (``hf_rect_lighting``): every sample draws
    ``num_rays`` (1..32) points of the lamp, uniform in area, from the TEA stream of ``sky_lighting`` (``seed``,
    ``ray_index``), traces ``si.spawn_ray_to(point)`` for those in front of both the sample and the lamp and averages
    ``albedo/pi * radiance * c_s * c_l * A / r^2`` over the unoccluded ones.  Returns the [n // spp] image; with
    ``return_visibility`` also the [n] int32 visibility words (bit k: point k was traced and is seen).  Differentiable
    with respect to ``si.sh_frame.n``, ``si.p``, ``weight`` ([n], optional) and the lamp's texture, in reverse and forward
    mode; the visibility, the masks, the draws and the lamp's pose and radiance are held.  Several lamps: one call each."""
    shape._check_ray(ray)
    image, vis = _RectLightingOp.apply(si.sh_frame.n, si.p, weight, light.texture, shape, si.n, ray.d, si.t, light._struct(),
                                       float(albedo), int(spp), int(num_rays), int(seed), _check_ray_index(ray_index, ray))
    return (image, vis) if return_visibility else image


def rect_rays(si, ray, light, k, seed=0, ray_index=None):
    """Shadow ray ``k`` of every sample of ``rect_lighting`` as a Ray3f (``hf_rect_rays``): what the fused kernel traces
    for that point of the lamp, bit for bit, ``maxt`` just short of the lamp.  Lanes it does not trace (no hit, seen from
    behind, the point behind the sample or the sample behind the lamp) get ``maxt = -1``, a miss."""
    rid = _check_ray_index(ray_index, ray)
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    if n:
        check(_capi.lib().hf_rect_rays(n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                       tt.data_ptr(), int(k), int(seed), _ptr(rid), C.byref(light._struct()),
                                       C.byref(_p3(r.o)), C.byref(_p3(r.d)), r.maxt.data_ptr(), _stream_of(pp.device)))
    return r


class _BounceLightingOp(torch.autograd.Function):
    """(image, hit_prim, lit_bits) of hf_bounce_lighting; backward = hf_bounce_lighting_adjoint (gradients of sh_n, weight
    and the heights), jvp = hf_bounce_lighting_tangent.  Both read the record the forward saved and trace nothing."""

    @staticmethod
    def _prefix(ctx, shape, sn, dd, tt, prim, lit, ww=None):
        """what hf_bounce_lighting_adjoint / _tangent start with"""
        spp, num_rays, seed, rid, L, K, albedo = ctx.misc
        n = sn.shape[1]
        return (shape._h, n, spp, C.byref(_p3(sn)), C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(rid),
                K, L, albedo, prim.data_ptr(), lit.data_ptr(), n)

    @staticmethod
    def forward(ctx, sh_n, weight, heights, shape, p, nrm, d, t, lights, albedo, spp, num_rays, seed, ray_index):
        sn, pp, gn, dd, tt, ww = map(_detached_f32, (sh_n, p, nrm, d, t, weight))
        n, (L, K) = sn.shape[1], _dir_lights(lights)
        ctx.misc = (spp, num_rays, seed, ray_index, L, K, albedo)
        image = torch.empty((K, n // max(spp, 1)), dtype=torch.float32, device=sn.device)
        prim = torch.empty((num_rays, n), dtype=torch.int32, device=sn.device)
        lit = torch.empty((num_rays, n), dtype=torch.uint8, device=sn.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_bounce_lighting(shape._h, n, spp, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)),
                                                 C.byref(_p3(dd)), tt.data_ptr(), _ptr(ww), num_rays, seed, _ptr(ray_index),
                                                 K, L, albedo, image.data_ptr(), prim.data_ptr(), lit.data_ptr(), n,
                                                 _stream_of(sn.device)))
        _op_save(ctx, shape, _with_weight(ctx, (sn, dd, tt, prim, lit), ww))
        ctx.mark_non_differentiable(prim, lit)
        return image, prim, lit

    @staticmethod
    def jvp(ctx, dsh_n, dweight, dheights, *_):
        shape, saved = _op_saved(ctx, "jvp")
        sn = saved[0]
        dn, dw = _weighted_tangents(ctx, dsh_n, dweight)
        dh = shape._dheights(dheights)
        dimage = torch.empty((ctx.misc[5], sn.shape[1] // ctx.misc[0]), dtype=torch.float32, device=sn.device)
        if sn.shape[1]:
            check(_capi.lib().hf_bounce_lighting_tangent(*_BounceLightingOp._prefix(ctx, shape, *saved), _ref(_row_ptrs(dn)),
                                                         _ptr(dw), _ptr(dh), dimage.data_ptr(), _stream_of(sn.device)))
        return dimage, None, None

    @staticmethod
    def backward(ctx, grad_image, _grad_prim, _grad_lit):
        shape, saved = _op_saved(ctx, "backward")
        sn = saved[0]
        gi, gn, gw = _weighted_grads(ctx, sn, grad_image)
        gh = shape._zero_heights() if ctx.needs_input_grad[2] else None
        if sn.shape[1]:
            check(_capi.lib().hf_bounce_lighting_adjoint(*_BounceLightingOp._prefix(ctx, shape, *saved), gi.data_ptr(),
                                                         C.byref(_p3(gn)), _ptr(gw), _ptr(gh), _stream_of(sn.device)))
        return (gn, gw, gh) + (None,) * 11


def _check_static_to_world(shape, what):
    """rows that do not differentiate to_world refuse a transform that asks for a derivative"""
    if shape._to_world_live() is not None:
        raise _capi.HfError(_capi.HF_EINVAL, f"{what}: to_world is not differentiated by this row (it requires "
                                             "grad or carries a tangent); detach it")


def bounce_lighting(shape, si, ray, lights, albedo=1.0, spp=1, num_rays=4, seed=0, weight=None, ray_index=None,
                    return_records=False):
    """One bounce of diffuse interreflection under directional lights + box-filter film, both rays of every path
    traced inside the lighting kernel (``hf_bounce_lighting``): every sample draws ``num_rays`` (1..32) cosine-weighted
    directions about ``si.sh_frame.n`` from the TEA stream of ``sky_lighting`` (``seed``, ``ray_index``; give the rows
    different seeds), traces ``si.spawn_ray(direction)`` to its closest hit and shades that hit, with its face normal
    and shadow rays of its own, under ``lights`` ([K, 4]: unit direction towards the light, irradiance).  Returns the
    [K, n // spp] image, whose rows add onto ``direct_lighting``'s; with ``return_records`` also ``hit_prim``
    ([num_rays, n] int32, -1 = no hit) and ``lit_bits`` ([num_rays, n] uint8, bit l: light l reaches the hit).
    Differentiable with respect to ``si.sh_frame.n``, ``weight`` ([n], optional) and ``shape.heightfield`` (through the
    normals of the hit triangles); visibility is piecewise constant and ``to_world`` is not differentiated."""
    shape._check_ray(ray)
    _check_static_to_world(shape, "bounce_lighting")
    lights = torch.as_tensor(lights, dtype=torch.float32).reshape(-1, 4)
    image, prim, lit = _BounceLightingOp.apply(si.sh_frame.n, weight, shape.heightfield, shape, si.p, si.n, ray.d, si.t,
                                               lights, float(albedo), int(spp), int(num_rays), int(seed),
                                               _check_ray_index(ray_index, ray))
    return (image, prim, lit) if return_records else image


def bounce_rays(shape, si, ray, k, seed=0, ray_index=None, to_light=None):
    """Ray ``k`` of every sample of ``bounce_lighting`` as a Ray3f (``hf_bounce_rays``), bit for bit what the fused
    kernel traces: the bounce ray, or with ``to_light`` (3 floats) the shadow ray from that bounce ray's hit towards
    the light.  Lanes the fused kernel does not trace get ``maxt = -1``, a miss."""
    rid = _check_ray_index(ray_index, ray)
    sn, pp, gn, dd, tt = map(_detached_f32, (si.sh_frame.n, si.p, si.n, ray.d, si.t))
    n, r = sn.shape[1], _empty_rays(pp)
    tl = (C.c_float * 3)(*[float(x) for x in to_light]) if to_light is not None else None
    if n:
        check(_capi.lib().hf_bounce_rays(shape._h, n, C.byref(_p3(pp)), C.byref(_p3(gn)), C.byref(_p3(sn)), C.byref(_p3(dd)),
                                         tt.data_ptr(), int(k), int(seed), _ptr(rid), _ref(tl), C.byref(_p3(r.o)),
                                         C.byref(_p3(r.d)), r.maxt.data_ptr(), _stream_of(pp.device)))
    return r


def _film_splat(values, ps, weight, K, n, width, height, stddev):
    """hf_film_splat of the [K, n] float32 values at ps into a zeroed [K, height * width] image and into weight"""
    image = torch.zeros((K, height * width), dtype=torch.float32, device=ps.device)
    px, py = _row_addrs(ps)
    check(_capi.lib().hf_film_splat(n, K, _row_ptrs(values), px, py, width, height, stddev, image.data_ptr(),
                                    weight.data_ptr(), _stream_of(ps.device)))
    return image


def _film_normalise(image, weight):
    """accumulated value / accumulated weight where the weight is positive, else 0"""
    covered = weight > 0
    return torch.where(covered[None], image / torch.where(covered, weight, torch.ones_like(weight))[None],
                       torch.zeros_like(image))


class _FilmGaussianOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, pos, width, height, stddev):
        K, n = values.shape
        v = values.detach().to(dtype=torch.float32).contiguous()
        ps = pos.detach().to(dtype=torch.float32).contiguous()
        weight = torch.zeros(height * width, dtype=torch.float32, device=v.device)
        ctx.misc = (K, n, width, height, stddev)
        image = _film_splat(v, ps, weight, *ctx.misc)
        ctx.save_for_backward(ps, weight)
        ctx.save_for_forward(ps, weight)
        return _film_normalise(image, weight)

    @staticmethod
    def jvp(ctx, dvalues, *_):
        # the film is linear in the values: its tangent is the splat of the tangent values over the primal weights
        ps, weight = ctx.saved_tensors
        image = _film_splat(dvalues.to(dtype=torch.float32).contiguous(), ps, torch.zeros_like(weight), *ctx.misc)
        return _film_normalise(image, weight)

    @staticmethod
    def backward(ctx, grad_film):
        ps, weight = ctx.saved_tensors
        K, n, width, height, stddev = ctx.misc
        ga = _film_normalise(grad_film.to(torch.float32), weight).contiguous()
        gv = torch.empty((K, n), dtype=torch.float32, device=ps.device)
        px, py = _row_addrs(ps)
        check(_capi.lib().hf_film_splat_adjoint(n, K, px, py, width, height, stddev, ga.data_ptr(), _row_ptrs(gv),
                                                _stream_of(ps.device)))
        return gv, None, None, None, None


class _FilmMotionOp(torch.autograd.Function):
    """The two accumulated planes (image [K, H W], weight [H W]) of samples that move and carry a weight:
    hf_film_splat_weighted; backward = hf_film_splat_weighted_adjoint (gradients of values, pos and weight),
    jvp = hf_film_splat_weighted_tangent.  ``weight`` None: every sample weighs 1."""

    @staticmethod
    def forward(ctx, values, pos, weight, width, height, stddev):
        K, n = values.shape
        v = values.detach().to(dtype=torch.float32).contiguous()
        ps = pos.detach().to(dtype=torch.float32, device=v.device).contiguous()
        sw = None if weight is None else weight.detach().to(dtype=torch.float32, device=v.device).contiguous().reshape(n)
        assert ps.shape == (2, n), f"pos: expected [2, {n}], got {tuple(ps.shape)}"
        ctx.misc = (n, K, width, height, stddev)
        ctx.like = [(x.dtype, x.device) if isinstance(x, torch.Tensor) else None for x in (values, pos, weight)]
        image = torch.zeros((K, height * width), dtype=torch.float32, device=v.device)
        plane = torch.zeros(height * width, dtype=torch.float32, device=v.device)
        px, py = _row_addrs(ps)
        check(_capi.lib().hf_film_splat_weighted(n, K, _row_ptrs(v), _ptr(sw), px, py, width, height, stddev,
                                                 image.data_ptr(), plane.data_ptr(), _stream_of(v.device)))
        saved = (v, ps) if sw is None else (v, ps, sw)
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        return image, plane

    @staticmethod
    def jvp(ctx, dvalues, dpos, dweight, *_):
        v, ps, sw = (*ctx.saved_tensors, None)[:3]
        n, K, width, height, stddev = ctx.misc
        dv = _tangent(dvalues, (K, n), v.device, "dvalues")
        dps = _tangent(dpos, (2, n), v.device, "dpos")
        dsw = _tangent(dweight, (n,), v.device, "dweight")
        dimage = torch.zeros((K, height * width), dtype=torch.float32, device=v.device)
        dplane = torch.zeros(height * width, dtype=torch.float32, device=v.device)
        px, py = _row_addrs(ps)
        dpx, dpy = (None, None) if dps is None else _row_addrs(dps)
        check(_capi.lib().hf_film_splat_weighted_tangent(n, K, _row_ptrs(v), _ptr(sw), px, py, width, height, stddev,
                                                         _row_ptrs(dv), _ptr(dsw), dpx, dpy, dimage.data_ptr(),
                                                         dplane.data_ptr(), _stream_of(v.device)))
        return dimage, dplane

    @staticmethod
    def backward(ctx, grad_image, grad_plane):
        v, ps, sw = (*ctx.saved_tensors, None)[:3]
        n, K, width, height, stddev = ctx.misc
        need_v, need_p, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and sw is not None
        if not (need_v or need_p or need_w):
            return None, None, None, None, None, None
        gi = grad_image.to(dtype=torch.float32).contiguous()
        gw = grad_plane.to(dtype=torch.float32).contiguous()
        gv = torch.empty((K, n), dtype=torch.float32, device=v.device) if need_v else None
        gp = torch.empty((2, n), dtype=torch.float32, device=v.device) if need_p else None
        gsw = torch.empty(n, dtype=torch.float32, device=v.device) if need_w else None
        px, py = _row_addrs(ps)
        gpx, gpy = (None, None) if gp is None else _row_addrs(gp)
        check(_capi.lib().hf_film_splat_weighted_adjoint(n, K, _row_ptrs(v), _ptr(sw), px, py, width, height, stddev,
                                                         gi.data_ptr(), gw.data_ptr(), _row_ptrs(gv), _ptr(gsw), gpx, gpy,
                                                         _stream_of(v.device)))
        back = lambda g, like: None if g is None else g.to(dtype=like[0], device=like[1])
        return back(gv, ctx.like[0]), back(gp, ctx.like[1]), back(gsw, ctx.like[2]), None, None, None


def film_gaussian(values, pos, width, height, stddev=0.5, weight=None):
    """Film with the reference's default reconstruction filter (Gaussian, stddev 0.5 pixel; ``hf_film_splat``;
    src/rfilters/gaussian.cpp, src/render/imageblock.cpp:258-330): ``values`` [K, n] per-sample values (e.g.
    ``direct_lighting(..., spp=1)``), ``pos`` [2, n] film positions in pixels (``workload.film_positions``).  Returns the
    normalised film [K, height * width] (accumulated value / accumulated weight); differentiable w.r.t. ``values``.

    ``weight`` [n]: what each sample adds to the weight plane per unit of filter weight (``ImageBlock::put(pos, value,
    weight)``; None = 1) -- the determinant of a reparameterised ray, with ``values`` = L det (common.py:868-970).  With a
    ``weight``, or a ``pos`` that requires a gradient or carries a forward-mode tangent, the film is differentiable
    w.r.t. ``values``, ``pos`` and ``weight`` (``hf_film_splat_weighted`` and its adjoint / tangent; the division by the
    weight plane is differentiated by torch, so the gradient reaches both planes as after ``film.develop()``)."""
    moving = isinstance(pos, torch.Tensor) and (pos.requires_grad or _has_tangent(pos))
    if weight is None and not moving:
        return _FilmGaussianOp.apply(values, pos, int(width), int(height), float(stddev))
    image, plane = _FilmMotionOp.apply(values, pos, weight, int(width), int(height), float(stddev))
    return _film_normalise(image, plane)


def _coordinate_system(n):
    """coordinate_system(), include/mitsuba/core/vector.h:116-136, on [3, k] tensors (differentiable)"""
    sign = torch.where(n[2] >= 0, torch.ones_like(n[2]), -torch.ones_like(n[2]))
    a = -1.0 / (sign + n[2])
    b = n[0] * n[1] * a
    s = torch.stack([torch.where(n[2] >= 0, n[0] * n[0] * a, -(n[0] * n[0] * a)) + 1.0,
                     torch.where(n[2] >= 0, b, -b),
                     torch.where(n[2] >= 0, -n[0], n[0])])
    t = torch.stack([b, n[1] * (n[1] * a) + sign, -n[1]])
    return s, t


REPARAM_FUSED = True   # tests switch this off to compare with the per-sample kernels
# The auxiliary hits of the first loop (36 B per ray and sample: pi + si.t, si.p, si.boundary_test) are kept for the
# second one when they fit; the reference re-traces (reparam.py:296-325), which is the fallback.
REPARAM_KEEP_BYTES = 64 << 30   # (288 GB of HBM per GPU: 16 samples of a 67 M-ray wavefront are 39 GB)


def _sample_structs(buf, si_hit=True):
    """hf_si_t / hf_pi_t over one sample buffer.  The backward's [9, n]: si.t, si.p[3], si.boundary_test | pi.t, u, v,
    prim_index; without ``si_hit`` only boundary_test of the SI record is written.  The tangent's [5, n]: the last
    five of those rows.  Returns (row addresses, si, pi)."""
    rows = _row_addrs(buf)
    si_s = hf_si_t()
    if si_hit and len(rows) == 9:
        _fill(si_s, [("t", 1), ("p", 3)], rows)
    si_s.boundary_test = rows[-5]
    return rows, si_s, _fill(hf_pi_t(), _PI_ROWS, rows[-4:])


def _reparam_inputs(ray_o, ray_d, active):
    """what the backward and the tangent of reparameterize_ray take: o, d as contiguous float32 [3, n] and active as
    uint8 [n] (None: every ray)"""
    o = ray_o.detach().to(torch.float32).contiguous()
    d = ray_d.detach().to(torch.float32).contiguous()
    act = None if active is None else torch.as_tensor(active, device=o.device).to(torch.uint8).reshape(-1).contiguous()
    if act is not None and act.numel() != o.shape[1]:
        raise ValueError("active: one flag per ray")
    return o, d, act


def _check_ray_index(ray_index, ray):
    """ray_index of reparameterize_ray / _tangent: contiguous, one int32/uint32 id per ray on the rays' device"""
    if ray_index is None:
        return None
    if ray_index.dtype not in (torch.int32, torch.uint32) or ray_index.numel() != ray.o.shape[1]:
        raise ValueError("ray_index must be an int32/uint32 tensor with one id per ray")
    if ray_index.device != ray.o.device:
        raise ValueError("ray_index must live on the rays' device")
    return ray_index.contiguous()


def _reparam_backward_fused(shape, o, d, gd, gdiv, act_p, rid_p, cfg, stream):
    """Heights only, hits kept: hf_reparam_trace_all traces every sample (pi and si.boundary_test; a ray is fetched
    once, batches whose cones miss are culled), then hf_reparam_backward does the weights, their sums and the adjoint
    of every auxiliary hit.  No per-sample intermediates (their zero fills: 1.3 GB, 0.2 ms for 67 M rays)."""
    L = _capi.lib()
    num_rays, kappa, exponent, antithetic, seed = cfg
    n = o.shape[1]
    o_p, d_p, gd_p = _p3(o), _p3(d), _p3(gd)
    store = torch.empty((num_rays, 9, n), dtype=torch.float32, device=o.device)   # sample k: 9 n floats further on
    grad_h = shape._zero_heights()
    rows, si_s, pi_s = _sample_structs(store[0], si_hit=False)
    check(L.hf_reparam_trace_all(shape._h, n, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, int(antithetic), seed,
                                 rid_p, C.byref(pi_s), C.byref(si_s), 9 * n, stream))
    check(L.hf_reparam_backward(shape._h, n, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, exponent,
                                int(antithetic), seed, rid_p, C.byref(pi_s), rows[4], 9 * n, C.byref(gd_p),
                                gdiv.data_ptr(), grad_h.data_ptr(), stream))
    return grad_h


def _reparam_backward_per_sample(shape, o, d, gd, gdiv, act, rid_p, cfg, keep, need_h, need_o, need_d, stream,
                                 grad_tw=None):
    """Per sample: hf_reparam_aux_rays + hf_ray_intersect + hf_reparam_weights for the weight sums, then
    hf_reparam_weights + hf_adjoint on the kept hits (re-traced without ``keep``); the ray gradients too.
    grad_tw (12 float32 device values): dL/d(to_world) is accumulated into it (hf_adjoint_transform)."""
    L = _capi.lib()
    num_rays, kappa, exponent, antithetic, seed = cfg
    dev = o.device
    n = o.shape[1]
    ray_grads = need_o or need_d
    act_p = _ptr(act)
    flags = int(RayFlags.All | RayFlags.FollowShape | RayFlags.BoundaryTest)
    aux_d = torch.empty((3, n), dtype=torch.float32, device=dev); aux_maxt = torch.empty(n, dtype=torch.float32, device=dev)
    Z = torch.zeros(n, dtype=torch.float32, device=dev); dZ = torch.zeros((3, n), dtype=torch.float32, device=dev)
    g_p = torch.empty((3, n), dtype=torch.float32, device=dev); g_t = torch.empty(n, dtype=torch.float32, device=dev)
    grad_h = shape._zero_heights() if need_h else None
    o_p, d_p, ad_p, dZ_p, gd_p, gp_p = _p3(o), _p3(d), _p3(aux_d), _p3(dZ), _p3(gd), _p3(g_p)
    r_s = shape._rays_struct(o, aux_d, aux_maxt)
    g_s = _fill(hf_si_grad_t(), [("t", 1), ("p", 3)], [g_t.data_ptr()] + _row_addrs(g_p))
    gvd_p = go_adj_p = gd_adj_p = grad_o = grad_d = None
    if ray_grads:   # per-sample ray gradients of the auxiliary hit + the gradient w.r.t. V_direct itself
        g_vd, go_adj, gd_adj = (torch.empty((3, n), dtype=torch.float32, device=dev) for _ in range(3))
        grad_o, grad_d = torch.zeros((3, n), dtype=torch.float32, device=dev), torch.zeros((3, n), dtype=torch.float32, device=dev)
        gvd_p, go_adj_p, gd_adj_p = C.byref(_p3(g_vd)), C.byref(_p3(go_adj)), C.byref(_p3(gd_adj))
    store = torch.empty((num_rays if keep else 1, 9, n), dtype=torch.float32, device=dev)

    def aux(k):
        check(L.hf_reparam_aux_rays(n, C.byref(o_p), C.byref(d_p), act_p, k, kappa, int(antithetic), seed, rid_p,
                                    C.byref(ad_p), aux_maxt.data_ptr(), stream))

    def trace(k, buf):
        aux(k)
        _, si_s, pi_s = _sample_structs(buf)
        check(L.hf_ray_intersect(shape._h, n, C.byref(r_s), flags, None, C.byref(pi_s), C.byref(si_s), stream))

    def weights(mode, k, buf):
        rows, sp_p = _row_addrs(buf), _p3(buf[1:4])
        check(L.hf_reparam_weights(mode, n, C.byref(o_p), C.byref(d_p), act_p, k, kappa, exponent, int(antithetic),
                                   seed, rid_p, rows[0], C.byref(sp_p), rows[4], Z.data_ptr(), C.byref(dZ_p), C.byref(gd_p),
                                   gdiv.data_ptr(), C.byref(gp_p), g_t.data_ptr(), gvd_p if mode == 1 else None, stream))

    for k in range(num_rays):   # weight normalisation (reparam.py:236-256)
        buf = store[k if keep else 0]
        trace(k, buf)
        weights(0, k, buf)
    for k in range(num_rays):
        buf = store[k if keep else 0]
        if keep:
            aux(k)                      # hf_adjoint needs the auxiliary ray again, not its trace
        else:
            trace(k, buf)
        weights(1, k, buf)
        _, si_s, pi_s = _sample_structs(buf)
        check(L.hf_adjoint_transform(shape._h, n, C.byref(r_s), C.byref(pi_s), flags, act_p, C.byref(g_s),
                                     _ptr(grad_h), go_adj_p, gd_adj_p, None, _ptr(grad_tw), stream))
        if ray_grads:
            hit = torch.isfinite(buf[0])
            if act is not None:
                hit = hit & (act != 0)
            # hit: V_direct = (p - o) / t  ->  dL/do = [t's dependence on o: hf_adjoint] - gVd / t  (= g_p);
            #      t's dependence on the auxiliary direction d_aux = Frame3f(d).to_world(omega) goes on to d
            # miss: V_direct = ray.d (reparam.py:93-95)  ->  dL/dd = gVd
            grad_o += torch.where(hit, go_adj - g_p, torch.zeros_like(g_p))
            if need_d:
                with torch.enable_grad():
                    dq = d.detach().clone().requires_grad_(True)
                    s_, t_ = _coordinate_system(dq)
                    sd, td = s_.detach(), t_.detach()
                    om = torch.stack([(sd * aux_d).sum(0), (td * aux_d).sum(0), (d * aux_d).sum(0)])  # omega_local
                    d_aux = s_ * om[0] + t_ * om[1] + dq * om[2]
                    (gd_through,) = torch.autograd.grad(d_aux, dq, torch.where(hit, gd_adj, torch.zeros_like(gd_adj)))
                grad_d += gd_through + torch.where(hit, torch.zeros_like(g_vd), g_vd)
    return grad_h, grad_o, grad_d


def _reparam_tangent(shape, o, d, act, ray_index, cfg, dh, do, dd, dtw, stream):
    """Forward mode (reparam.py:155-221): hf_reparam_trace_all keeps every auxiliary hit (pi + si.boundary_test,
    20 B per ray and sample), then hf_reparam_tangent.  When the records of all rays exceed REPARAM_KEEP_BYTES the rays
    go in chunks, each with its global ids as ray_id (or its slice of ray_index): the samples, and so the result, do
    not depend on the chunking.  Returns (V_theta [3, n], div [n])."""
    L = _capi.lib()
    num_rays, kappa, exponent, antithetic, seed = cfg
    dev = o.device
    n = o.shape[1]
    out_dir = torch.empty((3, n), dtype=torch.float32, device=dev)
    out_div = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out_dir, out_div
    chunk = max(1, min(n, REPARAM_KEEP_BYTES // (20 * num_rays)))
    store = torch.empty((num_rays, 5, chunk), dtype=torch.float32, device=dev)   # bt, t, u, v, prim per sample
    rows, si_s, pi_s = _sample_structs(store[0])
    for s in range(0, n, chunk):   # (column slices of the [3, n] tensors: no copies, see _row_addrs)
        m = min(chunk, n - s)
        sl = slice(s, s + m)
        if ray_index is not None:
            rid = ray_index[sl]
        elif m < n:
            rid = torch.arange(s, s + m, dtype=torch.int32, device=dev)
        else:
            rid = None
        o_p, d_p = _p3(o[:, sl]), _p3(d[:, sl])
        act_p, rid_p = _ptr(act[sl] if act is not None else None), _ptr(rid)
        check(L.hf_reparam_trace_all(shape._h, m, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, int(antithetic),
                                     seed, rid_p, C.byref(pi_s), C.byref(si_s), 5 * chunk, stream))
        check(L.hf_reparam_tangent(shape._h, m, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, exponent,
                                   int(antithetic), seed, rid_p, C.byref(pi_s), rows[0], 5 * chunk, _ptr(dh),
                                   _ref(_p3(do[:, sl]) if do is not None else None),
                                   _ref(_p3(dd[:, sl]) if dd is not None else None), _ptr(dtw),
                                   C.byref(_p3(out_dir[:, sl])), out_div[sl].data_ptr(), stream))
    return out_dir, out_div


def _reparam_backward_full(shape, o, d, gd, gdiv, act, ray_index, cfg, grad_h, need_o, need_d, grad_tw, stream):
    """Reverse mode with respect to any of the heights, ray.o, ray.d and to_world: hf_reparam_trace_all keeps every
    auxiliary hit (pi + si.boundary_test, 20 B per ray and sample, the layout of _reparam_tangent), then ONE
    hf_reparam_backward_full.  grad_h ([H, W]) and grad_tw (12 values) are the caller's accumulators (None: not
    wanted); returns (grad_o, grad_d) ([3, n], None when not wanted).  Chunked like _reparam_tangent when the records
    exceed REPARAM_KEEP_BYTES: the chunks' rays keep their global ids, grad_h / grad_tw accumulate across the chunks and
    grad_o / grad_d are written by column slice."""
    L = _capi.lib()
    num_rays, kappa, exponent, antithetic, seed = cfg
    dev = o.device
    n = o.shape[1]
    grad_o = torch.empty((3, n), dtype=torch.float32, device=dev) if need_o else None
    grad_d = torch.empty((3, n), dtype=torch.float32, device=dev) if need_d else None
    if n == 0:
        return grad_o, grad_d
    chunk = max(1, min(n, REPARAM_KEEP_BYTES // (20 * num_rays)))
    store = torch.empty((num_rays, 5, chunk), dtype=torch.float32, device=dev)   # bt, t, u, v, prim per sample
    rows, si_s, pi_s = _sample_structs(store[0])
    for s in range(0, n, chunk):   # (column slices of the [3, n] tensors: no copies, see _row_addrs)
        m = min(chunk, n - s)
        sl = slice(s, s + m)
        if ray_index is not None:
            rid = ray_index[sl]
        elif m < n:
            rid = torch.arange(s, s + m, dtype=torch.int32, device=dev)
        else:
            rid = None
        o_p, d_p, gd_p = _p3(o[:, sl]), _p3(d[:, sl]), _p3(gd[:, sl])
        act_p, rid_p = _ptr(act[sl] if act is not None else None), _ptr(rid)
        check(L.hf_reparam_trace_all(shape._h, m, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, int(antithetic),
                                     seed, rid_p, C.byref(pi_s), C.byref(si_s), 5 * chunk, stream))
        check(L.hf_reparam_backward_full(shape._h, m, C.byref(o_p), C.byref(d_p), act_p, num_rays, kappa, exponent,
                                         int(antithetic), seed, rid_p, C.byref(pi_s), rows[0], 5 * chunk, C.byref(gd_p),
                                         gdiv[sl].data_ptr(), _ptr(grad_h),
                                         _ref(_p3(grad_o[:, sl]) if need_o else None),
                                         _ref(_p3(grad_d[:, sl]) if need_d else None), _ptr(_grad12(grad_tw)), stream))
    return grad_o, grad_d


def _reparam_tangent_entry(shape, ray_o, ray_d, dh, do, dd, dtw, num_rays, kappa, exponent, antithetic, seed, active,
                           ray_index):
    o, d, act = _reparam_inputs(ray_o, ray_d, active)
    n, dev = o.shape[1], o.device
    dh = shape._dheights(dh, ValueError)
    do = _tangent(do, (3, n), dev, "d_o", ValueError)
    dd = _tangent(dd, (3, n), dev, "d_d", ValueError)
    dtw = _tw_tangent(dtw, dev, ValueError)
    if num_rays < 1 or num_rays > 32:
        raise ValueError("num_rays: 1..32 auxiliary rays per ray")
    cfg = (int(num_rays), float(kappa), float(exponent), bool(antithetic), int(seed))
    return _reparam_tangent(shape, o, d, act, ray_index, cfg, dh, do, dd, dtw, shape._stream())


class _ReparameterizeOp(torch.autograd.Function):
    """reparam.py:126-333 for a scene that is one heightfield: identity in primal mode; in backward mode the
    warped-area gradient of (direction, determinant) with respect to the heights AND the ray (reparam.py:296-325
    accumulates grad(ray.o), grad(ray.d) over the auxiliary samples)."""

    @staticmethod
    def forward(ctx, heightfield, ray_o, ray_d, shape, num_rays, kappa, exponent, antithetic, seed, active, ray_index=None,
                to_world=None):
        ctx.shape = shape
        ctx.tw_like = _tw_like(to_world)
        ctx.save_for_backward(ray_o, ray_d)
        ctx.save_for_forward(ray_o, ray_d)
        ctx.set_materialize_grads(False)   # jvp: an input without a tangent arrives as None, not as zeros
        ctx.cfg = (int(num_rays), float(kappa), float(exponent), bool(antithetic), int(seed), active, ray_index)
        n = ray_o.shape[1]
        # (an alias of ray.d, not a copy -- 0.8 GB and 0.27 ms for the bench wavefront: the values are ray.d's, reparam.py:139-155)
        return ray_d.detach(), torch.ones(n, dtype=torch.float32, device=ray_o.device)

    @staticmethod
    def jvp(ctx, dh, do, dd, _shape, _num_rays, _kappa, _exponent, _antithetic, _seed, _active, _ray_index, dtw=None):
        """reparam.py:155-221: the tangents (V_theta, div V_theta) of (direction, det), hf_reparam_tangent"""
        ray_o, ray_d = ctx.saved_tensors
        num_rays, kappa, exponent, antithetic, seed, active, ray_index = ctx.cfg
        return _reparam_tangent_entry(ctx.shape, ray_o, ray_d, dh, do, dd, dtw, num_rays, kappa, exponent, antithetic,
                                      seed, active, ray_index)

    @staticmethod
    def backward(ctx, grad_direction, grad_divergence):
        shape = ctx.shape
        ray_o, ray_d = ctx.saved_tensors
        num_rays, kappa, exponent, antithetic, seed, active, ray_index = ctx.cfg
        cfg = (num_rays, kappa, exponent, antithetic, seed)
        rid_p = _ptr(ray_index)
        need_h, need_o, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_tw = ctx.needs_input_grad[11]
        o, d, act = _reparam_inputs(ray_o, ray_d, active)
        n = o.shape[1]
        gd = _tangent(grad_direction, (3, n), o.device, "grad_direction", ValueError)
        gdiv = _tangent(grad_divergence, (n,), o.device, "grad_divergence", ValueError)
        if gd is None:
            gd = torch.zeros_like(d)
        if gdiv is None:
            gdiv = torch.zeros(n, dtype=torch.float32, device=d.device)
        stream = shape._stream()
        keep = 36 * n * num_rays <= REPARAM_KEEP_BYTES
        # (backward runs only when some input needs a gradient: without the ray's, that is the heights')
        # heights only: hf_reparam_backward; with the ray or to_world: hf_reparam_backward_full (chunked when the hits
        # do not fit).  The per-sample kernels are what REPARAM_FUSED = False selects
        grad_tw = torch.zeros(12, dtype=torch.float32, device=ray_o.device) if need_tw else None
        if REPARAM_FUSED and (need_o or need_d or need_tw) and num_rays <= 32:
            gh = shape._zero_heights() if need_h else None
            grad_o, grad_d = _reparam_backward_full(shape, o, d, gd, gdiv, act, ray_index, cfg, gh, need_o, need_d,
                                                    grad_tw, stream)
        elif REPARAM_FUSED and keep and num_rays <= 32:
            gh, grad_o, grad_d = _reparam_backward_fused(shape, o, d, gd, gdiv, _ptr(act), rid_p, cfg, stream), None, None
        else:
            gh, grad_o, grad_d = _reparam_backward_per_sample(shape, o, d, gd, gdiv, act, rid_p, cfg, keep,
                                                              need_h, need_o, need_d, stream, grad_tw)
        if gh is not None and gh.shape != shape.heightfield.shape:
            gh = gh.reshape(shape.heightfield.shape)
        return ((gh if need_h else None), (grad_o if need_o else None), (grad_d if need_d else None),
                None, None, None, None, None, None, None, None, _tw_grad(grad_tw, ctx.tw_like))


def reparameterize_ray(shape, ray, num_rays=4, kappa=1e5, exponent=3.0, antithetic=False, seed=0, active=None,
                       ray_index=None):
    """``mitsuba.ad.reparameterize_ray`` (reparam.py:336-420) for a scene made of this heightfield: returns
    ``(direction, det)`` = ``(ray.d, 1)`` -- the reparameterisation is the identity in primal mode, exactly as in
    the reference (reparam.py:139-155) -- whose gradients flow into ``shape.heightfield`` and into ``ray.o`` /
    ``ray.d`` (when those require grad) through ``num_rays`` auxiliary rays per ray (von Mises-Fisher around
    ``ray.d``, harmonic weights from ``si.boundary_test``, hits followed with ``RayFlags.FollowShape``).
    ``ray.d`` must be unit length.  PCG32 is replaced by sample_tea_32 keyed on (seed, pair, ray id) (include/hf.h);
    ``ray_index`` (int32/uint32 device tensor, one id per ray, e.g. the global pixel index) makes the samples of a
    ray independent of its position in the batch, so a partitioned render draws the same auxiliary rays as the
    unpartitioned one.  Without it the id is the position in the batch.  For a ``differentiable_to_world`` shape whose
    ``to_world`` needs a gradient, that gradient is accumulated too.  The backward is one trace of all auxiliary rays
    and one kernel: ``hf_reparam_backward`` when only the heights are differentiated, ``hf_reparam_backward_full``
    when ``ray.o``, ``ray.d`` or ``to_world`` is."""
    return _ReparameterizeOp.apply(shape.heightfield, ray.o, ray.d, shape, num_rays, kappa, exponent, antithetic, seed,
                                   active, _check_ray_index(ray_index, ray), shape._to_world_live())


def reparameterize_ray_tangent(shape, ray, dheights=None, d_o=None, d_d=None, d_to_world=None, num_rays=4, kappa=1e5,
                               exponent=3.0, antithetic=False, seed=0, active=None, ray_index=None):
    """Explicit forward mode of ``reparameterize_ray`` (reparam.py:155-221): ``(V_theta [3, n], div [n])``, the
    tangents of ``(direction, det)`` for tangents of the heights (``dheights`` [H, W]), of the ray (``d_o``, ``d_d``
    [3, n]) and of ``to_world`` (``d_to_world``: 3x4 / 4x4 / 12 values), any of them None (zero).  The same samples as
    ``reparameterize_ray`` for the same ``seed`` and ``ray_index``; ``hf_reparam_trace_all`` + ``hf_reparam_tangent``."""
    return _reparam_tangent_entry(shape, ray.o, ray.d, dheights, d_o, d_d, d_to_world, num_rays, kappa, exponent,
                                  antithetic, seed, active, _check_ray_index(ray_index, ray))


def _check_accumulator(x, numel, device, what):
    """a caller's gradient accumulator is handed to the kernel as a device pointer: float32, contiguous, `numel` values,
    on the rays' device"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != numel:
        raise ValueError(f"{what}: a contiguous float32 tensor of {numel} values")
    if x.device != device:
        raise ValueError(f"{what} lives on {x.device}, the rays on {device}")


def reparameterize_ray_adjoint(shape, ray, grad_direction, grad_divergence, num_rays=4, kappa=1e5, exponent=3.0,
                               antithetic=False, seed=0, active=None, ray_index=None, heights=True, o=False, d=False,
                               to_world=False, grad_heightfield=None, grad_to_world=None):
    """Explicit reverse mode of ``reparameterize_ray`` (reparam.py:224-333), the sibling of
    ``reparameterize_ray_tangent``: for upstream gradients ``grad_direction`` ([3, n]) and ``grad_divergence`` ([n]) of
    ``(direction, det)`` (None: zero) returns ``(grad_heights, grad_o, grad_d, grad_to_world)``, None for the outputs not
    asked for with ``heights`` / ``o`` / ``d`` / ``to_world``.  ``grad_heightfield`` ([H, W] float32) and
    ``grad_to_world`` (12 contiguous float32 device values, row-major 3x4) are accumulators of the caller's, as in
    ``Heightfield.adjoint``: the gradients are ADDED to them and they are returned; without them zeroed ones are made.
    ``grad_o`` / ``grad_d`` ([3, n]) are new tensors.  The same samples as ``reparameterize_ray`` for the same ``seed`` and
    ``ray_index``; ``hf_reparam_trace_all`` + ``hf_reparam_backward_full``."""
    ray_index = _check_ray_index(ray_index, ray)
    ro, rd, act = _reparam_inputs(ray.o, ray.d, active)
    n, dev = ro.shape[1], ro.device
    if num_rays < 1 or num_rays > 32:
        raise ValueError("num_rays: 1..32 auxiliary rays per ray")
    if not (heights or o or d or to_world):
        raise ValueError("reparameterize_ray_adjoint: no gradient asked for")
    gd = _tangent(grad_direction, (3, n), dev, "grad_direction", ValueError)
    gdiv = _tangent(grad_divergence, (n,), dev, "grad_divergence", ValueError)
    if gd is None:
        gd = torch.zeros_like(rd)
    if gdiv is None:
        gdiv = torch.zeros(n, dtype=torch.float32, device=dev)
    grad_h = grad_tw = None
    if heights:
        grad_h = shape._zero_heights() if grad_heightfield is None else grad_heightfield
        _check_accumulator(grad_h, shape.height * shape.width, dev, "grad_heightfield")
    if to_world:
        grad_tw = torch.zeros(12, dtype=torch.float32, device=dev) if grad_to_world is None else grad_to_world
        _check_accumulator(grad_tw, 12, dev, "grad_to_world")
    cfg = (int(num_rays), float(kappa), float(exponent), bool(antithetic), int(seed))
    grad_o, grad_d = _reparam_backward_full(shape, ro, rd, gd, gdiv, act, ray_index, cfg, grad_h, bool(o), bool(d), grad_tw,
                                            shape._stream())
    return grad_h, grad_o, grad_d, grad_tw


class _LargeStepsApplyOp(torch.autograd.Function):
    """u = (I + lambda L) v (hf_large_steps_apply).  The matrix is symmetric: backward and jvp are the apply."""

    @staticmethod
    def forward(ctx, ls, v):
        ctx.misc = ls
        return ls._apply(v)

    @staticmethod
    def jvp(ctx, _ls, dv):
        return ctx.misc._apply(dv)

    @staticmethod
    def backward(ctx, grad_u):
        return None, ctx.misc._apply(grad_u)


class _LargeStepsSolveOp(torch.autograd.Function):
    """v = (I + lambda L)^-1 u (hf_large_steps_solve); backward and jvp are the solve of the incoming gradient / tangent
    (SolveCholesky.forward / backward, largesteps.py:41-49), always from a cold start."""

    @staticmethod
    def forward(ctx, ls, u, guess, info):
        ctx.misc = ls
        return ls._solve(u, guess, info)

    @staticmethod
    def jvp(ctx, _ls, du, _guess, _info):
        return ctx.misc._solve(du, None, None)

    @staticmethod
    def backward(ctx, grad_v):
        return None, ctx.misc._solve(grad_v, None, None), None, None


class LargeSteps:
    """The reference's ``mitsuba.ad.largesteps.LargeSteps`` (src/python/python/ad/largesteps.py:55-161; Nicolet et al.
    2021) for a ``width`` x ``height`` height grid: optimise the latent ``u = (I + lambda_ L) v`` instead of the heights
    ``v``, with L the combinatorial Laplacian of the tessellation (include/hf.h).  ``to_differential`` is one stencil
    launch, ``from_differential`` a conjugate-gradient solve (at most ``max_iter`` iterations, to the relative residual
    ``tol``) in place of the reference's sparse Cholesky factorisation; both take and return [H, W] float32 device
    tensors, are differentiable in both modes, never synchronise (unless asked to check) and can be captured.  The object
    owns the solver's workspace: its calls belong on one stream at a time."""

    def __init__(self, width, height, lambda_=19.0, max_iter=256, tol=1e-6):
        if int(width) < 2 or int(height) < 2:
            raise ValueError("LargeSteps: the grid must have at least 2 x 2 vertices")
        if not (float(lambda_) >= 0.0 and math.isfinite(float(lambda_))):
            raise ValueError("LargeSteps: lambda_ must be finite and >= 0")
        if int(max_iter) < 1:
            raise ValueError("LargeSteps: max_iter must be at least 1")
        if not float(tol) >= 0.0:
            raise ValueError("LargeSteps: tol must be >= 0")
        self.width, self.height = int(width), int(height)
        self.lambda_, self.max_iter, self.tol = float(lambda_), int(max_iter), float(tol)
        self._workspace = None
        self._info = None

    def _field(self, x, what):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"LargeSteps: {what} must be a device tensor")
        if tuple(x.shape) != (self.height, self.width):
            raise ValueError(f"LargeSteps: {what} must be [{self.height}, {self.width}], got {tuple(x.shape)}")
        return x.detach().to(dtype=torch.float32).contiguous()

    def _apply(self, v):
        v = self._field(v, "v")
        u = torch.empty_like(v)
        check(_capi.lib().hf_large_steps_apply(self.width, self.height, self.lambda_, v.data_ptr(), u.data_ptr(),
                                               _stream_of(v.device)))
        return u

    def _solve(self, u, guess, info):
        u = self._field(u, "u")
        if self._workspace is None or self._workspace.device != u.device:
            n = _capi.lib().hf_large_steps_workspace_floats(self.width, self.height)
            self._workspace = torch.empty(n, dtype=torch.float32, device=u.device)
        v = torch.empty_like(u) if guess is None else self._field(guess, "guess").to(u.device).clone()
        check(_capi.lib().hf_large_steps_solve(self.width, self.height, self.lambda_, u.data_ptr(), v.data_ptr(),
                                               0 if guess is None else 1, self.max_iter, self.tol,
                                               self._workspace.data_ptr(), _ptr(info), _stream_of(u.device)))
        return v

    def to_differential(self, v):
        """the latent u = (I + lambda_ L) v of the heights v (largesteps.py:122-141)"""
        return _LargeStepsApplyOp.apply(self, v)

    def from_differential(self, u, guess=None, check=False):
        """the heights v = (I + lambda_ L)^-1 u of the latent u (largesteps.py:143-161).  ``guess``: a tensor the solve
        starts from (detached; the previous step's heights).  ``check``: synchronise and raise RuntimeError when the
        solve ended at ``max_iter`` above ``tol``."""
        info = torch.zeros(2, dtype=torch.float32, device=u.device) if isinstance(u, torch.Tensor) and u.is_cuda else None
        v = _LargeStepsSolveOp.apply(self, u, None if guess is None else guess.detach(), info)
        self._info = info
        if check:
            it, res = self.last_info()
            if not res <= self.tol:
                raise RuntimeError(f"LargeSteps.from_differential: relative residual {res:.3e} after {it} iterations "
                                   f"(tol {self.tol:.3e}, max_iter {self.max_iter})")
        return v

    def last_info(self):
        """(iterations, relative residual) of the last ``from_differential``; synchronises"""
        if self._info is None:
            raise RuntimeError("LargeSteps.last_info: no solve yet")
        it, res = self._info.tolist()
        return int(it), float(res)

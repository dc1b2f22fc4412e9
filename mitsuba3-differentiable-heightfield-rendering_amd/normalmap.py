"""The normal map on top of the C ABI (include/hf.h): ``NormalMap`` is the reference's ``normalmap``
(src/bsdfs/normalmap.cpp) as a map of the shading normal -- an RGB texture, finer than the height grid and independent of
it, that replaces ``si.sh_frame.n``.  ``NormalMap.normal`` is the fused launch (``hf_normalmap_eval``, its adjoint and its
tangent); ``NormalMap.perturb`` hands back an interaction that goes straight into any lighting row.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import copy

import torch

from . import _capi
from ._capi import check
from .shape import (_WRAPS, _caustic_active, _detached_f32, _ptr, _ref, _row_ptrs, _stream_of, _texel_grad, _texel_tangent,
                    Frame3f, RayFlags)


def _map_in(uu, sn, du, act, dat, wrap):
    """what the three hf_normalmap_* entries start with: n, uv, sh_n, dp_du, active, TW, TH, tex, wrap"""
    return (uu.shape[1], _ref(_row_ptrs(uu)), _ref(_row_ptrs(sn)), _ref(_row_ptrs(du)), _ptr(act), dat.shape[2], dat.shape[1],
            dat.data_ptr(), wrap)


def _row_tangent(x):
    """jvp: the tangent of a [k, n] row block as contiguous float32 (None: zero)"""
    return x.to(dtype=torch.float32).contiguous() if x is not None else None


def _with_normal(si, N):
    """a shallow copy of ``si`` with the shading normal ``N`` (``NormalMap.perturb``, ``BumpMap.perturb``): ``sh_frame`` is
    ``Frame3f(s, t, N)``, ``s`` and ``t`` the detached Gram-Schmidt of ``dp_du`` against ``N`` (the input's own ``s`` where that
    degenerates), and ``wi``, where present, re-expressed in the new frame"""
    out = copy.copy(si)
    with torch.no_grad():
        Nd, u = N.detach(), si.dp_du.detach()
        a = u - Nd * (Nd * u).sum(0, keepdim=True)
        len_a = torch.linalg.vector_norm(a, dim=0, keepdim=True)
        ok = (len_a > 0) & torch.isfinite(len_a)
        s = a / torch.where(ok, len_a, torch.ones_like(len_a))
        if si.sh_frame.s is not None:
            s = torch.where(ok, s, si.sh_frame.s.detach())
        t = torch.linalg.cross(Nd, s, dim=0)
    out.sh_frame = Frame3f(s, t, N)
    if si.wi is not None and si.sh_frame.s is not None:
        world = si.sh_frame.s * si.wi[0:1] + si.sh_frame.t * si.wi[1:2] + si.sh_frame.n * si.wi[2:3]
        out.wi = out.sh_frame.to_local(world.detach())
    return out


class _NormalMapOp(torch.autograd.Function):
    """(N [3, n], mask bytes) of hf_normalmap_eval; backward = hf_normalmap_eval_adjoint (gradients of the texels, uv, sh_n
    and dp_du), jvp = hf_normalmap_eval_tangent.  Both hold the cell and the perturbed / pass-through decision."""

    @staticmethod
    def forward(ctx, data, uv, sh_n, dp_du, active, wrap):
        dat, uu, sn, du = map(_detached_f32, (data, uv, sh_n, dp_du))
        n = uu.shape[1]
        ctx.misc = (active, wrap)
        out = torch.empty((3, n), dtype=torch.float32, device=uu.device)
        mask = torch.empty(n, dtype=torch.uint8, device=uu.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_normalmap_eval(*_map_in(uu, sn, du, active, dat, wrap), _ref(_row_ptrs(out)), mask.data_ptr(),
                                                _stream_of(uu.device)))
        ctx.save_for_backward(dat, uu, sn, du)
        ctx.save_for_forward(dat, uu, sn, du)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def jvp(ctx, ddata, duv, dsh_n, ddp_du, *_):
        act, wrap = ctx.misc
        dat, uu, sn, du = ctx.saved_tensors
        # (held until the call has been enqueued)
        dd, tu, tn, tp = _texel_tangent(ddata), _row_tangent(duv), _row_tangent(dsh_n), _row_tangent(ddp_du)
        out = torch.empty_like(sn)
        if uu.shape[1]:
            check(_capi.lib().hf_normalmap_eval_tangent(*_map_in(uu, sn, du, act, dat, wrap), _ptr(dd), _ref(_row_ptrs(tu)),
                                                        _ref(_row_ptrs(tn)), _ref(_row_ptrs(tp)), _ref(_row_ptrs(out)),
                                                        _stream_of(uu.device)))
        return out, None

    @staticmethod
    def backward(ctx, grad_out, _grad_mask):
        act, wrap = ctx.misc
        dat, uu, sn, du = ctx.saved_tensors
        gd = _texel_grad(ctx, 0, dat)
        gu, gn, gp = (torch.empty_like(x) if ctx.needs_input_grad[k] else None for k, x in ((1, uu), (2, sn), (3, du)))
        if uu.shape[1] and any(g is not None for g in (gd, gu, gn, gp)):
            go = _detached_f32(grad_out)
            check(_capi.lib().hf_normalmap_eval_adjoint(*_map_in(uu, sn, du, act, dat, wrap), _ref(_row_ptrs(go)), _ptr(gd),
                                                        _ref(_row_ptrs(gu)), _ref(_row_ptrs(gn)), _ref(_row_ptrs(gp)),
                                                        _stream_of(uu.device)))
        return gd, gu, gn, gp, None, None


class NormalMap:
    """The reference's ``normalmap`` (src/bsdfs/normalmap.cpp:188-196) over its ``bitmap`` texture with the bilinear filter:
    texel ``data[:, iy, ix]`` is ``0.5 * (m + 1)`` for the unit normal ``m`` in the tangent space (s, t, n) of the surface,
    with its centre at ``uv = ((ix + 0.5) / TW, (iy + 0.5) / TH)``.  ``data``: [3, TH, TW] float32 device tensor, PLANAR,
    kept by reference -- it may require grad or be a dual.  ``wrap``: ``"repeat"`` (the reference bitmap's default) or
    ``"clamp"``.  The reference's ``bumpmap`` is ``BumpMap`` (bumpmap.py).  Out of scope: nearest filtering, the
    mirror wrap, a gradient for the frame's s and t."""

    def __init__(self, data, wrap="repeat"):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32:
            data = torch.as_tensor(data, dtype=torch.float32)
        if data.dim() != 3 or data.shape[0] != 3 or data.shape[1] < 1 or data.shape[2] < 1:
            raise ValueError("NormalMap: data must be [3, TH >= 1, TW >= 1] (got %r)" % (tuple(data.shape),))
        if wrap not in _WRAPS:
            raise ValueError("NormalMap: wrap must be 'clamp' or 'repeat' (got %r)" % (wrap,))
        self.data = data
        self.wrap = wrap

    @property
    def resolution(self):
        """(TW, TH)"""
        return self.data.shape[2], self.data.shape[1]

    @classmethod
    def flat(cls, TW, TH, device="cuda", wrap="repeat"):
        """the map (0.5, 0.5, 1): every normal is the surface's own"""
        data = torch.empty((3, int(TH), int(TW)), dtype=torch.float32, device=device)
        data[0:2] = 0.5
        data[2] = 1.0
        return cls(data, wrap)

    @staticmethod
    def encode(normals):
        """[3, ...] unit normals in tangent space -> texels 0.5 (m + 1)"""
        return 0.5 * (normals + 1.0)

    def decode(self):
        """the texels as [3, TH, TW] unit normals (2 c - 1) / |2 c - 1|; a texel (0.5, 0.5, 0.5) decodes to zero"""
        m = 2.0 * self.data - 1.0
        return m / torch.linalg.vector_norm(m, dim=0, keepdim=True).clamp_min(1e-6)

    @staticmethod
    def _records(si):
        if si.uv is None or si.dp_du is None or si.sh_frame is None or si.sh_frame.n is None:
            raise ValueError("NormalMap: the interaction has no uv / dp_du / shading normal (compute it with RayFlags.All)")
        flags = getattr(si, "ray_flags", None)
        if flags is not None and not (int(flags) & int(RayFlags.dPdUV) and int(flags) & int(RayFlags.UV)):
            raise ValueError("NormalMap: the interaction was computed without RayFlags.UV | RayFlags.dPdUV (flags %#x)" % int(flags))
        return si.uv, si.sh_frame.n, si.dp_du

    def normal(self, si, active=True, return_mask=False):
        """the perturbed shading normal [3, n] of the interaction ``si`` (``hf_normalmap_eval``): one launch, and one each
        for ``backward`` and ``jvp``.  Differentiable in ``data``, ``si.uv`` (with the cell held), ``si.sh_frame.n`` and
        ``si.dp_du``, so gradients flow on into the heights and ``to_world``.  A lane that is inactive, not finite, without
        a lookup or with a degenerate texel or frame passes ``si.sh_frame.n`` through bit for bit.  With ``return_mask``
        also the [n] uint8 row: 1 where perturbed.  ``si`` must have been computed with ``RayFlags.dPdUV`` (ValueError)."""
        uv, sh_n, dp_du = self._records(si)
        n = uv.shape[1]
        out, mask = _NormalMapOp.apply(self.data, uv, sh_n, dp_du, _caustic_active(active, n, uv.device), _WRAPS[self.wrap])
        return (out, mask) if return_mask else out

    def perturb(self, si, active=True):
        """a shallow copy of ``si`` whose ``sh_frame`` is ``Frame3f(s, t, N)`` with ``N = self.normal(si, active)``; ``s``, ``t``
        are the detached Gram-Schmidt of ``dp_du`` against ``N`` (the input's own where that degenerates) and ``wi``, where
        present, is re-expressed in the new frame.  Host-side convenience in a few torch ops, not the hot path; only ``N``
        carries a gradient."""
        return _with_normal(si, self.normal(si, active))

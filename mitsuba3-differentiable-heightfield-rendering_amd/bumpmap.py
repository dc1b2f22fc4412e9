"""The bump map on top of the C ABI (include/hf.h): ``BumpMap`` is the reference's ``bumpmap``
(src/bsdfs/bumpmap.cpp) as a map of the shading normal -- a scalar relief, finer than the height grid and laid over it,
whose slopes tilt ``si.sh_frame.n``.  ``BumpMap.normal`` is the fused launch (``hf_bumpmap_eval``, its adjoint and its
tangent); ``BumpMap.perturb`` hands back an interaction that goes straight into any lighting row.

torch is used for device memory, streams and autograd plumbing only; the arithmetic happens in the HIP kernels."""
import math
import numbers

import torch

from . import _capi
from ._capi import check
from .normalmap import _row_tangent, _with_normal
from .shape import (_WRAPS, _caustic_active, _detached_f32, _ptr, _ref, _row_ptrs, _stream_of, _texel_grad, _texel_tangent,
                    RayFlags)


def _map_in(uu, sn, ng, du, dv, act, dat, wrap, scale):
    """what the three hf_bumpmap_* entries start with: n, uv, sh_n, n_geo, dp_du, dp_dv, active, TW, TH, tex, wrap, scale"""
    return (uu.shape[1], _ref(_row_ptrs(uu)), _ref(_row_ptrs(sn)), _ref(_row_ptrs(ng)), _ref(_row_ptrs(du)), _ref(_row_ptrs(dv)),
            _ptr(act), dat.shape[1], dat.shape[0], dat.data_ptr(), wrap, scale)


class _BumpMapOp(torch.autograd.Function):
    """(N [3, n], mask bytes) of hf_bumpmap_eval; backward = hf_bumpmap_eval_adjoint (gradients of the texels, uv, sh_n, dp_du
    and dp_dv), jvp = hf_bumpmap_eval_tangent.  Both hold the cell, the perturbed / pass-through decision, sigma and n_geo."""

    @staticmethod
    def forward(ctx, data, uv, sh_n, dp_du, dp_dv, n_geo, active, wrap, scale):
        dat, uu, sn, du, dv, ng = map(_detached_f32, (data, uv, sh_n, dp_du, dp_dv, n_geo))
        n = uu.shape[1]
        ctx.misc = (active, wrap, scale)
        out = torch.empty((3, n), dtype=torch.float32, device=uu.device)
        mask = torch.empty(n, dtype=torch.uint8, device=uu.device)
        if n:  # (an empty wavefront has no rows to point to)
            check(_capi.lib().hf_bumpmap_eval(*_map_in(uu, sn, ng, du, dv, active, dat, wrap, scale), _ref(_row_ptrs(out)),
                                              mask.data_ptr(), _stream_of(uu.device)))
        ctx.save_for_backward(dat, uu, sn, du, dv, ng)
        ctx.save_for_forward(dat, uu, sn, du, dv, ng)
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def jvp(ctx, ddata, duv, dsh_n, ddp_du, ddp_dv, *_):
        act, wrap, scale = ctx.misc
        dat, uu, sn, du, dv, ng = ctx.saved_tensors
        # (held until the call has been enqueued)
        dd, tu, tn, tp, tq = _texel_tangent(ddata), _row_tangent(duv), _row_tangent(dsh_n), _row_tangent(ddp_du), _row_tangent(ddp_dv)
        out = torch.empty_like(sn)
        if uu.shape[1]:
            check(_capi.lib().hf_bumpmap_eval_tangent(*_map_in(uu, sn, ng, du, dv, act, dat, wrap, scale), _ptr(dd),
                                                      _ref(_row_ptrs(tu)), _ref(_row_ptrs(tn)), _ref(_row_ptrs(tp)),
                                                      _ref(_row_ptrs(tq)), _ref(_row_ptrs(out)), _stream_of(uu.device)))
        return out, None

    @staticmethod
    def backward(ctx, grad_out, _grad_mask):
        act, wrap, scale = ctx.misc
        dat, uu, sn, du, dv, ng = ctx.saved_tensors
        gd = _texel_grad(ctx, 0, dat)
        gu, gn, gp, gq = (torch.empty_like(x) if ctx.needs_input_grad[k] else None for k, x in ((1, uu), (2, sn), (3, du), (4, dv)))
        if uu.shape[1] and any(g is not None for g in (gd, gu, gn, gp, gq)):
            go = _detached_f32(grad_out)
            check(_capi.lib().hf_bumpmap_eval_adjoint(*_map_in(uu, sn, ng, du, dv, act, dat, wrap, scale), _ref(_row_ptrs(go)),
                                                      _ptr(gd), _ref(_row_ptrs(gu)), _ref(_row_ptrs(gn)), _ref(_row_ptrs(gp)),
                                                      _ref(_row_ptrs(gq)), _stream_of(uu.device)))
        return gd, gu, gn, gp, gq, None, None, None, None


class BumpMap:
    """The reference's ``bumpmap`` (src/bsdfs/bumpmap.cpp:199-222) over its ``bitmap`` texture with the bilinear filter: texel
    ``data[iy, ix]`` is the relief's height at ``uv = ((ix + 0.5) / TW, (iy + 0.5) / TH)``, and the shading normal becomes the
    normal of the surface displaced along it by that relief -- ``scale`` times the relief's gradient with respect to ``uv``
    tilts ``dp_du`` and ``dp_dv``.  ``data``: [TH, TW] float32 device tensor, kept by reference -- it may require grad or be a
    dual.  ``scale``: a finite float, not differentiated (it is redundant with the texels).  ``wrap``: ``"repeat"`` (the
    reference bitmap's default) or ``"clamp"``.  Out of scope: nearest filtering, an RGB texture, a uv transform, the mirror
    wrap, a gradient for ``scale``, ``si.n`` and the frame's s and t."""

    def __init__(self, data, scale=1.0, wrap="repeat"):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.float32:
            data = torch.as_tensor(data, dtype=torch.float32)
        if data.dim() != 2 or data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError("BumpMap: data must be [TH >= 1, TW >= 1] (got %r)" % (tuple(data.shape),))
        if wrap not in _WRAPS:
            raise ValueError("BumpMap: wrap must be 'clamp' or 'repeat' (got %r)" % (wrap,))
        if isinstance(scale, bool) or not isinstance(scale, numbers.Real) or not math.isfinite(scale):
            raise ValueError("BumpMap: scale must be a finite number (got %r)" % (scale,))
        self.data = data
        self.scale = float(scale)
        self.wrap = wrap

    @property
    def resolution(self):
        """(TW, TH)"""
        return self.data.shape[1], self.data.shape[0]

    @classmethod
    def flat(cls, TW, TH, device="cuda", scale=1.0, wrap="repeat"):
        """the relief 0: every normal is the surface's own, to rounding"""
        return cls(torch.zeros((int(TH), int(TW)), dtype=torch.float32, device=device), scale, wrap)

    @staticmethod
    def _records(si):
        if si.uv is None or si.n is None or si.dp_du is None or si.dp_dv is None or si.sh_frame is None or si.sh_frame.n is None:
            raise ValueError("BumpMap: the interaction has no uv / n / dp_du / dp_dv / shading normal (compute it with RayFlags.All)")
        flags = getattr(si, "ray_flags", None)
        if flags is not None and not (int(flags) & int(RayFlags.dPdUV) and int(flags) & int(RayFlags.UV)):
            raise ValueError("BumpMap: the interaction was computed without RayFlags.UV | RayFlags.dPdUV (flags %#x)" % int(flags))
        return si.uv, si.sh_frame.n, si.dp_du, si.dp_dv, si.n

    def normal(self, si, active=True, return_mask=False):
        """the perturbed shading normal [3, n] of the interaction ``si`` (``hf_bumpmap_eval``): one launch, and one each
        for ``backward`` and ``jvp``.  Differentiable in ``data``, ``si.uv`` (with the cell held), ``si.sh_frame.n``,
        ``si.dp_du`` and ``si.dp_dv``, so gradients flow on into the heights and ``to_world``; ``si.n`` only picks the side.  A
        lane that is inactive, not finite, without a lookup or with degenerate tangents passes ``si.sh_frame.n`` through bit
        for bit.  With ``return_mask`` also the [n] uint8 row: 1 where perturbed.  ``si`` must have been computed with
        ``RayFlags.UV | RayFlags.dPdUV`` (ValueError)."""
        uv, sh_n, dp_du, dp_dv, n_geo = self._records(si)
        n = uv.shape[1]
        out, mask = _BumpMapOp.apply(self.data, uv, sh_n, dp_du, dp_dv, n_geo, _caustic_active(active, n, uv.device),
                                     _WRAPS[self.wrap], self.scale)
        return (out, mask) if return_mask else out

    def perturb(self, si, active=True):
        """a shallow copy of ``si`` whose ``sh_frame`` is ``Frame3f(s, t, N)`` with ``N = self.normal(si, active)``:
        ``NormalMap.perturb``'s host-side frame rebuild; only ``N`` carries a gradient."""
        return _with_normal(si, self.normal(si, active))

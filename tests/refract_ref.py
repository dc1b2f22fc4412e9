"""The refraction view (include/hf.h hf_refract_*, hf_bitmap_*) restated in numpy from the formulas of the header, not from
the kernel: the bitmap lookup of a film position (both wraps, its slopes and bilinear weights), the value of a sample --
the caustic row's vertex (caustic_ref.vertex) with the radiance-mode factor eta_ti^2, the absorption along the transmitted
segment and the texture where it lands -- the box film, and the adjoint and the tangent with respect to sh_n, p, weight
and the texels.  float64 by default; `dtype=np.float32` evaluates the same text in float32 (numpy has no fused
multiply-add: the order of operations then differs from the kernel's, which is what the tests' factor of four on the
float32-against-float64 error stands for).  All arrays are [3, n] / [2, n] / [n], world space.  A helper module."""
import types

import numpy as np

import caustic_ref as C
from caustic_ref import NOWHERE, plane_z, receiver  # noqa: F401

CLAMP, REPEAT = 0, 1
FAR = 8388608.0        # 2^23: beyond it (or not finite) a coordinate has no cell


def _axis(pos, res, wrap, dtype):
    """(i0, i1, f, ok) of one axis: q = pos - 0.5, i0 = floor(q), f = q - i0, the texels wrap(i0) and wrap(i0 + 1)"""
    with np.errstate(invalid="ignore"):
        q = np.asarray(pos, dtype) - dtype(0.5)
        far = ~(np.abs(q) < FAR)
        qs = np.where(far, dtype(0), q)
        fl = np.floor(qs)
        f = np.where(far, dtype(0), qs - fl).astype(dtype)
        i = fl.astype(np.int64)
        if wrap == CLAMP:
            edge = np.where(q > 0, res - 1, 0)              # what a float clamp of q to [-1, res] reads (NaN: -1)
            i0 = np.where(far, edge, np.clip(i, 0, res - 1))
            i1 = np.where(far, edge, np.clip(i + 1, 0, res - 1))
            return i0, i1, f, np.ones(q.shape, bool)
        return np.where(far, 0, np.mod(i, res)), np.where(far, 0, np.mod(i + 1, res)), f, ~far


def lookup(tex, pos, wrap, dtype=np.float64):
    """the bilinear lookup of film positions pos [2, n] in tex [TH, TW]: L, the slopes (Lx, Ly) with the cell held, the
    flat indices idx [4, n] of the texels v00, v10, v01, v11 and their bilinear weights b [4, n]"""
    tex = np.asarray(tex, dtype)
    TH, TW = tex.shape
    x0, x1, fx, okx = _axis(pos[0], TW, wrap, dtype)
    y0, y1, fy, oky = _axis(pos[1], TH, wrap, dtype)
    ok = okx & oky
    one = dtype(1)
    gx, gy = one - fx, one - fy
    e = types.SimpleNamespace(ok=ok, fx=fx, fy=fy)
    e.idx = np.stack([y0 * TW + x0, y0 * TW + x1, y1 * TW + x0, y1 * TW + x1])
    v00, v10, v01, v11 = (tex.ravel()[j] for j in e.idx)
    z = dtype(0)
    e.b = np.where(ok[None], np.stack([gy * gx, gy * fx, fy * gx, fy * fx]), z)
    e.L = np.where(ok, gy * (gx * v00 + fx * v10) + fy * (gx * v01 + fx * v11), z)
    e.Lx = np.where(ok, gy * (v10 - v00) + fy * (v11 - v01), z)
    e.Ly = np.where(ok, gx * (v01 - v00) + fx * (v11 - v10), z)
    return e


def near_border(pos, B):
    """lanes whose position lies within B texel of a border between two cells of the lookup (a texel centre line) in
    either coordinate: another rounding of pos may read another cell there"""
    with np.errstate(invalid="ignore"):
        q = np.asarray(pos, np.float64) - 0.5
        f = q - np.floor(q)
        return (np.minimum(f, 1 - f) < B).any(0)


def _shade(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, dtype):
    """what forward, adjoint and tangent form of every sample"""
    v = C.vertex(p, nrm, sh_n, d, t, active, eta, rcv, dtype)
    s = types.SimpleNamespace(v=v)
    s.lit = v.traced & np.asarray(vis).astype(bool)
    s.w = np.ones(v.F.shape, dtype) if weight is None else np.asarray(weight, dtype)
    with np.errstate(all="ignore"):
        X = v.p + v.wo * v.s - rcv.origin.astype(dtype)[:, None]
        s.pos = np.stack([C._dot(X, rcv.ex.astype(dtype)[:, None]), C._dot(X, rcv.ey.astype(dtype)[:, None])])
        s.e = lookup(tex, np.where(s.lit[None], s.pos, dtype(0)), wrap, dtype)
        outside = v.ci >= 0
        e_ti = np.where(outside, dtype(1) / dtype(eta), dtype(eta)).astype(dtype)
        s.oneF = dtype(1) - v.F
        T = np.exp(-dtype(sigma_t) * v.s).astype(dtype) if sigma_t != 0 else dtype(1)
        s.k = ((e_ti * e_ti) * T).astype(dtype)
        s.A = s.w * s.k
    return s


def film(value, spp):
    """the box film: image[i / spp] = 1/spp sum value_i"""
    return value.reshape(-1, spp).mean(1)


def forward(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, spp=1, dtype=np.float64):
    """(value [n], image [n / spp], pos [2, n]) for the visibility `vis` (a sample sees the receiver when it is traced
    and vis says so); value = weight (1 - F) eta_ti^2 exp(-sigma_t s) L(pos)"""
    s = _shade(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, dtype)
    with np.errstate(all="ignore"):
        value = np.where(s.lit, (s.A * s.oneF) * s.e.L, dtype(0))
    return value, film(value, spp), np.where(s.lit[None], s.pos, dtype(NOWHERE))


def adjoint(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, gimg, gvalue, spp=1, dtype=np.float64):
    """(grad_sh_n [3, n], grad_p [3, n], grad_weight [n], grad_tex [TH, TW]) for dL/dimage [n / spp] and dL/dvalue [n]
    (None: zero)"""
    s = _shade(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, dtype)
    v, n = s.v, s.lit.size
    g = np.zeros(n, dtype)
    if gimg is not None:
        g = g + np.repeat(np.asarray(gimg, dtype), spp) / dtype(spp)
    if gvalue is not None:
        g = g + np.asarray(gvalue, dtype)
    N = rcv.N.astype(dtype)[:, None]
    z = dtype(0)
    with np.errstate(all="ignore"):
        gA = g * s.A
        gAF = gA * s.oneF
        gw = g * (s.oneF * s.k) * s.e.L
        gX = rcv.ex.astype(dtype)[:, None] * (gAF * s.e.Lx) + rcv.ey.astype(dtype)[:, None] * (gAF * s.e.Ly)
        gs = C._dot(gX, v.wo) - gAF * dtype(sigma_t) * s.e.L
        c = -gs / v.b
        gp = gX + N * c
        gwo = gX * v.s + N * (c * v.s)
        gci = v.dq * C._dot(v.m, gwo) - gA * v.dF * s.e.L
        gm = gwo * v.q + v.wi * gci
    gtex = np.zeros(np.asarray(tex).size, dtype)
    for j in range(4):
        np.add.at(gtex, s.e.idx[j][s.lit], (gAF * s.e.b[j])[s.lit])
    return np.where(s.lit[None], gm, z), np.where(s.lit[None], gp, z), np.where(s.lit, gw, z), gtex.reshape(np.asarray(tex).shape)


def tangent(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, dn, dp, dw, dtex, spp=1, dtype=np.float64):
    """(dvalue [n], dimage [n / spp]) for tangents dn of sh_n, dp of p, dw of weight and dtex of the texels (None: zero)"""
    s = _shade(p, nrm, sh_n, d, t, active, weight, eta, sigma_t, rcv, tex, wrap, vis, dtype)
    v = s.v
    zero3 = np.zeros(v.m.shape, dtype)
    dn = zero3 if dn is None else np.asarray(dn, dtype)
    dp = zero3 if dp is None else np.asarray(dp, dtype)
    dw = np.zeros(v.F.shape, dtype) if dw is None else np.asarray(dw, dtype)
    N = rcv.N.astype(dtype)[:, None]
    with np.errstate(all="ignore"):
        dci = C._dot(dn, v.wi)
        dwo = dn * v.q + v.m * (v.dq * dci)
        ds = -(C._dot(dp, N) + v.s * C._dot(dwo, N)) / v.b
        dX = dp + v.wo * ds + dwo * v.s
        dx, dy = C._dot(dX, rcv.ex.astype(dtype)[:, None]), C._dot(dX, rcv.ey.astype(dtype)[:, None])
        dL = s.e.Lx * dx + s.e.Ly * dy - dtype(sigma_t) * s.e.L * ds
        if dtex is not None:
            dt = np.asarray(dtex, dtype).ravel()
            dL = dL + sum(s.e.b[j] * dt[s.e.idx[j]] for j in range(4))
        dvalue = dw * (s.oneF * s.k) * s.e.L + s.A * (s.oneF * dL - v.dF * dci * s.e.L)
    dvalue = np.where(s.lit, dvalue, dtype(0))
    return dvalue, film(dvalue, spp)


def textures(TW, TH):
    """the two textures of the row's tests as float32 [TH, TW]: a smooth sum of sines and a random one"""
    y, x = np.meshgrid((np.arange(TH) + 0.5) / TH, (np.arange(TW) + 0.5) / TW, indexing="ij")
    smooth = 0.6 + 0.25 * np.sin(2 * np.pi * 1.5 * x + 0.4) + 0.15 * np.sin(2 * np.pi * y + 1.1) * np.cos(2 * np.pi * x)
    return {"smooth": smooth.astype(np.float32), "random": np.random.default_rng(17).uniform(0.1, 1.0, (TH, TW)).astype(np.float32)}


def inputs(n, spp, tex_shape):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(3)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(n // spp), gv=f(n), dn=f(3, n), dp=f(3, n),
                                 dw=f(n), dtex=f(*tex_shape))


def whole_pixels(keep, spp):
    """the pixels all of whose samples are in `keep`"""
    return keep.reshape(-1, spp).all(1)

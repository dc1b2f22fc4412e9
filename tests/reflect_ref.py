"""Specular reflection of the environment map (include/hf.h hf_reflect_*) restated in numpy from the formulas of the
header, not from the kernel: the specular vertex (fresnel(), reflect(), the masks), the map lookup and its derivative
with respect to the direction, the value, and the adjoint and the tangent with respect to sh_n, weight and the texels.
float64 by default; `dtype=np.float32` evaluates the same text in float32 (numpy has no fused multiply-add and its
atan2 / acos are float32 then: the order of operations differs from the kernel's, which is what the tests' factor of
four on the float32-against-float64 error stands for).  All arrays are [3, n] / [n], world space; `data` is the [H, W]
map with its seam column, `rot` the 3 x 3 rotation map -> world (None: identity).  Visibility is an input: nothing here
traces.  A helper module."""
import types

import numpy as np

import sky_ref as S
from caustic_ref import fresnel
from envmap_ref import bilinear_weights, corners

POLE = 1e-12       # s2 or q below this: the direction derivative of the lookup is exactly zero


def _dot(a, b):
    return (a * b).sum(0)


def vertex(nrm, sh_n, d, t, active, eta, dtype=np.float64):
    """the specular vertex of every sample: the masks, wr, F, F'; `margin`: the smallest magnitude among the quantities
    whose sign decides a mask (c, <g, wi> and, for an eligible lane, <g, wr>)"""
    g, m, d = (np.asarray(x, dtype) for x in (nrm, sh_n, d))
    t = np.asarray(t)
    act = np.ones(m.shape[1], bool) if active is None else np.asarray(active).astype(bool)
    v = types.SimpleNamespace()
    wi = -d
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        c, gi = _dot(m, wi), _dot(g, wi)
        v.eligible = act & np.isfinite(t) & (c > 0) & (gi > 0)
        if eta == 0:                                    # the ideal mirror
            v.F, v.dF = np.ones(c.shape, dtype), np.zeros(c.shape, dtype)
        else:
            F, ct, _, _ = fresnel(c, eta, dtype)        # (c > 0 on every lane that is used: eta_it = eta)
            e = dtype(eta)
            cta = np.abs(ct).astype(dtype)
            dct = c / (e * e) / cta                     # d cos_theta_t / d c from cos_theta_t^2 = 1 - (1 - c^2) / eta^2
            ds_, dp_ = c + e * cta, cta + e * c
            a_s, a_p = (c - e * cta) / ds_, (cta - e * c) / dp_
            das = two * e * (cta - c * dct) / (ds_ * ds_)
            dap = two * e * (c * dct - cta) / (dp_ * dp_)
            tir = one - (one - c * c) / (e * e) <= 0    # F = 1 there, a constant
            v.F = F.astype(dtype)
            v.dF = np.where((e == 1) | tir, 0, a_s * das + a_p * dap).astype(dtype)
        v.wr = m * (two * c) - wi
        go = _dot(g, v.wr)
        v.consistent = go > 0
        v.traced = v.eligible & v.consistent
        first = np.minimum(np.abs(c), np.abs(gi))
        v.margin = np.where(v.eligible, np.minimum(first, np.abs(go)), first)
    v.wi, v.m, v.c = wi, m, c
    return v


def rays(p, nrm, sh_n, d, t, active=None):
    """(traced, origin [3, n], direction [3, n], maxt [n], vertex) of the reflected rays; untraced lanes: zero ray, maxt -1"""
    v = vertex(nrm, sh_n, d, t, active, 0.0)
    wr = np.where(v.traced[None], v.wr, 0.0)
    o = np.where(v.traced[None], S.spawn_origin(np.asarray(p, np.float64), np.asarray(nrm, np.float64), wr), 0.0)
    return v.traced, o, wr, np.where(v.traced, np.inf, -1.0), v


def lookup(w, W, H, rot=None, dtype=np.float64):
    """Emitter::eval's map coordinates of the world directions w [3, n] and what the direction derivative needs:
    (cx, cy, fx, fy, v = R^T w, R)"""
    R = (np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)).astype(dtype)
    v = (R.T @ np.asarray(w, dtype)).astype(dtype)
    pi = dtype(np.pi)
    with np.errstate(all="ignore"):
        ux = np.arctan2(v[0], -v[2]) / (dtype(2) * pi) - dtype(0.5) / dtype(W - 1)
        uy = np.arccos(np.clip(v[1], dtype(-1), dtype(1))) / pi
        ux = (ux - np.floor(ux)) * dtype(W - 1); uy = (uy - np.floor(uy)) * dtype(H - 1)
        cx = np.minimum(np.nan_to_num(ux).astype(np.int64), W - 2); cy = np.minimum(np.nan_to_num(uy).astype(np.int64), H - 2)
    return cx, cy, (ux - cx).astype(dtype), (uy - cy).astype(dtype), v, R


def shade(w, data, rot=None, dtype=np.float64):
    """per direction: L, G = R dL/dv [3, n] (zero at the poles), the bilinear weights b [4, n], the texel indices
    idx [4, n], and `pole`"""
    data = np.asarray(data, dtype)
    H, W = data.shape
    cx, cy, fx, fy, v, R = lookup(w, W, H, rot, dtype)
    idx = corners(W, cx, cy)
    b = bilinear_weights(fx, fy).astype(dtype)
    tex = data.ravel()[idx]
    one, pi = dtype(1), dtype(np.pi)
    with np.errstate(all="ignore"):
        L = (b * tex).sum(0)
        Lx = (one - fy) * (tex[1] - tex[0]) + fy * (tex[3] - tex[2])
        Ly = (one - fx) * (tex[2] - tex[0]) + fx * (tex[3] - tex[1])
        s2, q = v[0] * v[0] + v[2] * v[2], one - v[1] * v[1]
        pole = (s2 < POLE) | (q < POLE)
        kx = Lx * dtype(W - 1) / (dtype(2) * pi) / s2
        dv = np.stack([-kx * v[2], -Ly * dtype(H - 1) / pi / np.sqrt(q), kx * v[0]])
        G = np.where(pole[None], 0, R @ dv).astype(dtype)
    return types.SimpleNamespace(L=L, G=G, b=b, idx=idx, pole=pole, fx=fx, fy=fy)


def smooth_lanes(w, W, H, rot=None, border=1e-4):
    """lanes whose lookup is at least `border` of a cell away from a cell border and not at a pole: where the value is a
    smooth function of the direction"""
    _, _, fx, fy, v, _ = lookup(w, W, H, rot)
    pole = (v[0] * v[0] + v[2] * v[2] < POLE) | (1 - v[1] * v[1] < POLE)
    return (np.minimum.reduce([fx, 1 - fx, fy, 1 - fy]) >= border) & ~pole


def _common(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, dtype):
    v = vertex(nrm, sh_n, d, t, active, eta, dtype)
    lit = v.traced & np.asarray(vis).astype(bool)
    w = np.ones(v.F.shape, dtype) if weight is None else np.asarray(weight, dtype)
    return v, lit, w, shade(v.wr, data, rot, dtype)


def forward(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, spp=1, dtype=np.float64):
    """(image [n / spp], value [n]) for the visibility `vis` (a sample counts when it is traced and vis says so)"""
    v, lit, w, s = _common(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, dtype)
    value = np.where(lit, (w * v.F) * s.L, dtype(0)).astype(dtype)
    return value.reshape(-1, spp).mean(1, dtype=dtype), value


def adjoint(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, spp, grad_image, grad_value, dtype=np.float64):
    """(grad_sh_n [3, n], grad_weight [n], grad_data [H, W]) for dL/dimage [n / spp] and dL/dvalue [n] (None: zero)"""
    v, lit, w, s = _common(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, dtype)
    g = np.zeros(v.F.shape, dtype)
    if grad_image is not None:
        g = g + np.repeat(np.asarray(grad_image, dtype), spp) / dtype(spp)
    if grad_value is not None:
        g = g + np.asarray(grad_value, dtype)
    two, z = dtype(2), dtype(0)
    with np.errstate(all="ignore"):
        gm = (g * w) * (v.wi * (v.dF * s.L) + two * v.F * (s.G * v.c + v.wi * _dot(v.m, s.G)))
        gw = g * v.F * s.L
        contrib = np.where(lit[None], (g * w * v.F)[None] * s.b, z)
    gd = np.zeros(np.asarray(data).size, dtype)
    np.add.at(gd, s.idx[:, lit], contrib[:, lit])
    return np.where(lit[None], gm, z), np.where(lit, gw, z), gd.reshape(np.asarray(data).shape)


def tangent(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, spp, dsh_n=None, dweight=None, ddata=None, dtype=np.float64):
    """(dimage [n / spp], dvalue [n]) for tangents dsh_n [3, n], dweight [n] and ddata [H, W] (None: zero)"""
    v, lit, w, s = _common(nrm, sh_n, d, t, active, weight, eta, data, rot, vis, dtype)
    dn = np.zeros(v.m.shape, dtype) if dsh_n is None else np.asarray(dsh_n, dtype)
    dw = np.zeros(v.F.shape, dtype) if dweight is None else np.asarray(dweight, dtype)
    two = dtype(2)
    with np.errstate(all="ignore"):
        dci = _dot(dn, v.wi)
        dwr = two * (dn * v.c + v.m * dci)
        dv = dw * v.F * s.L + w * (v.dF * dci * s.L + v.F * _dot(s.G, dwr))
        if ddata is not None:
            dv = dv + w * v.F * (s.b * np.asarray(ddata, dtype).ravel()[s.idx]).sum(0)
    dv = np.where(lit, dv, dtype(0)).astype(dtype)
    return dv.reshape(-1, spp).mean(1, dtype=dtype), dv

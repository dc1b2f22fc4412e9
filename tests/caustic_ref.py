"""Refractive caustics (include/hf.h hf_caustic_*) restated in numpy from the formulas of the header, not from the kernel:
the specular vertex (fresnel(), refract(), the masks, the receiver), the landing position and value, and the adjoint and
the tangent with respect to sh_n, p and weight.  float64 by default; `dtype=np.float32` evaluates the same text in float32
(numpy has no fused multiply-add: the order of operations then differs from the kernel's, which is what the tests' factor
of four on the float32-against-float64 error stands for).  All arrays are [3, n] / [n], world space.  A helper module."""
import types

import numpy as np

import sky_ref as S

NOWHERE = -16.0        # pos of a sample that deposits nothing: outside every film by more than the filter radius


def receiver(origin, ex, ey):
    """the plane through origin spanned by ex, ey; N = normalize(ex x ey)"""
    o, ex, ey = (np.asarray(v, np.float64) for v in (origin, ex, ey))
    N = np.cross(ex, ey)
    return types.SimpleNamespace(origin=o, ex=ex, ey=ey, N=N / np.linalg.norm(N))


def plane_z(z, x_range, y_range, width, height):
    sx, sy = width / (x_range[1] - x_range[0]), height / (y_range[1] - y_range[0])
    return receiver((x_range[0], y_range[0], z), (sx, 0.0, 0.0), (0.0, sy, 0.0))


def fresnel(ci, eta, dtype=np.float64):
    """fresnel() of include/mitsuba/render/fresnel.h:35-71 with its special cases: (F, cos_theta_t, eta_it, eta_ti)"""
    ci = np.asarray(ci, dtype)
    eta = dtype(eta)
    one = dtype(1)
    outside = ci >= 0
    rcp = one / eta
    eta_it, eta_ti = np.where(outside, eta, rcp), np.where(outside, rcp, eta)
    ct2 = one - (one - ci * ci) * (eta_ti * eta_ti)
    cia, cta = np.abs(ci), np.sqrt(np.maximum(ct2, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        a_s = (cia - eta_it * cta) / (cia + eta_it * cta)
        a_p = (cta - eta_it * cia) / (cta + eta_it * cia)
    F = dtype(0.5) * (a_s * a_s + a_p * a_p)
    F = np.where(eta == 1, 0, np.where(cia == 0, 1, F)).astype(dtype)
    return F, np.where(outside, -cta, cta), eta_it, eta_ti


def _dot(a, b):
    return (a * b).sum(0)


def vertex(p, nrm, sh_n, d, t, active, eta, rcv, dtype=np.float64):
    """the specular vertex of every sample: the masks, wo, s, F and what the derivatives need; `margin`: the smallest
    magnitude among the quantities whose sign or vanishing decides a mask (a lane below a few float32 roundings of it is
    decided by rounding)"""
    p, g, m, d = (np.asarray(x, dtype) for x in (p, nrm, sh_n, d))
    t = np.asarray(t)
    n = m.shape[1]
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    N, org = rcv.N.astype(dtype)[:, None], rcv.origin.astype(dtype)[:, None]
    v = types.SimpleNamespace()
    wi = -d
    with np.errstate(all="ignore"):
        ci, gi = _dot(m, wi), _dot(g, wi)
        v.eligible = act & np.isfinite(t) & (ci != 0) & (gi * ci > 0)
        outside = ci >= 0
        eta_ = dtype(eta)
        rcp = dtype(1) / eta_
        eta_it, e = np.where(outside, eta_, rcp), np.where(outside, rcp, eta_)
        ct2 = dtype(1) - (dtype(1) - ci * ci) * (e * e)
        v.tir = ct2 <= 0
        cia, cta = np.abs(ci), np.sqrt(np.maximum(ct2, 0))
        ds_, dp_ = cia + eta_it * cta, cta + eta_it * cia
        a_s, a_p = (cia - eta_it * cta) / ds_, (cta - eta_it * cia) / dp_
        matched = eta_ == 1
        v.F = np.where(matched, 0, dtype(0.5) * (a_s * a_s + a_p * a_p)).astype(dtype)
        ct = np.where(outside, -cta, cta)
        v.q = ci * e + ct
        v.wo = m * v.q - wi * e
        go = _dot(g, v.wo)
        v.consistent = go * gi < 0
        v.b = _dot(v.wo, N)
        v.s = _dot(org - p, N) / v.b
        v.reach = np.isfinite(v.s) & (v.s > 0)
        v.traced = v.eligible & ~v.tir & v.consistent & v.reach
        sg = np.where(outside, 1, -1).astype(dtype)
        dcta = ci * e * e / cta
        das = 2 * ((eta_it * cta) * sg - cia * (eta_it * dcta)) / (ds_ * ds_)
        dap = 2 * ((eta_it * cia) * dcta - cta * (eta_it * sg)) / (dp_ * dp_)
        v.dF = np.where(matched, 0, a_s * das + a_p * dap).astype(dtype)
        v.dq = e - sg * dcta
        # the masks are decided in order: what follows a failed one decides nothing
        first = np.minimum.reduce([np.abs(ci), np.abs(gi * ci), np.abs(ct2)])
        v.margin = np.where(v.eligible & ~v.tir, np.minimum.reduce([first, np.abs(go * gi), np.abs(v.s), np.abs(v.b)]), first)
    v.wi, v.m, v.p, v.ci, v.ct2 = wi, m, p, ci, ct2
    return v


def rays(p, nrm, sh_n, d, t, active, eta, rcv):
    """(traced, origin [3, n], direction [3, n], maxt [n]) of the refracted rays; untraced lanes: zero ray, maxt -1"""
    v = vertex(p, nrm, sh_n, d, t, active, eta, rcv)
    wo = np.where(v.traced[None], v.wo, 0.0)
    o = np.where(v.traced[None], S.spawn_origin(np.asarray(p, np.float64), np.asarray(nrm, np.float64), wo), 0.0)
    return v.traced, o, wo, np.where(v.traced, v.s, -1.0), v


def forward(p, nrm, sh_n, d, t, active, weight, eta, power, rcv, vis, dtype=np.float64):
    """(pos [2, n], value [n]) for the deposit mask `vis` (a sample deposits when it is traced and vis says so)"""
    v = vertex(p, nrm, sh_n, d, t, active, eta, rcv, dtype)
    lit = v.traced & np.asarray(vis).astype(bool)
    w = np.ones(v.F.shape, dtype) if weight is None else np.asarray(weight, dtype)
    with np.errstate(all="ignore"):
        X = v.p + v.wo * v.s - rcv.origin.astype(dtype)[:, None]
        pos = np.stack([_dot(X, rcv.ex.astype(dtype)[:, None]), _dot(X, rcv.ey.astype(dtype)[:, None])])
        value = w * (dtype(power) * (1 - v.F))
    return np.where(lit[None], pos, dtype(NOWHERE)), np.where(lit, value, dtype(0))


def adjoint(p, nrm, sh_n, d, t, active, weight, eta, power, rcv, vis, gpos, gvalue, dtype=np.float64):
    """(grad_sh_n [3, n], grad_p [3, n], grad_weight [n]) for dL/dpos [2, n] and dL/dvalue [n]"""
    v = vertex(p, nrm, sh_n, d, t, active, eta, rcv, dtype)
    lit = v.traced & np.asarray(vis).astype(bool)
    w = np.ones(v.F.shape, dtype) if weight is None else np.asarray(weight, dtype)
    gpos, gv = np.asarray(gpos, dtype), np.asarray(gvalue, dtype)
    N = rcv.N.astype(dtype)[:, None]
    with np.errstate(all="ignore"):
        gX = rcv.ex.astype(dtype)[:, None] * gpos[0] + rcv.ey.astype(dtype)[:, None] * gpos[1]
        c = -_dot(gX, v.wo) / v.b
        gp = gX + N * c
        gwo = gX * v.s + N * (c * v.s)
        gci = v.dq * _dot(v.m, gwo) - (w * dtype(power) * v.dF) * gv
        gm = gwo * v.q + v.wi * gci
        gw = dtype(power) * (1 - v.F) * gv
    z = dtype(0)
    return np.where(lit[None], gm, z), np.where(lit[None], gp, z), np.where(lit, gw, z)


def tangent(p, nrm, sh_n, d, t, active, weight, eta, power, rcv, vis, dn, dp, dw, dtype=np.float64):
    """(dpos [2, n], dvalue [n]) for tangents dn of sh_n, dp of p, dw of weight (None: zero)"""
    v = vertex(p, nrm, sh_n, d, t, active, eta, rcv, dtype)
    lit = v.traced & np.asarray(vis).astype(bool)
    w = np.ones(v.F.shape, dtype) if weight is None else np.asarray(weight, dtype)
    zero3 = np.zeros(v.m.shape, dtype)
    dn = zero3 if dn is None else np.asarray(dn, dtype)
    dp = zero3 if dp is None else np.asarray(dp, dtype)
    dw = np.zeros(v.F.shape, dtype) if dw is None else np.asarray(dw, dtype)
    N = rcv.N.astype(dtype)[:, None]
    with np.errstate(all="ignore"):
        dci = _dot(dn, v.wi)
        dwo = dn * v.q + v.m * (v.dq * dci)
        ds = -(_dot(dp, N) + v.s * _dot(dwo, N)) / v.b
        dX = dp + v.wo * ds + dwo * v.s
        dpos = np.stack([_dot(dX, rcv.ex.astype(dtype)[:, None]), _dot(dX, rcv.ey.astype(dtype)[:, None])])
        dvalue = dw * (dtype(power) * (1 - v.F)) - (w * dtype(power) * v.dF) * dci
    z = dtype(0)
    return np.where(lit[None], dpos, z), np.where(lit, dvalue, z)


def filter_mass(stddev=0.5):
    """(int w)^2 of the film's filter w(x) = exp(-x^2 / (2 stddev^2)) - exp(-8) on |x| <= 4 stddev, by quadrature"""
    x = np.linspace(-4 * stddev, 4 * stddev, 400001)
    w = np.exp(-x * x / (2 * stddev * stddev)) - np.exp(-8.0)
    return float(((w[:-1] + w[1:]).sum() * 0.5 * (x[1] - x[0])) ** 2)


def film(pos, value, width, height, stddev=0.5):
    """the accumulated Gaussian film of the samples over the filter's mass, [height, width], float64"""
    img = np.zeros((height, width))
    r, alpha = 4 * stddev, -1 / (2 * stddev * stddev)
    bias = np.exp(alpha * r * r)
    for k in np.flatnonzero(np.asarray(value) != 0):
        fx, fy = pos[0][k] - 0.5, pos[1][k] - 0.5
        x0, x1 = max(int(np.ceil(fx - r)), 0), min(int(np.floor(fx + r)), width - 1)
        y0, y1 = max(int(np.ceil(fy - r)), 0), min(int(np.floor(fy + r)), height - 1)
        if x1 < x0 or y1 < y0:
            continue
        wx = np.maximum(np.exp(alpha * (np.arange(x0, x1 + 1) - fx) ** 2) - bias, 0)
        wy = np.maximum(np.exp(alpha * (np.arange(y0, y1 + 1) - fy) ** 2) - bias, 0)
        img[y0:y1 + 1, x0:x1 + 1] += value[k] * wy[:, None] * wx[None]
    return img / filter_mass(stddev)

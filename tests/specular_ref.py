"""The specular row (include/hf.h hf_specular_lighting, _adjoint, _tangent) restated in numpy.  The value is the
reflection lobe of a rough surface as the reference evaluates it -- roughplastic.cpp:315-350 and roughconductor.cpp's
eval: F D G / (4 cos theta_i), with MicrofacetDistribution::eval (microfacet.h:185-207, the isotropic GGX branch),
smith_g1 (microfacet.h:341-365) and fresnel() (fresnel.h:35-71) -- times the irradiance of a `directional` emitter
(directional.cpp:150-177) from l = to_light / |to_light|.  forward / tangent / adjoint are what the header FREEZES.  The
tangent is the header's closed form; the adjoint is a reverse sweep through the steps of the forward, written on its own:
it shares no line with the tangent.  Visibility is an input, [K, n] booleans (bit k of the directional row's byte):
nothing here traces.  (The header's clause for cosines below about 1e-13, where the float32 G1 leaves its range and its
log-derivative counts as 0, has no counterpart here: float64 does not leave its range there.)  float64 by default; `dtype=np.float32` evaluates the same text in float32
(scripts/specular_f32_error.py).  The rig, the scenes, the film and the error measures are directional_ref's, G1 is
glossy_ref's.  A helper module."""
import types

import numpy as np

import directional_ref as D
from directional_ref import NAMES, ORIGINS, PARAMS, RIG, SPP, film, light, oracle_scenes, pack, rig, row4, unit, unpack  # noqa: F401
from glossy_ref import smith
from sensor_ref import err_abs, err_l2

ALPHA_MIN = 1e-4
ETA = 1.5


def _dot(a, b):
    return (a * b).sum(0)


def fresnel(u, eta, dt=np.float64):
    """(F, dF/du) of the unpolarised fresnel() of fresnel.h:35-71 seen from outside (u = <wi, h> > 0 on every lane that
    is used).  eta = 0: the ideal mirror F = 1; eta = 1: F = 0; under total internal reflection F = 1, a constant"""
    u = np.asarray(u, dt)
    if eta == 0:
        return np.ones(u.shape, dt), np.zeros(u.shape, dt)
    one, two, e = dt(1), dt(2), dt(eta)
    with np.errstate(all="ignore"):
        ct2 = one - (one - u * u) / (e * e)
        cta = np.sqrt(np.maximum(ct2, dt(0)))
        dct = u / (e * e) / cta
        ds_, dp_ = u + e * cta, cta + e * u
        a_s, a_p = (u - e * cta) / ds_, (cta - e * u) / dp_
        das = two * e * (cta - u * dct) / (ds_ * ds_)
        dap = two * e * (u * dct - cta) / (dp_ * dp_)
        F = dt(0.5) * (a_s * a_s + a_p * a_p)
        flat = (e == 1) | (ct2 <= 0)
        return (np.where(e == 1, dt(0), F).astype(dt), np.where(flat, dt(0), a_s * das + a_p * dap).astype(dt))


def ggx(ch, a, dt=np.float64):
    """(D, s^2, q) of MicrofacetDistribution::eval, isotropic GGX (microfacet.h:185-207):
    D = 1 / (pi a^2 q^2), q = s^2 / a^2 + c_h^2, s^2 = max(1 - c_h^2, 0)"""
    s2 = np.maximum(dt(1) - ch * ch, dt(0))
    q = s2 / (a * a) + ch * ch
    return dt(1) / (dt(np.pi) * a * a * q * q), s2, q


def roughness(alpha, n, dt=np.float64):
    """the [n] row of a scalar or a row, and a = max(alpha, 1e-4)"""
    al = np.broadcast_to(np.asarray(alpha, dt), (n,)).astype(dt)
    return al, np.maximum(al, dt(ALPHA_MIN))


def _terms(L, sh_n, d, weight, alpha, eta, vis, dt):
    """the steps of the forward of every sample under one light"""
    x = types.SimpleNamespace(dt=dt)
    x.sn = np.asarray(sh_n, dt)
    x.n = x.sn.shape[1]
    x.wi = -np.asarray(d, dt)
    x.l, x.len = unit(L, dt)
    x.lc = x.l[:, None]
    x.E = dt(L.irradiance)
    x.w = np.ones(x.n, dt) if weight is None else np.asarray(weight, dt)
    x.alpha, x.a = roughness(alpha, x.n, dt)
    with np.errstate(all="ignore"):
        x.ci, x.co = _dot(x.sn, x.wi), _dot(x.sn, x.lc)
        x.ok = np.asarray(vis, bool) & np.isfinite(x.alpha) & (x.ci > 0) & (x.co > 0)
        m = x.wi + x.lc
        x.M = np.sqrt(_dot(m, m))
        x.h = m / x.M
        x.ch, x.u = _dot(x.sn, x.h), _dot(x.wi, x.h)
        x.F, x.dF = fresnel(x.u, eta, dt)
        x.Gi, x.Gi_c, x.Gi_a = smith(x.a, x.ci, dt)
        x.Go, x.Go_c, x.Go_a = smith(x.a, x.co, dt)
        x.D, x.s2, x.q = ggx(x.ch, x.a, dt)
        x.R = x.D * x.Gi * x.Go / (dt(4) * x.ci)
        x.v = x.F * x.R
    return x


def forward(lights, sh_n, d, weight, alpha, eta, vis, spp=1, dtype=np.float64):
    """(image [K, n / spp], value [K, n])"""
    value = []
    for L, v in zip(lights, vis):
        x = _terms(L, sh_n, d, weight, alpha, eta, v, dtype)
        value.append(np.where(x.ok, x.w * x.E * x.v, dtype(0)))
    value = np.stack(value)
    return np.stack([film(v, spp) for v in value]), value


def partials(x):
    """the header's closed partial derivatives of v: (N [3, n], A [n], Ld [3, n])"""
    dt = x.dt
    with np.errstate(all="ignore"):
        ia2 = dt(1) / (x.a * x.a)
        kD = dt(-4) * x.ch * (dt(1) - np.where(x.s2 > 0, ia2, dt(0))) / x.q
        kDa = dt(-2) / x.a + dt(4) * x.s2 * ia2 / (x.a * x.q)
        ki, ko = x.Gi_c / x.Gi - dt(1) / x.ci, x.Go_c / x.Go
        ka = x.Gi_a / x.Gi + x.Go_a / x.Go
        N = x.v * (kD * x.h + ki * x.wi + ko * x.lc)
        A = x.v * (kDa + ka)
        Ld = x.v * ko * x.sn + (x.v * kD * (x.sn - x.h * x.ch) + x.R * x.dF * (x.wi - x.h * x.u)) / x.M
    return N, A, Ld


def tangent(lights, sh_n, d, weight, alpha, eta, vis, spp=1, dn=None, dw=None, da=None, d_lights=None, dtype=np.float64):
    """(dimage [K, n / spp], dvalue [K, n]) for the tangents dn [3, n], dw [n], da [n], d_lights [K, 4] (None: zero)"""
    dt = dtype
    out = []
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, sh_n, d, weight, alpha, eta, v, dt)
        z = lambda a, shape: np.zeros(shape, dt) if a is None else np.broadcast_to(np.asarray(a, dt), shape)
        dnn, dww, daa = z(dn, (3, x.n)), z(dw, x.n), z(da, x.n)
        d4 = np.zeros(PARAMS, dt) if d_lights is None else np.asarray(d_lights, dt)[k]
        dv3, dE = d4[:3], d4[3]
        dl = (dv3 - x.l * _dot(x.l, dv3)) / x.len
        N, A, Ld = partials(x)
        daa = np.where(x.alpha > dt(ALPHA_MIN), daa, dt(0))
        dval = dww * x.E * x.v + x.w * dE * x.v + x.w * x.E * (_dot(N, dnn) + A * daa + _dot(Ld, dl[:, None]))
        out.append(np.where(x.ok, dval, dt(0)))
    out = np.stack(out)
    return np.stack([film(v, spp) for v in out]), out


def adjoint(lights, sh_n, d, weight, alpha, eta, vis, spp=1, grad_image=None, grad_value=None, dtype=np.float64, rows=None):
    """the reverse sweep through the steps of _terms: a namespace with gn [3, n], gw [n], ga [n] (the lights summed in
    light order) and g4 [K, 4].  rows: a slice of the samples the sums g4 are taken over (None: all)"""
    dt = dtype
    K = len(lights)
    out = types.SimpleNamespace(g4=np.zeros((K, PARAMS), dt))
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, sh_n, d, weight, alpha, eta, v, dt)
        if k == 0:
            out.gn, out.gw, out.ga = np.zeros((3, x.n), dt), np.zeros(x.n, dt), np.zeros(x.n, dt)
        keep = np.zeros(x.n, bool)
        keep[slice(None) if rows is None else rows] = True
        g = np.zeros(x.n, dt)
        if grad_image is not None:
            g = g + np.repeat(np.asarray(grad_image, dt)[k], spp) / dt(spp)
        if grad_value is not None:
            g = g + np.asarray(grad_value, dt)[k]
        g = np.where(x.ok, g, dt(0))
        z = lambda a: np.where(x.ok, a, dt(0))                    # (a masked lane carries nothing back)
        with np.errstate(all="ignore"):
            # value = w E v
            b_w, b_E, b_v = z(g * x.E * x.v), z(g * x.w * x.v), z(g * x.w * x.E)
            # v = F R
            b_F, b_R = b_v * x.R, b_v * x.F
            # R = D Gi Go / (4 ci)
            f = dt(1) / (dt(4) * x.ci)
            b_D, b_Gi, b_Go = z(b_R * x.Gi * x.Go * f), z(b_R * x.D * x.Go * f), z(b_R * x.D * x.Gi * f)
            b_ci = z(-b_R * x.R / x.ci)
            # Gi = G1(a, ci), Go = G1(a, co)
            b_ci = b_ci + z(b_Gi * x.Gi_c)
            b_co = z(b_Go * x.Go_c)
            b_a = z(b_Gi * x.Gi_a + b_Go * x.Go_a)
            # D = 1 / (pi a^2 q^2)
            b_q = z(b_D * (dt(-2) * x.D / x.q))
            b_a = b_a + z(b_D * (dt(-2) * x.D / x.a))
            # q = s2 / a^2 + ch^2
            b_s2, b_ch = z(b_q / (x.a * x.a)), z(b_q * dt(2) * x.ch)
            b_a = b_a + z(b_q * (dt(-2) * x.s2 / (x.a * x.a * x.a)))
            # s2 = max(1 - ch^2, 0)
            b_ch = b_ch + np.where(x.s2 > 0, z(b_s2 * (dt(-2) * x.ch)), dt(0))
            # F = F(u), u = <wi, h>, ch = <sn, h>
            b_u = z(b_F * x.dF)
            b_h = b_u * x.wi + b_ch * x.sn
            b_sn = b_ch * x.h
            # h = m / M, m = wi + l
            b_l = z((b_h - x.h * _dot(x.h, b_h)) / x.M)
            # co = <sn, l>, ci = <sn, wi>
            b_sn = b_sn + b_co * x.lc + b_ci * x.wi
            b_l = b_l + b_co * x.sn
            b_sn, b_l = z(b_sn), z(b_l)                           # (a missed lane's records need not be finite)
        out.gw += b_w
        out.gn += b_sn
        out.ga += np.where(x.alpha > dt(ALPHA_MIN), b_a, dt(0))   # a = max(alpha, 1e-4)
        g_l = (b_l * keep[None]).sum(1)                           # dL/dl, as if l were free
        g_v = (g_l - x.l * _dot(x.l, g_l)) / x.len                # l = to_light / |to_light|: the part orthogonal to l
        out.g4[k] = np.append(g_v, (b_E * keep).sum())
    return out


def alpha_row(kind, n, dt=np.float32):
    """the roughness rows of the row's tests: "row" is spread over [0.05, 0.6], "sharp" a constant 0.02"""
    if kind == "sharp":
        return np.full(n, 0.02, dt)
    return (0.05 + 0.55 * np.random.default_rng(21).random(n)).astype(dt)


def inputs(n, spp, K, seed=5):
    """directional_ref's weights, upstream gradients and tangents, and a tangent of alpha"""
    x = D.inputs(n, spp, K, seed)
    x.da = (0.05 * np.random.default_rng(seed + 1).normal(size=n)).astype(np.float32)
    return x


def errors(got, ref):
    """the error measures scripts/specular_f32_error.py records and tests/test_gpu_specular.py holds the kernels to.
    got, ref: namespaces with image, value, dimage, dvalue, gn, gw (or None), ga, g4.  Per-lane quantities: the largest
    difference over max(1, largest value); the reduced rows: relative L2"""
    out = {"image": err_abs(got.image, ref.image), "value": err_abs(got.value, ref.value),
           "dimage": err_abs(got.dimage, ref.dimage), "dvalue": err_abs(got.dvalue, ref.dvalue),
           "grad_sh_n": err_abs(got.gn, ref.gn), "grad_alpha": err_abs(got.ga, ref.ga), "grad4": err_l2(got.g4, ref.g4)}
    if ref.gw is not None and got.gw is not None:
        out["grad_weight"] = err_abs(got.gw, ref.gw)
    return out


def evaluate(lights, sh_n, d, x, alpha, eta, vis, spp, dtype=np.float64, weighted=True):
    """forward, tangent and adjoint under the inputs x: the namespace errors() takes"""
    a = (lights, sh_n, d, x.w if weighted else None, alpha, eta, vis, spp)
    r = types.SimpleNamespace()
    r.image, r.value = forward(*a, dtype=dtype)
    r.dimage, r.dvalue = tangent(*a, dn=x.dn, dw=x.dw if weighted else None, da=x.da, d_lights=x.dl, dtype=dtype)
    g = adjoint(*a, grad_image=x.gi, grad_value=x.gv, dtype=dtype)
    r.gn, r.gw, r.ga, r.g4 = g.gn, g.gw if weighted else None, g.ga, g.g4
    return r

"""The projector row (include/hf.h hf_projector_rays, hf_projector_lighting, _adjoint, _tangent) restated in numpy the way
the reference computes it, NOT from the closed forms of the header.  steps() is Emitter::sample_direction of
src/emitters/projector.cpp:204-246 line by line -- camera_to_sample is the product of the matrices of
perspective_projection(size, size, 0, fov, 1e-4, 1e4) (sensor_ref.camera_to_sample), it_local comes from numpy.linalg.inv of
to_world, ds.d, ds.n and -dot(ds.n, ds.d) are formed as the reference forms them -- times the diffuse BSDF's albedo / pi
<sh_n, ds.d>, with the tangent as the chain rule through exactly those steps.  forward / tangent / adjoint are what the
header FREEZES: the same matrices and the same inverse for ref and uv, and the shading term written as G = <sh_n, c - p> /
ref.z^3.  For a scale-free to_world the two agree (tests/test_projector_ref.py: the primal, and the tangent in every
direction that keeps to_world rigid); for the other directions of the 12 unconstrained entries the header's convention is
hf_sensor_project's -- G differentiated as written -- and only forward / tangent / adjoint state it.  The adjoint is a
reverse sweep written on its own: it shares no line with the tangent.  Visibility is an input: nothing here traces.
float64 by default; `dtype=np.float32` evaluates the same text in float32 (scripts/projector_f32_error.py).  The bilinear
lookup is refract_ref's, the masks and the spawned origin sky_ref's, the box film refract_ref's.  A helper module."""
import types

import numpy as np

import refract_ref as R
import sensor_ref as SR
import sky_ref as S
from refract_ref import CLAMP, REPEAT, film, near_border, textures  # noqa: F401
from sensor_ref import err_abs, err_l2, look_at  # noqa: F401
from sky_ref import eligible  # noqa: F401

SHADOW_EPSILON = 10.0 * S.RAY_EPSILON  # math.h:22
# a mask is decided by the sign of <sh_n, -d>, of <sh_n, u> or of the distance of uv to 0 or 1; the kernel's quantities are
# within 2e-6 of the restatement's on the tests' scenes (|u| <= 2.5, ref.z >= 0.8, float32 inputs): a lane on which one of
# them is below this is decided by rounding and is left out of mask comparisons
MARGIN = 1e-5
# a lane whose texel coordinate lies within this of a border between two cells may read another cell after another
# rounding: its slopes are another cell's.  Such lanes are left out of the derivative comparisons (float32 moves a
# coordinate below 16 by 4e-6 at most)
BORDER = 1e-4
TEX = (16, 8)   # TW, TH
SCALE, ALBEDO = 1.5, 0.8
TARGET = (0.0, 0.0, 0.25)


def projector(to_world, fov, scale=1.0, res=TEX):
    m = np.asarray(to_world, np.float64).reshape(-1, 4)[:3]
    return types.SimpleNamespace(to_world=m, fov=float(fov), scale=float(np.float32(scale)), res=(int(res[0]), int(res[1])))


# the two projectors of the row's tests: one above the terrain whose frustum's border crosses it, one beside it whose light
# grazes the relief
PROJECTORS = {"above": lambda **kw: projector(look_at((0.3, -0.2, 2.0), TARGET, (0, 1, 0)), 40.0, SCALE, **kw),
              "side": lambda **kw: projector(look_at((1.8, 0.4, 0.7), (0, 0, 0.2), (0, 0, 1)), 50.0, SCALE, **kw)}


def _dot(a, b):
    return (a * b).sum(0)


def _sensor(pr):
    """the sensor whose camera_to_sample the projector's is: film = the texture's size, no crop, the clip planes of :148-150"""
    return SR.sensor(SR.PERSPECTIVE, pr.to_world, pr.fov, pr.res, None, 1e-4, 1e4)


def mapping(pr, p, dt=np.float64, dp=None, d_to_world=None, d_fov=None):
    """projector.cpp:209-214: it_local = to_world^-1 p (numpy.linalg.inv), uv = head<2>(camera_to_sample it_local), lit;
    and their tangents (zeros without one)"""
    p = np.asarray(p, dt)
    n = p.shape[1]
    T = np.eye(4, dtype=dt)
    T[:3] = pr.to_world.astype(dt)
    dT = np.zeros((4, 4), dt)
    dT[:3, :3], dT[:3, 3] = SR._split(d_to_world, dt)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    dp4 = np.concatenate([np.zeros((3, n), dt) if dp is None else np.asarray(dp, dt), np.zeros((1, n), dt)])
    ref4 = Ti @ p4
    dref4 = Ti @ dp4 - Ti @ dT @ ref4
    C, dC = SR.camera_to_sample(_sensor(pr), dt, d_fov)
    with np.errstate(all="ignore"):
        h = C @ ref4
        dh = dC @ ref4 + C @ dref4
        uv = h[:2] / h[3]
        duv = dh[:2] / h[3] - h[:2] * dh[3] / h[3] ** 2
        lit = (uv >= 0).all(0) & (uv <= 1).all(0) & (ref4[2] > 0)
        edge = np.minimum(np.abs(uv), np.abs(1 - uv)).min(0)
    return types.SimpleNamespace(ref=ref4[:3], dref=dref4[:3], uv=uv, duv=duv, lit=lit, edge=edge, T=T, dT=dT, Ti=Ti, p4=p4,
                                 ref4=ref4, C=C, h=h)


def texel(pr, m, tex, wrap, dt):
    """the lookup at (uv.x TW, uv.y TH); None without a texture (I = 1)"""
    if tex is None:
        return None
    with np.errstate(all="ignore"):
        return R.lookup(tex, np.stack([m.uv[0] * dt(pr.res[0]), m.uv[1] * dt(pr.res[1])]).astype(dt), wrap, dt)


def traced(pr, p, sh_n, d, t):
    """(traced [n], unsure [n]): an eligible sample is traced when it is lit, <sh_n, u> > 0 with u = c - p, and |u|^2 is
    finite and > 0; unsure: one of the deciding quantities is within MARGIN of its threshold"""
    el, c = eligible(sh_n, d, t)
    m = mapping(pr, p)
    u = pr.to_world[:, 3:4] - np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        cu, r2 = _dot(np.asarray(sh_n, np.float64), u), _dot(u, u)
        tr = el & m.lit & (cu > 0) & np.isfinite(r2) & (r2 > 0)
        hit = np.isfinite(np.asarray(t, np.float64))
        unsure = hit & ((c < MARGIN) | (el & (m.ref[2] > 0) & ((m.edge < MARGIN) | (m.lit & (np.abs(cu) < MARGIN)))))
    return tr, unsure


def rays(pr, p, nrm, sh_n, d, t):
    """the shadow ray of every sample, spawn_ray_to(c) (interaction.h:141-147): (o [3, n], direction [3, n], maxt [n],
    traced [n]); lanes that are not traced: zeros and maxt = -1"""
    tr, _ = traced(pr, p, sh_n, d, t)
    c = pr.to_world[:, 3:4].astype(np.float32).astype(np.float64)
    o = S.spawn_origin(p, nrm, c - np.asarray(p, np.float64))
    dv = c - o
    dist = np.sqrt(_dot(dv, dv))
    with np.errstate(all="ignore"):
        w = dv / dist
    return np.where(tr[None], o, 0.0), np.where(tr[None], w, 0.0), np.where(tr, dist * (1.0 - SHADOW_EPSILON), -1.0), tr


def steps(pr, p, sh_n, weight, tex, wrap, albedo, dt=np.float64, dn=None, dp=None, dw=None, dtex=None, d_to_world=None,
          d_fov=None, d_scale=None):
    """(value [n], dvalue [n], uv [2, n]) of EVERY lane, unmasked: sample_direction line by line times albedo / pi
    <sh_n, ds.d>, and the chain rule through the same lines"""
    f = lambda x, shape: np.zeros(shape, dt) if x is None else np.asarray(x, dt)
    p, sh_n = np.asarray(p, dt), np.asarray(sh_n, dt)
    n = p.shape[1]
    dn, dpp = f(dn, (3, n)), f(dp, (3, n))
    w, dw = (np.ones(n, dt) if weight is None else np.asarray(weight, dt)), f(dw, n)
    m = mapping(pr, p, dt, dp, d_to_world, d_fov)                       # :209-214
    e = texel(pr, m, tex, wrap, dt)                                     # :216-220
    I, dI = np.ones(n, dt), np.zeros(n, dt)
    if e is not None:
        I = e.L
        dI = e.Lx * dt(pr.res[0]) * m.duv[0] + e.Ly * dt(pr.res[1]) * m.duv[1]
        if dtex is not None:
            dI = dI + sum(e.b[j] * np.asarray(dtex, dt).ravel()[e.idx[j]] for j in range(4))
    A, dA = m.T[:3, :3], m.dT[:3, :3]
    ds_p, d_ds_p = m.T[:3, 3:4], m.dT[:3, 3:4]                          # :224
    ds_n, d_ds_n = A @ np.array([[0], [0], [1]], dt), dA @ np.array([[0], [0], [1]], dt)   # :225
    with np.errstate(all="ignore"):
        ds_d, d_ds_d = ds_p - p, d_ds_p - dpp                           # :231
        dist2 = _dot(ds_d, ds_d)                                        # :232
        dist = np.sqrt(dist2)                                           # :233
        ddist = _dot(ds_d, d_ds_d) / dist
        d_ds_d = d_ds_d / dist - ds_d * ddist / dist2                   # :234
        ds_d = ds_d / dist
        cosn = -_dot(ds_n, ds_d)                                        # :243
        dcosn = -(_dot(d_ds_n, ds_d) + _dot(ds_n, d_ds_d))
        z, dz = m.ref[2], m.dref[2]
        q = dt(1) / (z * z * cosn)                                      # :242-243
        dq = -q * (dt(2) * dz / z + dcosn / cosn)
        scale, dscale = dt(pr.scale), dt(0 if d_scale is None else d_scale)
        spec = dt(np.pi) * scale * I * q
        dspec = dt(np.pi) * (dscale * I * q + scale * dI * q + scale * I * dq)
        cs, dcs = _dot(sh_n, ds_d), _dot(dn, ds_d) + _dot(sh_n, d_ds_d)  # diffuse.cpp: albedo / pi cos_theta_o
        bs, dbs = dt(albedo) / dt(np.pi) * cs, dt(albedo) / dt(np.pi) * dcs
        value = w * spec * bs
        dvalue = dw * spec * bs + w * (dspec * bs + spec * dbs)
    return value, dvalue, m.uv


def _terms(pr, p, sh_n, weight, tex, wrap, albedo, vis, dt):
    """what forward, adjoint and tangent form of every sample: the mapping, the lookup, u = c - p and G = <sh_n, u> / z^3"""
    x = types.SimpleNamespace(dt=dt)
    x.p, x.sn = np.asarray(p, dt), np.asarray(sh_n, dt)
    x.n = x.p.shape[1]
    x.m = mapping(pr, x.p, dt)
    x.e = texel(pr, x.m, tex, wrap, dt)
    x.v = np.asarray(vis, bool) & x.m.lit
    x.u = pr.to_world[:, 3:4].astype(dt) - x.p
    with np.errstate(all="ignore"):
        x.z = x.m.ref[2]
        x.G = np.where(x.v, _dot(x.sn, x.u) / x.z ** 3, dt(0))
    x.I = np.ones(x.n, dt) if x.e is None else x.e.L
    x.w = np.ones(x.n, dt) if weight is None else np.asarray(weight, dt)
    x.cs = dt(albedo) * dt(pr.scale)
    return x


def forward(pr, p, sh_n, weight, tex, wrap, albedo, vis, spp=1, dtype=np.float64):
    """(image [n / spp], value [n], uv [2, n] with zeros where ref.z <= 0)"""
    x = _terms(pr, p, sh_n, weight, tex, wrap, albedo, vis, dtype)
    value = np.where(x.v, x.w * x.cs * x.I * x.G, dtype(0))
    with np.errstate(invalid="ignore"):
        uv = np.where(x.z > 0, x.m.uv, dtype(0))
    return film(value, spp), value, uv


def tangent(pr, p, sh_n, weight, tex, wrap, albedo, vis, spp=1, dn=None, dp=None, dw=None, dtex=None, d_to_world=None,
            d_fov=None, d_scale=None, dtype=np.float64):
    """(dimage [n / spp], dvalue [n]): the header's dG and dI with d ref and d uv from the matrices"""
    dt = dtype
    x = _terms(pr, p, sh_n, weight, tex, wrap, albedo, vis, dt)
    f = lambda a, shape: np.zeros(shape, dt) if a is None else np.asarray(a, dt)
    dn, dpp, dw = f(dn, (3, x.n)), f(dp, (3, x.n)), f(dw, x.n)
    m = mapping(pr, x.p, dt, dp, d_to_world, d_fov)
    dc = m.dT[:3, 3:4]
    with np.errstate(all="ignore"):
        dG = _dot(dn, x.u) / x.z ** 3 + _dot(x.sn, dc - dpp) / x.z ** 3 - 3 * _dot(x.sn, x.u) * m.dref[2] / x.z ** 4
        dI = np.zeros(x.n, dt)
        if x.e is not None:
            dI = x.e.Lx * dt(pr.res[0]) * m.duv[0] + x.e.Ly * dt(pr.res[1]) * m.duv[1]
            if dtex is not None:
                dI = dI + sum(x.e.b[j] * np.asarray(dtex, dt).ravel()[x.e.idx[j]] for j in range(4))
        dcs = dt(albedo) * dt(0 if d_scale is None else d_scale)
        dv = (dw * x.cs + x.w * dcs) * x.I * x.G + x.w * x.cs * (dI * x.G + x.I * dG)
    dv = np.where(x.v, dv, dt(0))
    return film(dv, spp), dv


def adjoint(pr, p, sh_n, weight, tex, wrap, albedo, vis, spp=1, grad_image=None, grad_value=None, dtype=np.float64, rows=None):
    """the reverse sweep: a namespace with gn, gp [3, n], gw [n], gtex [TH, TW] (None without a texture) and g14 = (dL/d
    to_world [12], dL/dfov, dL/dscale).  rows: a slice of the samples the sums g14 and gtex are taken over (None: all)"""
    dt = dtype
    x = _terms(pr, p, sh_n, weight, tex, wrap, albedo, vis, dt)
    g = np.zeros(x.n, dt)
    if grad_image is not None:
        g = g + np.repeat(np.asarray(grad_image, dt), spp) / dt(spp)
    if grad_value is not None:
        g = g + np.asarray(grad_value, dt)
    g = np.where(x.v, g, dt(0))
    keep = np.zeros(x.n, bool)
    keep[slice(None) if rows is None else rows] = True
    out = types.SimpleNamespace()
    m = x.m
    with np.errstate(all="ignore"):
        zero = lambda a: np.where(x.v, a, dt(0))
        # value = w cs I G
        out.gw = zero(g * x.cs * x.I * x.G)
        g_scale = (zero(g * x.w * dt(albedo) * x.I * x.G) * keep).sum()
        gI, gG = zero(g * x.w * x.cs * x.G), zero(g * x.w * x.cs * x.I)
        # G = <sn, u> / z^3, u = c - p
        iz3 = zero(dt(1) / x.z ** 3)
        out.gn = gG * iz3 * np.where(x.v, x.u, dt(0))
        g_u = np.where(x.v[None], gG * iz3 * x.sn, dt(0))
        g_z = zero(-3 * gG * _dot(x.sn, x.u) / x.z ** 4)
        # I = lookup(uv res)
        g_uv = np.zeros((2, x.n), dt)
        out.gtex = None
        if x.e is not None:
            g_uv = np.stack([gI * x.e.Lx * dt(pr.res[0]), gI * x.e.Ly * dt(pr.res[1])])
            gt = np.zeros(np.asarray(tex).size, dt)
            for j in range(4):
                np.add.at(gt, x.e.idx[j][keep], (gI * x.e.b[j])[keep])
            out.gtex = gt.reshape(np.asarray(tex).shape)
        # uv = h[:2] / h[3], h = C ref4; ref4 = T^-1 p4
        hs = np.where(x.v[None], m.h, dt(1))
        g_h = SR._unhom_back(hs, g_uv)
        g_ref4 = m.C.T @ np.where(x.v[None], g_h, dt(0))
        g_ref4[2] += g_z
        r4 = np.where(x.v[None], m.ref4, dt(0))
        gC = (np.where(x.v[None], g_h, dt(0)) * keep) @ r4.T
        gT = -m.Ti.T @ ((g_ref4 * keep) @ np.where(x.v[None], m.p4, dt(0)).T) @ m.Ti.T
        out.gp = np.where(x.v[None], (m.Ti.T @ g_ref4)[:3] - g_u, dt(0))
        g12 = gT[:3].copy()
        g12[:, 3] += (g_u * keep).sum(1)
    s = _sensor(pr)
    out.g14 = np.concatenate([g12.reshape(-1), [SR._fov_back(s, gC, SR._pre(s, dt), dt), g_scale]]).astype(dt)
    return out


def inputs(n, spp, tex_shape, seed=5):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(n // spp), gv=f(n), dn=f(3, n),
                                 dp=(0.2 * f(3, n)).astype(np.float32), dw=f(n), dtex=f(*tex_shape),
                                 dtw=(0.3 * f(12)).astype(np.float32), dfov=np.float32(0.7), dscale=np.float32(-0.4))


def steady(pr, p, vis):
    """vis without the lanes whose texel coordinate is within BORDER of a border between two cells of the lookup"""
    m = mapping(pr, p)
    with np.errstate(invalid="ignore"):
        pos = np.stack([m.uv[0] * pr.res[0], m.uv[1] * pr.res[1]])
    return np.asarray(vis, bool) & ~near_border(pos, BORDER)


def errors(got, ref, lanes):
    """the error measures scripts/projector_f32_error.py records and tests/test_gpu_projector.py holds the kernels to.  got,
    ref: namespaces with image, value, uv, dimage, dvalue, gn, gp, gw, gtex (or None), g14; lanes: where uv is compared
    (ref.z > 0)"""
    out = {"image": err_abs(got.image, ref.image), "value": err_abs(got.value, ref.value),
           "uv": float(np.abs(np.asarray(got.uv, np.float64) - ref.uv)[:, lanes].max()),
           "dimage": err_abs(got.dimage, ref.dimage), "dvalue": err_abs(got.dvalue, ref.dvalue),
           "grad_sh_n": err_abs(got.gn, ref.gn), "grad_p": err_abs(got.gp, ref.gp), "grad_weight": err_abs(got.gw, ref.gw),
           "grad14": err_l2(got.g14, ref.g14)}
    if ref.gtex is not None:
        out["grad_tex"] = err_l2(got.gtex, ref.gtex)
    return out


def evaluate(pr, rec, x, tex, wrap, vis, spp, dtype=np.float64, weighted=True):
    """forward, tangent and adjoint of the scene records rec (p, sh_n) under the inputs x: the namespace errors() takes"""
    a = (pr, rec["p"], rec["sh_n"], x.w if weighted else None, tex, wrap, ALBEDO, vis, spp)
    r = types.SimpleNamespace()
    r.image, r.value, r.uv = forward(*a, dtype=dtype)
    r.dimage, r.dvalue = tangent(*a, dn=x.dn, dp=x.dp, dw=x.dw if weighted else None, dtex=x.dtex if tex is not None else None,
                                 d_to_world=x.dtw, d_fov=x.dfov, d_scale=x.dscale, dtype=dtype)
    g = adjoint(*a, grad_image=x.gi, grad_value=x.gv, dtype=dtype)
    r.gn, r.gp, r.gw, r.gtex, r.g14 = g.gn, g.gp, g.gw, g.gtex, g.g14
    return r

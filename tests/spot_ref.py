"""The spot row (include/hf.h hf_spot_rays, hf_spot_lighting, _adjoint, _tangent) restated in numpy the way the reference
computes it.  steps() is SpotLight::sample_direction of src/emitters/spot.cpp:177-212 line by line -- ds.d normalised,
local_d = to_world^-1 (-ds.d) through numpy.linalg.inv, falloff_curve (:143-151) with acos of local_d.z, spec = intensity
falloff / dist^2 -- times the diffuse BSDF's albedo / pi <sh_n, ds.d> (diffuse.cpp:135-140).  forward / tangent / adjoint
are what the header FREEZES: ref = A^-1 (p - c), theta = atan2(hypot(ref.x, ref.y), ref.z), the shading term written as
<sh_n, u> / |u|^3, and the 12 entries of to_world unconstrained (hf_projector_lighting's convention: ref differentiated as
written).  For a scale-free to_world the two agree (tests/test_spot_ref.py).  The adjoint is a reverse sweep written on its
own: it shares no line with the tangent.  Visibility is an input, [K, n] booleans (bit k of the kernel's byte): nothing
here traces.  float64 by default; `dtype=np.float32` evaluates the same text in float32 (scripts/spot_f32_error.py).  The
masks and the spawned origin are sky_ref's, the shadow ray projector_ref's, the box film refract_ref's.  A helper module."""
import types

import numpy as np

import projector_ref as PR
import sky_ref as S
from refract_ref import film  # noqa: F401
from sensor_ref import err_abs, err_l2, look_at  # noqa: F401
from sky_ref import eligible  # noqa: F401

# a mask is decided by the sign of <sh_n, -d>, of <sh_n, u>, of cos(theta) - cos(cutoff) or of cutoff - theta; the kernel's
# quantities are within 2e-6 of the restatement's on the tests' scenes (|u| <= 2.6, float32 inputs, the mapping in double
# on both sides): a lane on which one of them is below this is decided by rounding and is left out of mask comparisons
MARGIN = 1e-5
# the slope of the falloff jumps at theta = beam: lanes within this many radians of it have their bit for that light cleared
# in the visibility that the derivative kernels and the restatement are given (float32 moves theta by 4e-7 at most)
KINK = 1e-4
PARAMS = 15     # to_world[12], intensity, cutoff_angle, beam_width
ALBEDO = 0.8
TARGET = (0.0, 0.0, 0.25)


def light(to_world, intensity=1.0, cutoff=20.0, beam=None):
    """the angles and the intensity as the float32 values hf_spot_light_t holds"""
    m = np.asarray(to_world, np.float64).reshape(-1, 4)[:3]
    beam = 0.75 * cutoff if beam is None else beam
    return types.SimpleNamespace(to_world=m, intensity=float(np.float32(intensity)), cutoff=float(np.float32(cutoff)),
                                 beam=float(np.float32(beam)))


# the rig of the row's tests: name -> (origin, target, up, cutoff, beam, intensity)
RIG = {"above": ((0.3, -0.2, 2.0), TARGET, (0, 1, 0), 20, 15, 3.0),
       "side": ((1.8, 0.4, 0.7), (0, 0, 0.2), (0, 0, 1), 35, 10, 2.5),
       "wide": ((-0.8, -0.9, 1.1), TARGET, (0, 0, 1), 100, 60, 1.5),
       "hard": ((-1.2, 0.9, 0.9), TARGET, (0, 0, 1), 30, 30, 2.0),
       "point": ((0.2, 0.6, 0.8), TARGET, (0, 0, 1), 180, 180, 1.0),
       "graze": ((0, -2.2, 0.45), TARGET, (0, 0, 1), 25, 5, 4.0),
       "near": ((0.4, 0.1, 0.62), (0.1, 0, 0.25), (0, 1, 0), 60, 45, 0.5),
       "back": ((-1.5, -0.2, 1.6), TARGET, (0, 0, 1), 28, 21, 3.5)}
NAMES = tuple(RIG)


def rig(names=NAMES):
    return [light(look_at(*RIG[k][:3]), RIG[k][5], RIG[k][3], RIG[k][4]) for k in names]


def row15(L):
    return np.concatenate([L.to_world.reshape(-1), [L.intensity, L.cutoff, L.beam]])


def _dot(a, b):
    return (a * b).sum(0)


def mapping(L, p, dt=np.float64, dp=None, d15=None):
    """ref = A^-1 (p - c) (numpy.linalg.inv of the 4x4), cos(theta), theta = atan2(rho, ref.z), the cone, the full beam, the
    falloff of the branch the point is on, and their tangents for dp and a row d15 of the light's 15 numbers (zeros
    without); angles' tangents per degree"""
    p = np.asarray(p, dt)
    n = p.shape[1]
    d15 = np.zeros(PARAMS, dt) if d15 is None else np.asarray(d15, dt)
    T, dT = np.eye(4, dtype=dt), np.zeros((4, 4), dt)
    T[:3] = L.to_world.astype(dt)
    dT[:3] = d15[:12].reshape(3, 4)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    dp4 = np.concatenate([np.zeros((3, n), dt) if dp is None else np.asarray(dp, dt), np.zeros((1, n), dt)])
    ref = (Ti @ p4)[:3]
    dref = (Ti @ dp4 - Ti @ dT @ (Ti @ p4))[:3]
    rad = dt(np.pi) / dt(180)
    cut, beam = dt(L.cutoff) * rad, dt(L.beam) * rad
    dcut, dbeam = d15[13] * rad, d15[14] * rad
    m = types.SimpleNamespace(ref=ref, dref=dref, Ti=Ti, p4=p4, cut=cut, beam=beam)
    with np.errstate(all="ignore"):
        m.r2 = _dot(ref, ref)
        m.rho = np.sqrt(ref[0] * ref[0] + ref[1] * ref[1])
        m.cos = ref[2] / np.sqrt(m.r2)
        m.theta = np.arctan2(m.rho, ref[2])
        m.cone = m.cos > np.cos(cut)
        m.full = m.cos >= np.cos(beam)
        drho = (ref[0] * dref[0] + ref[1] * dref[1]) / m.rho
        m.dtheta = (ref[2] * drho - m.rho * dref[2]) / m.r2
        if L.cutoff > L.beam:
            ramp = (cut - m.theta) / (cut - beam)
            dramp = ((dcut - m.dtheta) - ramp * (dcut - dbeam)) / (cut - beam)
        else:                                           # a hard edge: no zone, nothing divides by the zero width
            ramp, dramp = np.zeros(n, dt), np.zeros(n, dt)
        m.f = np.where(m.full, dt(1), ramp)
        m.df = np.where(m.full, dt(0), dramp)
        m.lit = m.cone & (m.f > 0)
        m.zone = m.cone & ~m.full
    return m


def traced(L, p, sh_n, d, t):
    """(traced [n], unsure [n]): an eligible sample is traced when f > 0, <sh_n, u> > 0 with u = c - p, and |u|^2 is finite
    and > 0; unsure: one of the deciding quantities is within MARGIN of its threshold"""
    el, c = eligible(sh_n, d, t)
    m = mapping(L, p)
    u = L.to_world[:, 3:4] - np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        cu, r2 = _dot(np.asarray(sh_n, np.float64), u), _dot(u, u)
        tr = el & m.lit & (cu > 0) & np.isfinite(r2) & (r2 > 0)
        hit = np.isfinite(np.asarray(t, np.float64))
        edge = np.minimum(np.abs(m.cos - np.cos(m.cut)), np.abs(m.cut - m.theta))
        unsure = hit & ((c < MARGIN) | (el & ((edge < MARGIN) | (m.lit & (np.abs(cu) < MARGIN)))))
    return tr, unsure


def rays(L, p, nrm, sh_n, d, t):
    """the shadow ray of every sample, spawn_ray_to(c): projector_ref.rays' text with this row's traced"""
    tr, _ = traced(L, p, sh_n, d, t)
    c = L.to_world[:, 3:4].astype(np.float32).astype(np.float64)
    o = S.spawn_origin(p, nrm, c - np.asarray(p, np.float64))
    dv = c - o
    dist = np.sqrt(_dot(dv, dv))
    with np.errstate(all="ignore"):
        w = dv / dist
    return np.where(tr[None], o, 0.0), np.where(tr[None], w, 0.0), np.where(tr, dist * (1.0 - PR.SHADOW_EPSILON), -1.0), tr


def steps(L, p, sh_n, weight, albedo, dt=np.float64):
    """value [n] of EVERY lane, unmasked but for the falloff: sample_direction line by line times albedo / pi <sh_n, ds.d>"""
    p, sh_n = np.asarray(p, dt), np.asarray(sh_n, dt)
    w = np.ones(p.shape[1], dt) if weight is None else np.asarray(weight, dt)
    T = np.eye(4, dtype=dt)
    T[:3] = L.to_world.astype(dt)
    with np.errstate(all="ignore"):
        ds_p = T[:3, 3:4]                                               # :183
        ds_d = ds_p - p                                                 # :189
        dist2 = _dot(ds_d, ds_d)                                        # :190
        dist = np.sqrt(dist2)
        inv_dist = dt(1) / dist                                         # :191
        ds_d = ds_d * inv_dist                                          # :192
        local_d = np.linalg.inv(T)[:3, :3] @ -ds_d                      # :193
        cos_theta = local_d[2]                                          # falloff_curve, :143-151
        cut, beam = dt(np.deg2rad(L.cutoff)), dt(np.deg2rad(L.beam))
        inv_width = dt(1) / (cut - beam) if L.cutoff > L.beam else dt(0)
        beam_res = np.where(cos_theta >= np.cos(beam), dt(1), (cut - np.arccos(np.clip(cos_theta, -1, 1))) * inv_width)
        falloff = np.where(cos_theta > np.cos(cut), beam_res, dt(0))
        falloff = np.where(falloff > 0, falloff, dt(0))                 # :198
        spec = dt(L.intensity) * falloff * inv_dist * inv_dist          # :206
        bs = dt(albedo) / dt(np.pi) * _dot(sh_n, ds_d)                  # diffuse.cpp: albedo / pi cos_theta_o
    return w * spec * bs


def _terms(L, p, sh_n, weight, albedo, vis, dt):
    """what forward, adjoint and tangent form of every sample under one light"""
    x = types.SimpleNamespace(dt=dt)
    x.p, x.sn = np.asarray(p, dt), np.asarray(sh_n, dt)
    x.n = x.p.shape[1]
    x.m = mapping(L, x.p, dt)
    x.u = L.to_world[:, 3:4].astype(dt) - x.p
    with np.errstate(all="ignore"):
        x.S, x.r2 = _dot(x.sn, x.u), _dot(x.u, x.u)
        x.v = np.asarray(vis, bool) & (x.r2 > 0) & (x.m.r2 > 0) & (x.m.full | (x.m.rho > 0))
        x.r3 = x.r2 * np.sqrt(x.r2)
        x.G = np.where(x.v, x.S / x.r3, dt(0))
        x.f = np.where(x.v, x.m.f, dt(0))
    x.w = np.ones(x.n, dt) if weight is None else np.asarray(weight, dt)
    x.ap = dt(albedo) / dt(np.pi)
    x.ci = x.ap * dt(L.intensity)
    return x


def forward(lights, p, sh_n, weight, albedo, vis, spp=1, dtype=np.float64):
    """(image [K, n / spp], value [K, n])"""
    value = []
    for L, v in zip(lights, vis):
        x = _terms(L, p, sh_n, weight, albedo, v, dtype)
        value.append(np.where(x.v, x.w * x.ci * x.f * x.G, dtype(0)))
    value = np.stack(value)
    return np.stack([film(v, spp) for v in value]), value


def tangent(lights, p, sh_n, weight, albedo, vis, spp=1, dn=None, dp=None, dw=None, d_lights=None, dtype=np.float64):
    """(dimage [K, n / spp], dvalue [K, n]) for the tangents dn, dp [3, n], dw [n], d_lights [K, 15] (None: zero)"""
    dt = dtype
    out = []
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, p, sh_n, weight, albedo, v, dt)
        z = lambda a, shape: np.zeros(shape, dt) if a is None else np.asarray(a, dt)
        dnn, dpp, dww = z(dn, (3, x.n)), z(dp, (3, x.n)), z(dw, x.n)
        d15 = np.zeros(PARAMS, dt) if d_lights is None else np.asarray(d_lights, dt)[k]
        m = mapping(L, x.p, dt, dp, d15)
        du = d15[:12].reshape(3, 4)[:, 3:4] - dpp
        with np.errstate(all="ignore"):
            dG = _dot(dnn, x.u) / x.r3 + _dot(x.sn, du) / x.r3 - 3 * x.S * _dot(x.u, du) / (x.r3 * x.r2)
            dv = (dww * x.ci + x.w * x.ap * d15[12]) * x.f * x.G + x.w * x.ci * (m.df * x.G + x.f * dG)
        out.append(np.where(x.v, dv, dt(0)))
    out = np.stack(out)
    return np.stack([film(v, spp) for v in out]), out


def adjoint(lights, p, sh_n, weight, albedo, vis, spp=1, grad_image=None, grad_value=None, dtype=np.float64, rows=None):
    """the reverse sweep: a namespace with gn, gp [3, n], gw [n] (the lights summed) and g15 [K, 15] (angles per degree).
    rows: a slice of the samples the sums g15 are taken over (None: all)"""
    dt = dtype
    K = len(lights)
    out = types.SimpleNamespace(g15=np.zeros((K, PARAMS), dt))
    rad = dt(np.pi) / dt(180)
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, p, sh_n, weight, albedo, v, dt)
        if k == 0:
            out.gn, out.gp, out.gw = np.zeros((3, x.n), dt), np.zeros((3, x.n), dt), np.zeros(x.n, dt)
        keep = np.zeros(x.n, bool)
        keep[slice(None) if rows is None else rows] = True
        g = np.zeros(x.n, dt)
        if grad_image is not None:
            g = g + np.repeat(np.asarray(grad_image, dt)[k], spp) / dt(spp)
        if grad_value is not None:
            g = g + np.asarray(grad_value, dt)[k]
        g = np.where(x.v, g, dt(0))
        m = x.m
        with np.errstate(all="ignore"):
            zero = lambda a: np.where(x.v, a, dt(0))
            # value = w ci f G
            out.gw += zero(g * x.ci * x.f * x.G)
            g_int = (zero(g * x.w * x.ap * x.f * x.G) * keep).sum()
            gf, gG = zero(g * x.w * x.ci * x.G), zero(g * x.w * x.ci * x.f)
            # G = S / r^3, S = <sn, u>, r^2 = <u, u>, u = c - p
            gS, g_r2 = zero(gG / x.r3), zero(-1.5 * gG * x.S / (x.r3 * x.r2))
            out.gn += np.where(x.v[None], gS * x.u, dt(0))
            g_u = np.where(x.v[None], gS * x.sn + 2 * g_r2 * x.u, dt(0))
            # f = (cut - theta) / (cut - beam) in the zone
            zone = x.v & ~m.full
            if L.cutoff > L.beam:
                width = m.cut - m.beam
                g_theta = np.where(zone, -gf / width, dt(0))
                g_cut = (np.where(zone, gf * (1 - x.f) / width, dt(0)) * keep).sum()
                g_beam = (np.where(zone, gf * x.f / width, dt(0)) * keep).sum()
            else:
                g_theta, g_cut, g_beam = np.zeros(x.n, dt), dt(0), dt(0)
            # theta = atan2(rho, z): d theta / d rho = z / r2, d theta / dz = -rho / r2; rho = hypot(x, y)
            g_rho = np.where(zone, g_theta * m.ref[2] / m.r2, dt(0))
            g_ref = np.stack([np.where(zone, g_rho * m.ref[0] / m.rho, dt(0)), np.where(zone, g_rho * m.ref[1] / m.rho, dt(0)),
                              np.where(zone, -g_theta * m.rho / m.r2, dt(0))])
            # ref4 = T^-1 p4
            g_ref4 = np.concatenate([g_ref, np.zeros((1, x.n), dt)])
            gT = -m.Ti.T @ ((g_ref4 * keep) @ np.where(x.v[None], m.p4, dt(0)).T) @ m.Ti.T
            out.gp += np.where(x.v[None], (m.Ti.T @ g_ref4)[:3] - g_u, dt(0))
            g12 = gT[:3].copy()
            g12[:, 3] += (g_u * keep).sum(1)
        out.g15[k] = np.concatenate([g12.reshape(-1), [g_int, g_cut * rad, g_beam * rad]])
    return out


def inputs(n, spp, K, seed=5):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    dl = (0.3 * f(K, PARAMS)).astype(np.float32)
    dl[:, 13:] = f(K, 2)                # (degrees)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(K, n // spp), gv=f(K, n), dn=f(3, n),
                                 dp=(0.2 * f(3, n)).astype(np.float32), dw=f(n), dl=dl)


def steady(L, p, vis):
    """vis without the lanes within KINK of theta = beam, where the slope of the falloff jumps (none for a hard edge and
    for beam = 180, where no zone is reached)"""
    m = mapping(L, p)
    with np.errstate(invalid="ignore"):
        return np.asarray(vis, bool) & ~(np.abs(m.theta - m.beam) < KINK)


def unpack(byte, K):
    """the kernel's visibility byte as [K, n] booleans"""
    b = np.asarray(byte, np.uint8)
    return np.stack([(b >> k) & 1 for k in range(K)]).astype(bool)


def pack(vis):
    return sum((np.asarray(v, np.uint8) << k) for k, v in enumerate(vis)).astype(np.uint8)


def errors(got, ref):
    """the error measures scripts/spot_f32_error.py records and tests/test_gpu_spot.py holds the kernels to.  got, ref:
    namespaces with image, value, dimage, dvalue, gn, gp, gw (or None), g15"""
    out = {"image": err_abs(got.image, ref.image), "value": err_abs(got.value, ref.value),
           "dimage": err_abs(got.dimage, ref.dimage), "dvalue": err_abs(got.dvalue, ref.dvalue),
           "grad_sh_n": err_abs(got.gn, ref.gn), "grad_p": err_abs(got.gp, ref.gp), "grad15": err_l2(got.g15, ref.g15)}
    if ref.gw is not None and got.gw is not None:
        out["grad_weight"] = err_abs(got.gw, ref.gw)
    return out


def evaluate(lights, rec, x, vis, spp, dtype=np.float64, weighted=True):
    """forward, tangent and adjoint of the scene records rec (p, sh_n) under the inputs x: the namespace errors() takes"""
    a = (lights, rec["p"], rec["sh_n"], x.w if weighted else None, ALBEDO, vis, spp)
    r = types.SimpleNamespace()
    r.image, r.value = forward(*a, dtype=dtype)
    r.dimage, r.dvalue = tangent(*a, dn=x.dn, dp=x.dp, dw=x.dw if weighted else None, d_lights=x.dl, dtype=dtype)
    g = adjoint(*a, grad_image=x.gi, grad_value=x.gv, dtype=dtype)
    r.gn, r.gp, r.gw, r.g15 = g.gn, g.gp, g.gw if weighted else None, g.g15
    return r


# ---- the GPU test's scenes on the CPU: the oracle's records and visibility (scripts/spot_f32_error.py, tests/test_spot_ref.py) ----
ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
SPP = 4


def oracle_scenes(film=(64, 64, SPP)):
    """yields (key, rec, rays, t, field) for the four scenes: sine_heights(96), max_height 0.5, the orthographic wavefront
    from the two origins, flat and smooth shading normals; rec holds p, n, sh_n as float32"""
    import hf_amd
    import lighting_scenes as LS
    from oracle import hf_oracle as O
    O.build()
    h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
    f = O.OracleField(h, max_height=0.5)
    for origin in ORIGINS:
        r = hf_amd.workload.ortho_rays(*film, "cpu", seed=1, origin=origin, target=TARGET, scale=(0.9, 0.9, 1.0)).numpy()
        t, u, v, prim = f.ray_intersect_preliminary(r)
        rec = f.compute_surface_interaction(r, t, u, v, prim, O.RAY_ALL)
        sc = types.SimpleNamespace(h64=h.astype(np.float64), max_height=0.5, to_world=LS.IDENTITY, flip=False)
        smooth = LS.smooth_normals(sc, r, prim, np.isfinite(t)).astype(np.float32)
        for mode, sh in (("face", rec["sh_n"]), ("smooth", smooth)):
            yield "origin %s, %s normals" % (origin, mode), {"p": rec["p"], "n": rec["n"], "sh_n": sh}, r, t, f


def probe(L, rec, r, t, field):
    """one light on one scene through the oracle: a namespace with el, tr, unsure, occ, vis, kink [n] and the shares"""
    q = types.SimpleNamespace()
    q.el, _ = eligible(rec["sh_n"], r[3:6], t)
    q.tr, q.unsure = traced(L, rec["p"], rec["sh_n"], r[3:6], t)
    o, w, maxt, _ = rays(L, rec["p"], rec["n"], rec["sh_n"], r[3:6], t)
    rows = np.concatenate([o, w, maxt[None]]).astype(np.float32)
    q.occ = np.zeros(len(t), bool)
    q.occ[q.tr] = field.ray_test(rows[:, q.tr]).astype(bool)
    q.vis = q.tr & ~q.occ
    m = mapping(L, rec["p"])
    q.kink = q.vis & ~steady(L, rec["p"], q.vis)
    q.shares = {"in_cone_of_eligible": float(m.cone[q.el].mean()), "zone_of_traced": float(m.zone[q.tr].mean()),
                "occluded_of_traced": float(q.occ[q.tr].mean()), "traced_of_eligible": float(q.tr[q.el].mean()),
                "unsure_share": float(q.unsure.mean()), "kink_share": float(q.kink.mean())}
    return q


def assert_shares(shares, unsure_union):
    """what tests/test_spot_ref.py and tests/test_gpu_spot.py assert on the restatement before comparing anything; shares:
    name -> the dict of probe() (or the same keys from the GPU's visibility)"""
    from row_helpers import UNSURE_CAP
    assert unsure_union <= UNSURE_CAP, unsure_union
    assert 0.15 <= shares["above"]["in_cone_of_eligible"] <= 0.95, shares["above"]
    for k in ("side", "graze"):
        assert 0.3 <= shares[k]["occluded_of_traced"] <= 0.9, (k, shares[k])
    for k in ("side", "graze", "above"):
        assert shares[k]["zone_of_traced"] >= 0.3, (k, shares[k])
    for k in ("hard", "point"):
        assert shares[k]["zone_of_traced"] == 0, (k, shares[k])

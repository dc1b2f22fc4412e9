"""The directional row (include/hf.h hf_directional_rays, hf_directional_lighting, _adjoint, _tangent) restated in numpy.
The value is DirectionalEmitter::sample_direction (src/emitters/directional.cpp:150-177: ds.d = -direction, spec =
irradiance) times the diffuse BSDF's albedo / pi <sh_n, ds.d> (diffuse.cpp:135-140), with the direction given as
to_light = -direction of any length: l = to_light / |to_light|.  forward / tangent / adjoint are what the header FREEZES;
differentiating to_light goes beyond the reference (directional.cpp:96 keeps to_world non-differentiable), so its
yardstick is this text and the central differences of tests/test_directional_ref.py.  The adjoint is a reverse sweep
written on its own: it shares no line with the tangent.  Visibility is an input, [K, n] booleans (bit k of the kernel's
byte): nothing here traces.  float64 by default; `dtype=np.float32` evaluates the same text in float32
(scripts/directional_f32_error.py).  The masks and the spawned origin are sky_ref's, the box film refract_ref's, the
scenes spot_ref's.  A helper module."""
import types

import numpy as np

import sky_ref as S
from refract_ref import film  # noqa: F401
from sensor_ref import err_abs, err_l2  # noqa: F401
from sky_ref import eligible  # noqa: F401
from spot_ref import ORIGINS, SPP, oracle_scenes, pack, unpack  # noqa: F401

# a mask is decided by the sign of <sh_n, -d> or of <sh_n, l>, formed in float32 from float32 inputs of length about 1: a
# lane on which one of them is below this is decided by rounding and is left out of mask and value comparisons
MARGIN = 1e-5
PARAMS = 4      # to_light[3], irradiance
ALBEDO = 0.8


def light(to_light, irradiance=1.0):
    """to_light as the doubles and the irradiance as the float32 value hf_directional_light_t holds"""
    return types.SimpleNamespace(to_light=np.asarray(to_light, np.float64).reshape(3), irradiance=float(np.float32(irradiance)))


def from_direction(direction, irradiance=1.0):
    """the reference's `direction` property: the light travels along it"""
    return light(-np.asarray(direction, np.float64), irradiance)


# the rig of the row's tests: name -> (to_light, deliberately not unit; irradiance, all distinct)
RIG = {"zenith": ((0, 0, 1), 3.0),
       "high": ((0.3, 0.2, 0.9), 2.5),
       "low_x": ((1, 0.1, 0.25), 1.5),
       "low_y": ((-0.2, -1, 0.2), 2.0),
       "graze": ((-1, 0.3, 0.08), 4.0),
       "diag": ((0.7, -0.7, 0.35), 1.0),
       "below": ((0.3, 0.1, -0.6), 0.5),
       "unnorm": ((2, 1, 1.5), 3.5)}
NAMES = tuple(RIG)


def rig(names=NAMES):
    return [light(*RIG[k]) for k in names]


def row4(L):
    return np.append(L.to_light, L.irradiance)


def _dot(a, b):
    return (a * b).sum(0)


def unit(L, dt=np.float64):
    """(l [3], |to_light|): the host's normalisation, in double whatever dt is (the kernels are handed l in double)"""
    length = np.sqrt(_dot(L.to_light, L.to_light))
    return (L.to_light / length).astype(dt), dt(length)


def traced(L, sh_n, d, t):
    """(traced [n], unsure [n]): an eligible sample is traced when <sh_n, l> > 0; unsure: one of the two deciding
    quantities of a hit is within MARGIN of zero"""
    el, c = eligible(sh_n, d, t)
    l, _ = unit(L)
    co = _dot(np.asarray(sh_n, np.float64), l[:, None])
    hit = np.isfinite(np.asarray(t, np.float64))
    return el & (co > 0), hit & ((c < MARGIN) | (el & (np.abs(co) < MARGIN)))


def rays(L, p, nrm, sh_n, d, t):
    """the shadow ray of every sample, si.spawn_ray(l): (o [3, n], d [3, n], maxt [n], traced [n]); the direction is l
    rounded to float32, an untraced lane has a zero origin and direction and maxt = -1"""
    tr, _ = traced(L, sh_n, d, t)
    lf = unit(L)[0].astype(np.float32).astype(np.float64)[:, None]
    o = S.spawn_origin(p, nrm, lf)
    n = len(tr)
    return np.where(tr[None], o, 0.0), np.where(tr[None], np.repeat(lf, n, 1), 0.0), np.where(tr, np.inf, -1.0), tr


def _terms(L, sh_n, weight, albedo, vis, dt):
    """what forward, adjoint and tangent form of every sample under one light"""
    x = types.SimpleNamespace(dt=dt)
    x.sn = np.asarray(sh_n, dt)
    x.n = x.sn.shape[1]
    x.l, x.len = unit(L, dt)
    x.S = _dot(x.sn, x.l[:, None])
    x.v = np.asarray(vis, bool)
    x.w = np.ones(x.n, dt) if weight is None else np.asarray(weight, dt)
    x.ap = dt(albedo) / dt(np.pi)
    x.ce = x.ap * dt(L.irradiance)
    return x


def forward(lights, sh_n, weight, albedo, vis, spp=1, dtype=np.float64):
    """(image [K, n / spp], value [K, n])"""
    value = []
    for L, v in zip(lights, vis):
        x = _terms(L, sh_n, weight, albedo, v, dtype)
        value.append(np.where(x.v, x.w * x.ce * x.S, dtype(0)))
    value = np.stack(value)
    return np.stack([film(v, spp) for v in value]), value


def tangent(lights, sh_n, weight, albedo, vis, spp=1, dn=None, dw=None, d_lights=None, dtype=np.float64):
    """(dimage [K, n / spp], dvalue [K, n]) for the tangents dn [3, n], dw [n], d_lights [K, 4] (None: zero)"""
    dt = dtype
    out = []
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, sh_n, weight, albedo, v, dt)
        z = lambda a, shape: np.zeros(shape, dt) if a is None else np.asarray(a, dt)
        dnn, dww = z(dn, (3, x.n)), z(dw, x.n)
        d4 = np.zeros(PARAMS, dt) if d_lights is None else np.asarray(d_lights, dt)[k]
        dv3, dE = d4[:3], d4[3]
        dl = (dv3 - x.l * _dot(x.l, dv3)) / x.len
        dval = x.ap * (dww * dt(L.irradiance) * x.S + x.w * dE * x.S
                       + x.w * dt(L.irradiance) * (_dot(dnn, x.l[:, None]) + _dot(x.sn, dl[:, None])))
        out.append(np.where(x.v, dval, dt(0)))
    out = np.stack(out)
    return np.stack([film(v, spp) for v in out]), out


def adjoint(lights, sh_n, weight, albedo, vis, spp=1, grad_image=None, grad_value=None, dtype=np.float64, rows=None):
    """the reverse sweep: a namespace with gn [3, n], gw [n] (the lights summed in light order) and g4 [K, 4].  rows: a
    slice of the samples the sums g4 are taken over (None: all)"""
    dt = dtype
    K = len(lights)
    out = types.SimpleNamespace(g4=np.zeros((K, PARAMS), dt))
    for k, (L, v) in enumerate(zip(lights, vis)):
        x = _terms(L, sh_n, weight, albedo, v, dt)
        if k == 0:
            out.gn, out.gw = np.zeros((3, x.n), dt), np.zeros(x.n, dt)
        keep = np.zeros(x.n, bool)
        keep[slice(None) if rows is None else rows] = True
        g = np.zeros(x.n, dt)
        if grad_image is not None:
            g = g + np.repeat(np.asarray(grad_image, dt)[k], spp) / dt(spp)
        if grad_value is not None:
            g = g + np.asarray(grad_value, dt)[k]
        g = np.where(x.v, g, dt(0))
        # value = w ce S, ce = ap E, S = <sn, l>, l = v / |v|
        out.gw += g * x.ce * x.S
        gS = g * x.w * x.ce
        out.gn += gS[None] * x.l[:, None]
        g_l = (x.sn * (gS * keep)[None]).sum(1)                  # dL/dl, as if l were free
        g_v = (g_l - x.l * _dot(x.l, g_l)) / x.len                # through the normalisation: the part orthogonal to l
        g_E = (g * x.w * x.ap * x.S * keep).sum()
        out.g4[k] = np.append(g_v, g_E)
    return out


def inputs(n, spp, K, seed=5):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(K, n // spp), gv=f(K, n), dn=f(3, n),
                                 dw=f(n), dl=(0.3 * f(K, PARAMS)).astype(np.float32))


def errors(got, ref):
    """the error measures scripts/directional_f32_error.py records and tests/test_gpu_directional.py holds the kernels
    to.  got, ref: namespaces with image, value, dimage, dvalue, gn, gw (or None), g4.  Per-lane quantities: the largest
    difference over max(1, largest value); the reduced rows: relative L2"""
    out = {"image": err_abs(got.image, ref.image), "value": err_abs(got.value, ref.value),
           "dimage": err_abs(got.dimage, ref.dimage), "dvalue": err_abs(got.dvalue, ref.dvalue),
           "grad_sh_n": err_abs(got.gn, ref.gn), "grad4": err_l2(got.g4, ref.g4)}
    if ref.gw is not None and got.gw is not None:
        out["grad_weight"] = err_abs(got.gw, ref.gw)
    return out


def evaluate(lights, rec, x, vis, spp, dtype=np.float64, weighted=True):
    """forward, tangent and adjoint of the scene records rec (sh_n) under the inputs x: the namespace errors() takes"""
    a = (lights, rec["sh_n"], x.w if weighted else None, ALBEDO, vis, spp)
    r = types.SimpleNamespace()
    r.image, r.value = forward(*a, dtype=dtype)
    r.dimage, r.dvalue = tangent(*a, dn=x.dn, dw=x.dw if weighted else None, d_lights=x.dl, dtype=dtype)
    g = adjoint(*a, grad_image=x.gi, grad_value=x.gv, dtype=dtype)
    r.gn, r.gw, r.g4 = g.gn, g.gw if weighted else None, g.g4
    return r


# ---- the GPU test's scenes on the CPU: spot_ref.oracle_scenes' records, this row's visibility through the oracle ----
def probe(L, rec, r, t, field):
    """one light on one scene through the oracle: a namespace with el, tr, unsure, occ, vis [n] and the shares"""
    q = types.SimpleNamespace()
    q.el, _ = eligible(rec["sh_n"], r[3:6], t)
    q.tr, q.unsure = traced(L, rec["sh_n"], r[3:6], t)
    o, w, maxt, _ = rays(L, rec["p"], rec["n"], rec["sh_n"], r[3:6], t)
    rows = np.concatenate([o, w, maxt[None]]).astype(np.float32)
    q.occ = np.zeros(len(t), bool)
    q.occ[q.tr] = field.ray_test(rows[:, q.tr]).astype(bool)
    q.vis = q.tr & ~q.occ
    q.shares = shares(q.el, q.tr, q.vis)
    return q


def shares(el, tr, vis):
    return {"traced_of_eligible": float(tr[el].mean()), "occluded_of_traced": float((tr & ~vis)[tr].mean())}


def assert_shares(sh, unsure_union):
    """what tests/test_directional_ref.py and tests/test_gpu_directional.py assert before comparing anything; sh: name ->
    the dict of shares()"""
    from row_helpers import UNSURE_CAP
    assert unsure_union <= UNSURE_CAP, unsure_union
    assert sh["zenith"]["traced_of_eligible"] == 1.0 and sh["zenith"]["occluded_of_traced"] == 0, sh["zenith"]
    for k in ("low_x", "low_y", "graze", "diag"):
        assert 0.3 <= sh[k]["occluded_of_traced"] <= 0.9, (k, sh[k])
    assert 0.15 <= sh["below"]["traced_of_eligible"] <= 0.5, sh["below"]

"""The medium row (include/hf.h hf_medium_rays, hf_medium_lighting, _adjoint, _tangent) restated in float64 numpy: the
segment of a primary ray inside the half space below the top plane, the draws (distance sampling in proportion to the
transmittance, medium.cpp:71, truncated to the segment and normalised), the shadow rays that start in free space, the
value (homogeneous.cpp:139-175: sigma_s = albedo sigma_t; hg.cpp:66-69, 99: wi = -d, wo = l), its adjoint and its
tangent.  forward / tangent / adjoint are what the header FREEZES: the bits and the branch of the segment are held.  The
adjoint is a reverse sweep written on its own: it shares no line with the tangent.  Visibility is an input, [J, n]
uint32 words (bit k: point k sees light j): nothing here traces.  `dtype=np.float32` in rays() rounds the distance and
forms the origin as the kernel does (scripts/medium_f32_error.py); everything else is float64 as in the kernels.  The
sample stream is sky_ref's, the box film refract_ref's, the lights directional_ref's.  A helper module."""
import types

import numpy as np

import sky_ref as S
from directional_ref import light, unit  # noqa: F401
from refract_ref import film  # noqa: F401

PARAMS = 3      # sigma_t, albedo, g: then one irradiance per light


def medium(sigma_t, albedo=0.75, g=0.0, top_origin=(0.0, 0.0, 1.0), top_normal=(0.0, 0.0, 1.0)):
    """the plane as the doubles and the three scalars as the float32 values hf_medium_t holds"""
    f = lambda x: float(np.float32(x))
    return types.SimpleNamespace(sigma_t=f(sigma_t), albedo=f(albedo), g=f(g), top_origin=np.asarray(top_origin, np.float64).reshape(3),
                                 top_normal=np.asarray(top_normal, np.float64).reshape(3))


def normal(M):
    return M.top_normal / np.sqrt((M.top_normal * M.top_normal).sum())


def _dot(a, b):
    return (a * b).sum(0)


def nu(M, L):
    """<l, N>: a light shines into the medium when it is > 0"""
    return float(_dot(unit(L)[0], normal(M)))


def segment(M, o, d, t):
    """the part of every primary ray inside the medium: a namespace with h, c, u_in, u_out, S, D [n] and the masks elig
    (t > 0, not NaN, u_out > u_in) and at_t (the segment ends at t: dS/dt = 1)"""
    o, d, t = (np.asarray(x, np.float64) for x in (o, d, t))
    N = normal(M)
    q = types.SimpleNamespace()
    q.h = _dot(o - M.top_origin[:, None], N[:, None])
    q.c = _dot(d, N[:, None])
    down, inside = q.c < 0, (q.c >= 0) & (q.h < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q.u_in = np.where(down, np.maximum(0.0, q.h / -q.c), 0.0)
        top = np.where(inside & (q.c > 0), -q.h / q.c, np.inf)
    q.at_t = down | (t <= top)
    q.u_out = np.where(down, t, np.where(inside, np.where(q.at_t, t, top), 0.0))
    q.elig = (down | inside) & (t > 0) & (q.u_out > q.u_in)
    with np.errstate(invalid="ignore"):
        q.S = np.where(q.elig, q.u_out - q.u_in, 0.0)
    q.D = np.where(q.u_in == 0.0, -q.h, 0.0)
    return q


def draws(M, q, ids, K, seed):
    """(xi [K, n], a [n], tau [K, n]): xi_k the first number of sky_ref.samples(ids, k, seed), a = 1 - exp(-sigma_t S),
    tau_k = -log1p(-xi_k a)"""
    xi = np.stack([S.samples(ids, k, seed)[0] for k in range(K)])
    a = -np.expm1(-M.sigma_t * q.S)
    return xi, a, -np.log1p(-xi * a[None])


def ids_of(n, ray_id=None):
    return np.arange(n, dtype=np.uint64) if ray_id is None else np.asarray(ray_id).astype(np.uint64)


def rays(M, L, o, d, t, k, seed=0, ray_id=None, dtype=np.float64):
    """shadow ray k of every sample towards the light L: (o [3, n], d [3, n], maxt [n], traced [n]); the direction is l
    rounded to float32; an untraced lane has a zero origin and direction and maxt = -1.  float64: the exact point
    o + u_k d; float32: u_k rounded to float32, then one fused multiply-add per component, as the kernel forms it"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    q = segment(M, o, d, t)
    n = o.shape[1]
    xi, a, tau = draws(M, q, ids_of(n, ray_id), k + 1, seed)
    u = q.u_in + tau[k] / M.sigma_t
    tr = q.elig & (nu(M, L) > 0)
    if dtype == np.float32:
        # (the product of two float32 is exact in float64: one rounding to float64, one to float32, an fma to within 2^-53)
        with np.errstate(over="ignore", invalid="ignore"):
            p = (u.astype(np.float32).astype(np.float64)[None] * d + o).astype(np.float32).astype(np.float64)
    else:
        with np.errstate(invalid="ignore"):
            p = o + u[None] * d
    lf = unit(L)[0].astype(np.float32).astype(np.float64)[:, None]
    return np.where(tr[None], p, 0.0), np.where(tr[None], np.repeat(lf, n, 1), 0.0), np.where(tr, np.inf, -1.0), tr


def phase(M, L, d):
    """(p [n], dp/dg [n]) of hg.cpp:66-69 with wi = -d, wo = l"""
    g = M.g
    cs = -_dot(np.asarray(d, np.float64), unit(L)[0][:, None])
    temp = 1.0 + g * g + 2.0 * g * cs
    return (1.0 - g * g) / (4.0 * np.pi * temp ** 1.5), (-2.0 * g * temp - 3.0 * (1.0 - g * g) * (g + cs)) / (4.0 * np.pi * temp ** 2.5)


def unpack(words, K):
    """[K, n] booleans of one light's [n] words"""
    w = np.asarray(words).astype(np.uint32)
    return np.stack([((w >> np.uint32(k)) & np.uint32(1)).astype(bool) for k in range(K)])


def pack(vis):
    """[n] uint32 words of [K, n] booleans"""
    return sum((np.asarray(v).astype(np.uint32) << np.uint32(k)) for k, v in enumerate(vis))


def _terms(M, lights, o, d, t, weight, bits, K, seed, ray_id):
    """what forward, adjoint and tangent form of every sample: the segment, the draws and per light the two sums over the
    points whose bit is set, A0 = sum exp(-x_k) and A1 = sum exp(-x_k) xi_k / (1 - xi_k a), added in k order"""
    x = types.SimpleNamespace()
    d = np.asarray(d, np.float64)
    x.q = segment(M, o, d, t)
    x.n = d.shape[1]
    x.xi, x.a, x.tau = draws(M, x.q, ids_of(x.n, ray_id), K, seed)
    x.w = np.ones(x.n) if weight is None else np.asarray(weight, np.float64)
    eS = np.exp(-M.sigma_t * x.q.S)
    x.a_S = M.sigma_t * eS
    x.a_sigma = np.where(np.isfinite(x.q.S), x.q.S, 0.0) * eS
    x.nu, x.E, x.p, x.dpdg, x.A0, x.A1 = [], [], [], [], [], []
    for L, words in zip(lights, bits):
        v = nu(M, L)
        b = unpack(words, K) & x.q.elig[None] & (v > 0)
        A0, A1 = np.zeros(x.n), np.zeros(x.n)
        for k in range(K):
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(b[k], np.exp(-(M.sigma_t * x.q.D - x.tau[k] * x.q.c) / v), 0.0) if v > 0 else np.zeros(x.n)
            A0 = A0 + e
            A1 = A1 + e * x.xi[k] / (1.0 - x.xi[k] * x.a)
        p, dpdg = phase(M, L, d)
        x.nu.append(v); x.E.append(L.irradiance); x.p.append(p); x.dpdg.append(dpdg); x.A0.append(A0); x.A1.append(A1)
    return x


def forward(M, lights, o, d, t, weight, bits, K, seed=0, ray_id=None, spp=1):
    """(image [J, n / spp], value [J, n])"""
    x = _terms(M, lights, o, d, t, weight, bits, K, seed, ray_id)
    value = np.stack([x.w * M.albedo * x.a * x.p[j] * x.E[j] * x.A0[j] / K for j in range(len(lights))])
    return np.stack([film(v, spp) for v in value]), value


def tangent(M, lights, o, d, t, weight, bits, K, seed=0, ray_id=None, spp=1, dw=None, dt=None, d_params=None):
    """(dimage [J, n / spp], dvalue [J, n]) for the tangents dw [n], dt [n], d_params [3 + J] (None: zero)"""
    x = _terms(M, lights, o, d, t, weight, bits, K, seed, ray_id)
    z = lambda a: np.zeros(x.n) if a is None else np.asarray(a, np.float64)
    dp = np.zeros(PARAMS + len(lights)) if d_params is None else np.asarray(d_params, np.float64)
    dsig, dalb, dg = dp[:PARAMS]
    dS = np.where(x.q.at_t, z(dt), 0.0)
    da = x.a_S * dS + x.a_sigma * dsig
    out = []
    for j in range(len(lights)):
        if not x.nu[j] > 0:
            out.append(np.zeros(x.n)); continue
        T = x.A0[j] / K
        dT = -(x.q.D * dsig * x.A0[j] - x.q.c * da * x.A1[j]) / (K * x.nu[j])
        p, E = x.p[j], x.E[j]
        out.append(z(dw) * M.albedo * x.a * p * E * T + x.w * dalb * x.a * p * E * T + x.w * M.albedo * da * p * E * T
                   + x.w * M.albedo * x.a * x.dpdg[j] * dg * E * T + x.w * M.albedo * x.a * p * dp[PARAMS + j] * T
                   + x.w * M.albedo * x.a * p * E * dT)
    out = np.stack(out)
    return np.stack([film(v, spp) for v in out]), out


def adjoint(M, lights, o, d, t, weight, bits, K, seed=0, ray_id=None, spp=1, grad_image=None, grad_value=None, rows=None):
    """the reverse sweep: a namespace with gw [n], gt [n] (the lights summed in light order), gp [3 + J] and gp_abs, the
    sums of the absolute values of the terms of gp (what a bound on the rounding of such a sum is relative to).  rows: a
    slice of the samples the sums gp are taken over (None: all)"""
    x = _terms(M, lights, o, d, t, weight, bits, K, seed, ray_id)
    J = len(lights)
    out = types.SimpleNamespace(gw=np.zeros(x.n), gt=np.zeros(x.n), gp=np.zeros(PARAMS + J), gp_abs=np.zeros(PARAMS + J))
    keep = np.zeros(x.n, bool)
    keep[slice(None) if rows is None else rows] = True
    for j in range(J):
        if not x.nu[j] > 0:
            continue
        g = np.zeros(x.n)
        if grad_image is not None:
            g = g + np.repeat(np.asarray(grad_image, np.float64)[j], spp) / spp
        if grad_value is not None:
            g = g + np.asarray(grad_value, np.float64)[j]
        lit = x.A0[j] > 0
        g = np.where(lit, g, 0.0)
        # value = w alb a p E T, T = A0 / K;  T depends on a (through tau) and on sigma_t (through sigma_t D)
        T = x.A0[j] / K
        front = M.albedo * x.p[j] * x.E[j]
        out.gw += g * front * x.a * T
        g_a = g * x.w * front * T                                  # the explicit factor a
        g_T = g * x.w * front * x.a
        g_a = g_a + g_T * x.q.c * x.A1[j] / (K * x.nu[j])          # T's points move with a
        g_sigma = -g_T * x.q.D * x.A0[j] / (K * x.nu[j]) + g_a * x.a_sigma
        out.gt += np.where(x.q.at_t, g_a * x.a_S, 0.0)
        rows4 = (g_sigma, g * x.w * x.a * x.p[j] * x.E[j] * T, g * x.w * M.albedo * x.a * x.dpdg[j] * x.E[j] * T,
                 g * x.w * M.albedo * x.a * x.p[j] * T)
        for m, row in zip((0, 1, 2, PARAMS + j), rows4):
            out.gp[m] += (row * keep).sum()
            out.gp_abs[m] += (np.abs(row) * keep).sum()
    return out


# ---- the scene of tests/test_gpu_medium.py, shared with scripts/medium_f32_error.py (CPU, through the oracle) ----
# Two orthographic wavefronts of 64 x 64 x 4 samples with one direction: row_helpers.base_scene's (scale 0.9: over the
# terrain) and a narrower one centred over the terrain's +x edge, of which about nine tenths pass beside the terrain
# (t = inf) and go on below it, under the sheet: from there a shadow ray meets the terrain from below.  The camera plane
# lies between z = 1.5 and z = 3: above the first medium (u_in > 0, D = 0), inside the second (u_in = 0, D > 0).
ORIGIN = (1.8, 0.5, 2.25)
TARGET = (0.0, 0.0, 0.25)
FILM = (64, 64, 4)
SHIFT = (1.3, 0.36, 0.0)
NARROW = (0.5, 0.5, 1.0)
K = 4
SEED = 11
# two lights, to_light deliberately not unit: a raking one (19 degrees: shadows three times as long as the relief is
# high) and a high one
RIG = (((-1.0, -0.2, 0.35), 1.5), ((-0.1, 0.15, 1.0), 2.5))
BELOW = ((0.3, 0.1, -0.6), 1.0)      # does not shine into a medium whose top faces up
MEDIA = {"above": dict(sigma_t=0.3, albedo=0.75, g=0.3, top_origin=(0.0, 0.0, 1.5)),
         "inside": dict(sigma_t=0.3, albedo=0.9, g=-0.2, top_origin=(0.3, -0.2, 3.0)),
         "tilted": dict(sigma_t=0.4, albedo=0.6, g=0.5, top_origin=(0.0, 0.0, 1.5), top_normal=(0.3, -0.2, 2.0))}


def rig(specs=RIG):
    return [light(*s) for s in specs]


def wide_rays(ortho_rays, device):
    """the second wavefront, [7, n]: the first one's direction, moved by SHIFT"""
    moved = lambda v: tuple(a + b for a, b in zip(v, SHIFT))
    return ortho_rays(*FILM, device, seed=2, origin=moved(ORIGIN), target=moved(TARGET), scale=NARROW)


def spawn_offset(p):
    """the sky row's spawn offset at the primary hit p [3, n]: (1 + max|p_c|) 1500 2^-24"""
    return (1.0 + np.abs(np.asarray(p, np.float64)).max(0)) * S.RAY_EPSILON


def assert_scene(name, q, t):
    """what the GPU test and the script assert of a medium on the scene before comparing anything"""
    hit = np.isfinite(t)
    assert 0.05 <= hit.mean() <= 0.95, hit.mean()
    assert q.elig.all()
    if name == "above":
        assert (q.u_in > 0).all() and (q.D == 0).all() and q.S.min() >= 1.0, (q.u_in.min(), q.S.min())
    if name == "inside":
        assert (q.u_in == 0).all() and (q.D > 0).all()


def inputs(n, spp, J, seed=5):
    """the weights, upstream gradients and tangents of the GPU test"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(J, n // spp), gv=f(J, n), dw=f(n), dt=(0.1 * f(n)),
                                 dp=(0.3 * f(PARAMS + J)).astype(np.float32))


def oracle_scene():
    """the scene on the CPU: (rays [7, n] float32 of both wavefronts, t [n], the primary hit points p [3, n], the oracle's
    field)"""
    import hf_amd
    from oracle import hf_oracle as O
    O.build()
    h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
    f = O.OracleField(h, max_height=0.5)
    r = np.concatenate([hf_amd.workload.ortho_rays(*FILM, "cpu", seed=1, origin=ORIGIN, target=TARGET, scale=(0.9, 0.9, 1.0)).numpy(),
                        wide_rays(hf_amd.workload.ortho_rays, "cpu").numpy()], 1)
    t = f.ray_intersect_preliminary(r)[0]
    with np.errstate(invalid="ignore"):
        p = r[0:3].astype(np.float64) + np.asarray(t, np.float64)[None] * r[3:6]
    return r, t, p, f


def probe(M, L, r, t, p, field, k, seed=SEED):
    """point k towards one light through the oracle: a namespace with the float64 and float32 origins, traced, vis [n] and
    near [n]: the lanes whose origin lies closer to the primary hit than the sky row's spawn offset (left out of the
    comparison with the oracle's ray_test)"""
    q = types.SimpleNamespace()
    q.o64, w, maxt, q.tr = rays(M, L, r[0:3], r[3:6], t, k, seed)
    q.o32 = rays(M, L, r[0:3], r[3:6], t, k, seed, dtype=np.float32)[0]
    rows = np.concatenate([q.o32, w, maxt[None]]).astype(np.float32)
    occ = np.zeros(len(t), bool)
    occ[q.tr] = field.ray_test(rows[:, q.tr]).astype(bool)
    q.vis = q.tr & ~occ
    with np.errstate(invalid="ignore"):
        q.near = q.tr & np.isfinite(t) & (np.sqrt(((q.o32 - p) ** 2).sum(0)) < spawn_offset(p))
    return q

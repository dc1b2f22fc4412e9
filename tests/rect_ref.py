"""The area-light row (include/hf.h hf_rect_rays, hf_rect_lighting, _adjoint, _tangent) restated in numpy from the formulas
of the header, not from the kernel: the lamp (n_l, A), the points its draws pick, the geometry term G = c_s c_l / r^2,
the masks, the shadow rays of spawn_ray_to, the value, the box film, and the adjoint and the tangent with respect to sh_n,
p, weight and the texels.  Visibility is an input (a [K, n] bit array): nothing here traces.  float64 by default;
`dtype=np.float32` evaluates the same text in float32 (scripts/rect_f32_error.py: the kernel forms G in double, so this is
the coarser of the two).  The sample stream is sky_ref's, the bilinear lookup refract_ref's.  A helper module."""
import types

import numpy as np

import refract_ref as R
import sky_ref as S
from refract_ref import film, textures  # noqa: F401
from sky_ref import eligible, unpack  # noqa: F401

SHADOW_EPSILON = 10.0 * S.RAY_EPSILON  # math.h:22
TARGET = (0.0, 0.0, 0.25)
# what scripts/rect_f32_error.py measured the float32 error of the restatement with, and tests/test_gpu_rect.py runs with
RADIANCE, ALBEDO = 10.0, 0.8
# a mask is decided by the sign of a float32 quantity (<sh_n, -d>, c_s, c_l); the kernel's u = q - p is within 3e-7 of the
# restatement's and r >= 0.17 on the tests' scenes, so its cosines are within 2e-6: a lane on which one of them is below
# this is decided by rounding and is left out of mask comparisons
MARGIN = 1e-5


def lamp(center, ex, ey, radiance=1.0, towards=None):
    """the rectangle emitter with to_world = (center, ex, ey): the float32 fields the entries take, n_l = normalize(ex x ey)
    and A = 4 |ex x ey| in float64.  `towards`: a point the normal is turned to (ex and ey change places if it faces away)"""
    c, ex, ey = (np.asarray(v, np.float32).astype(np.float64) for v in (center, ex, ey))
    if towards is not None and np.dot(np.cross(ex, ey), np.asarray(towards, np.float64) - c) < 0:
        ex, ey = ey, ex
    cr = np.cross(ex, ey)
    return types.SimpleNamespace(center=c, ex=ex, ey=ey, nl=cr / np.linalg.norm(cr), A=4.0 * np.linalg.norm(cr),
                                 radiance=float(np.float32(radiance)))


# the two lamps of the row's tests: one above the terrain, one beside it whose light grazes the relief
LAMPS = {"above": lambda L=1.0: lamp((0.2, -0.1, 1.1), (0.3, 0.0, 0.05), (0.0, 0.2, 0.0), L, TARGET),
         "side": lambda L=1.0: lamp((1.1, -0.9, 0.6), (0.25, 0.25, 0.0), (0.1, -0.1, 0.2), L, TARGET)}


def _dot(a, b):
    return (a * b).sum(-2)


def draws(ids, K, seed):
    """[K, 2, n]: the draws (s.x, s.y) of every sample, sky_ref's stream (pair = k)"""
    return np.stack([np.stack(S.samples(ids, k, seed)) for k in range(K)])


def geometry(p, sh_n, s, lm, dtype=np.float64):
    """of the draws s [K, 2, n]: q = center + (2 s.x - 1) ex + (2 s.y - 1) ey [K, 3, n], u = q - p, r, w = u / r,
    c_s = <sh_n, w>, c_l = -<n_l, w>"""
    f = lambda x: np.asarray(x, dtype)
    p, sh_n, s = f(p), f(sh_n), f(s)
    col = lambda v: f(v)[None, :, None]
    g = types.SimpleNamespace()
    g.q = col(lm.center) + (dtype(2) * s[:, 0:1] - dtype(1)) * col(lm.ex) + (dtype(2) * s[:, 1:2] - dtype(1)) * col(lm.ey)
    g.u = g.q - p[None]
    with np.errstate(all="ignore"):
        g.r = np.sqrt(_dot(g.u, g.u))
        g.w = g.u / g.r[:, None]
        g.cs = _dot(sh_n[None], g.w)
        g.cl = -_dot(col(lm.nl), g.w)
    return g


def traced(sh_n, d, t, g):
    """[K, n]: draw k of an eligible sample is traced when c_s > 0, c_l > 0 and r is finite and > 0; and the margin of
    the decision, min(|c_s|, |c_l|)"""
    el, _ = eligible(sh_n, d, t)
    with np.errstate(invalid="ignore"):
        ok = (g.cs > 0) & (g.cl > 0) & np.isfinite(g.r) & (g.r > 0)
    return el[None] & ok, np.minimum(np.abs(g.cs), np.abs(g.cl))


def rays(p, nrm, sh_n, d, t, ids, k, seed, lm):
    """shadow ray k of every sample, spawn_ray_to(q_k) (interaction.h:141-147): (o [3, n], direction [3, n], maxt [n],
    traced [n]); lanes that are not traced: zeros and maxt = -1"""
    s = draws(ids, k + 1, seed)[k:k + 1]
    g = geometry(p, sh_n, s, lm)
    tr = traced(sh_n, d, t, g)[0][0]
    o = S.spawn_origin(p, nrm, g.u[0])
    dv = g.q[0] - o
    dist = np.sqrt(_dot(dv, dv))
    with np.errstate(all="ignore"):
        w = dv / dist
    return np.where(tr[None], o, 0.0), np.where(tr[None], w, 0.0), np.where(tr, dist * (1.0 - SHADOW_EPSILON), -1.0), tr


def _terms(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, dtype):
    """what forward, adjoint and tangent form of every draw: the bit (of eligible samples only), L_k (the texture's part:
    1 without one), G and its derivatives dG/dsh_n = w c_l / r^2, dG/dp = (4 c_s c_l w - c_l sh_n + c_s n_l) / r^3"""
    bits = np.asarray(bits, bool)
    K, n = bits.shape
    el, _ = eligible(sh_n, d, t)
    x = types.SimpleNamespace(b=bits & el[None], K=K, n=n)
    s = draws(ids, K, seed)
    g = geometry(p, sh_n, s, lm, dtype)
    sn = np.asarray(sh_n, dtype)[None]
    nl = np.asarray(lm.nl, dtype)[None, :, None]
    with np.errstate(all="ignore"):
        r2 = g.r * g.r
        x.G = g.cs * g.cl / r2
        x.Gn = g.w * (g.cl / r2)[:, None]
        x.Gp = (dtype(4) * (g.cs * g.cl)[:, None] * g.w - g.cl[:, None] * sn + g.cs[:, None] * nl) / (r2 * g.r)[:, None]
    z = dtype(0)
    x.G, x.Gn, x.Gp = np.where(x.b, x.G, z), np.where(x.b[:, None], x.Gn, z), np.where(x.b[:, None], x.Gp, z)
    x.L, x.e = np.ones((K, n), dtype), None
    if tex is not None:
        TH, TW = np.asarray(tex).shape
        x.e = [R.lookup(tex, np.stack([s[k, 0] * TW, s[k, 1] * TH]).astype(dtype), R.CLAMP, dtype) for k in range(K)]
        x.L = np.stack([e.L for e in x.e])
    x.wgt = np.ones(n, dtype) if weight is None else np.asarray(weight, dtype)
    x.c = dtype(lm.radiance) * dtype(lm.A) / dtype(np.pi * K)   # times the albedo: the scale of the sum
    return x


def forward(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, albedo, spp, dtype=np.float64):
    """(image [n / spp], per-sample values [n]): value = weight (albedo A / (pi K)) sum_k bit L_k G_k"""
    x = _terms(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, dtype)
    value = x.wgt * (dtype(albedo) * x.c) * (x.L * x.G).sum(0)
    return film(value, spp), value


def adjoint(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, albedo, spp, grad_image, dtype=np.float64):
    """(grad_sh_n [3, n], grad_p [3, n], grad_weight [n], grad_tex [TH, TW] or None)"""
    x = _terms(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, dtype)
    g = np.repeat(np.asarray(grad_image, dtype), spp) / dtype(spp)
    c = g * (dtype(albedo) * x.c)
    gn = (c * x.wgt)[None] * (x.L[:, None] * x.Gn).sum(0)
    gp = (c * x.wgt)[None] * (x.L[:, None] * x.Gp).sum(0)
    gw = c * (x.L * x.G).sum(0)
    gtex = None
    if tex is not None:
        gtex = np.zeros(np.asarray(tex).size, dtype)
        for k in range(x.K):
            m = x.b[k]
            for j in range(4):
                np.add.at(gtex, x.e[k].idx[j][m], ((c * x.wgt) * x.G[k] * x.e[k].b[j])[m])
        gtex = gtex.reshape(np.asarray(tex).shape)
    return gn, gp, gw, gtex


def tangent(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, albedo, spp, dn=None, dp=None, dw=None, dtex=None,
            dtype=np.float64):
    """(dimage [n / spp], dvalue [n]) for tangents dn of sh_n, dp of p, dw of weight and dtex of the texels (None: zero)"""
    x = _terms(p, sh_n, d, t, weight, bits, ids, seed, lm, tex, dtype)
    sd = np.zeros(x.n, dtype)
    if dn is not None:
        sd = sd + (x.L * _dot(np.asarray(dn, dtype)[None], x.Gn)).sum(0)
    if dp is not None:
        sd = sd + (x.L * _dot(np.asarray(dp, dtype)[None], x.Gp)).sum(0)
    if dtex is not None and tex is not None:
        dt = np.asarray(dtex, dtype).ravel()
        for k in range(x.K):
            sd = sd + x.G[k] * sum(x.e[k].b[j] * dt[x.e[k].idx[j]] for j in range(4))
    dv = x.wgt * sd
    if dw is not None:
        dv = dv + np.asarray(dw, dtype) * (x.L * x.G).sum(0)
    dv = (dtype(albedo) * x.c) * dv
    return film(dv, spp), dv


def inputs(n, spp, tex_shape):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(5)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return types.SimpleNamespace(w=rng.uniform(0.5, 1.5, n).astype(np.float32), gi=f(n // spp), dn=f(3, n), dp=f(3, n),
                                 dw=f(n), dtex=f(*tex_shape))

"""Glossy reflection of the environment map (include/hf.h hf_glossy_*) restated in numpy from the formulas of the
header, not from the kernel: the visible-normal draw of the GGX microfacet normal, the masks, the mirror rays, the Smith
term, the value, and the adjoint and the tangent with respect to sh_n, weight, alpha and the texels.  float64 by
default; `dtype=np.float32` evaluates the same text in float32 (numpy has no fused multiply-add and its trigonometry is
float32 then: the order of operations differs from the kernel's, which is what the tests' factor of four on the
float32-against-float64 error stands for).  All arrays are [3, n] / [n], world space; per direction [K, ...]; `data` is
the [H, W] map with its seam column, `rot` the 3 x 3 rotation map -> world (None: identity); `alpha` a scalar or [n].
Visibility is an input ([K, n] bits): nothing here traces.  `held`: the draws of another (sh_n, alpha), for which the
forward evaluates the attached numerator D(c_h) G1(c_i) G1(c_o) / c_i over the held one -- the function the
derivative differentiates.  A helper module."""
import types

import numpy as np

import sky_ref as S
from caustic_ref import fresnel
from reflect_ref import shade

ALPHA_MIN = 1e-4
EPS4 = 4.0 * 2.0 ** -24        # Frame3f::sincos_phi's threshold


def _dot(a, b):
    return (a * b).sum(0)


def _coordinate_system(n, dtype):
    one = dtype(1)
    sign = np.where(n[2] >= 0, one, -one).astype(dtype)
    a = -one / (sign + n[2])
    b = n[0] * n[1] * a
    return np.stack([sign * (n[0] * n[0] * a) + one, sign * b, -sign * n[0]]), np.stack([b, n[1] * n[1] * a + sign, -n[1]])


def _disk(sx, sy, dtype):
    """square_to_uniform_disk_concentric as hf_bounce_* has it: (px, py)"""
    x, y = dtype(2) * sx.astype(dtype) - dtype(1), dtype(2) * sy.astype(dtype) - dtype(1)
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = dtype(0.25 * np.pi) * rp / r
    phi = np.where((x == 0) & (y == 0), dtype(0), phi).astype(dtype)
    sn, cs = np.sin(phi), np.cos(phi)
    return (r * np.where(q13, sn, cs)).astype(dtype), (r * np.where(q13, cs, sn)).astype(dtype)


def roughness(alpha, n, dtype=np.float64):
    """(a = max(alpha, 1e-4) [n], `free`: alpha > 1e-4, `finite`)"""
    al = np.broadcast_to(np.asarray(alpha, dtype), (n,))
    with np.errstate(invalid="ignore"):
        return np.maximum(np.nan_to_num(al, nan=0.0, posinf=1.0, neginf=0.0), dtype(ALPHA_MIN)).astype(dtype), al > ALPHA_MIN, np.isfinite(al)


def draw(sh_n, d, alpha, ids, k, seed, eta=0.0, dtype=np.float64):
    """draw k of every sample: h, wo [3, n], cwh = <wi, h>, ch = <n, h>, co = <n, wo>, F, valid, and `den`, the
    denominator of sample_visible_11's norm"""
    n_, d = np.asarray(sh_n, dtype), np.asarray(d, dtype)
    a, _, _ = roughness(alpha, n_.shape[1], dtype)
    one, two, z = dtype(1), dtype(2), dtype(0)
    g = types.SimpleNamespace()
    with np.errstate(all="ignore"):
        s, t = _coordinate_system(n_, dtype)
        wi = -d
        wl = np.stack([_dot(wi, s), _dot(wi, t), _dot(wi, n_)])
        wp = np.stack([a * wl[0], a * wl[1], wl[2]])
        wp = wp * (one / np.sqrt(_dot(wp, wp)))
        st2 = wp[0] * wp[0] + wp[1] * wp[1]
        ist = one / np.sqrt(st2)
        pole = np.abs(st2) <= dtype(EPS4)
        cphi = np.where(pole, one, np.clip(wp[0] * ist, -one, one)).astype(dtype)
        sphi = np.where(pole, z, np.clip(wp[1] * ist, -one, one)).astype(dtype)
        ct = wp[2]
        sx, sy = S.samples(ids, k, seed)
        px, py = _disk(sx, sy, dtype)
        sh = dtype(0.5) * (one + ct)
        e = np.sqrt(np.maximum(one - px * px, z))
        x, y = px, py * sh + (e - e * sh)
        zz = np.sqrt(np.maximum(one - (x * x + y * y), z))
        si = np.sqrt(np.maximum(one - ct * ct, z))
        g.den = si * y + ct * zz
        nr = one / g.den
        slx, sly = (ct * y - si * zz) * nr, x * nr
        rx, ry = (cphi * slx - sphi * sly) * a, (sphi * slx + cphi * sly) * a
        hl = np.stack([-rx, -ry, np.ones_like(rx)])
        hl = hl * (one / np.sqrt(_dot(hl, hl)))
        g.h = (s * hl[0] + t * hl[1] + n_ * hl[2]).astype(dtype)
        g.cwh = _dot(wi, g.h)
        g.wo = (g.h * (two * g.cwh) - wi).astype(dtype)
        g.valid = np.isfinite(g.h).all(0) & (g.cwh > 0)
        g.ch, g.co = _dot(n_, g.h), _dot(n_, g.wo)
        g.F = np.ones(g.cwh.shape, dtype) if eta == 0 else fresnel(g.cwh, eta, dtype)[0].astype(dtype)
    g.wi, g.n, g.a = wi, n_, a
    return g


def eligible(nrm, sh_n, d, t, active, alpha):
    """(eligible [n], margin: the smallest magnitude among the quantities whose sign decides it)"""
    g, n_, d = (np.asarray(x, np.float64) for x in (nrm, sh_n, d))
    act = np.ones(n_.shape[1], bool) if active is None else np.asarray(active).astype(bool)
    _, _, fin = roughness(alpha, n_.shape[1])
    ci, gi = -_dot(n_, d), -_dot(g, d)
    return act & np.isfinite(np.asarray(t, np.float64)) & fin & (ci > 0) & (gi > 0), np.minimum(np.abs(ci), np.abs(gi))


def traced(nrm, dr, elig):
    """(traced [n], margin) of one draw: eligible, valid, c_o > 0 and <g, wo> > 0; the margin counts <wi, h>, c_o,
    <g, wo> and the denominator of the draw's norm (scaled: 1e-4 there is 1e-5 here)"""
    go = _dot(np.asarray(nrm, dr.wo.dtype), dr.wo)
    with np.errstate(invalid="ignore"):
        tr = elig & dr.valid & (dr.co > 0) & (go > 0)
        m = np.minimum.reduce([np.abs(dr.cwh), np.abs(dr.co), np.abs(go), 0.1 * np.abs(dr.den)])
    return tr, np.nan_to_num(m, nan=0.0)


def rays(p, nrm, sh_n, d, t, alpha, k, seed=0, ids=None, active=None):
    """(traced, origin [3, n], direction [3, n], maxt [n], h [3, n], margin, draw) of mirror ray k in float64; untraced
    lanes: zero ray, maxt -1; h is zero for an invalid draw or a sample that is not eligible"""
    n = np.asarray(sh_n).shape[1]
    ids = np.arange(n) if ids is None else ids
    el, m0 = eligible(nrm, sh_n, d, t, active, alpha)
    dr = draw(sh_n, d, alpha, ids, k, seed)
    tr, m1 = traced(nrm, dr, el)
    wo = np.where(tr[None], dr.wo, 0.0)
    o = np.where(tr[None], S.spawn_origin(np.asarray(p, np.float64), np.asarray(nrm, np.float64), wo), 0.0)
    h = np.where((el & dr.valid)[None], dr.h, 0.0)
    return tr, o, wo, np.where(tr, np.inf, -1.0), h, np.where(el, np.minimum(m0, m1), m0), dr


def smith(a, c, dtype=np.float64):
    """(G1, dG1/dc, dG1/da) of the header's frame-free Smith term"""
    one, two = dtype(1), dtype(2)
    with np.errstate(all="ignore"):
        a2, m, c2 = a * a, np.maximum(one - c * c, dtype(0)), c * c
        T = a2 * m / c2
        r = np.sqrt(one + T)
        q = one + r
        dT = -one / ((q * q) * r)
        return two / q, dT * (-two * a2 / (c2 * c)), dT * (two * a * m / c2)


def _lnD(a, ch):
    """ln of the GGX distribution up to a constant"""
    q = ch * ch * (a * a - 1) + 1
    return 2 * np.log(a) - 2 * np.log(q)


def _setup(nrm, sh_n, d, t, active, weight, alpha, K, seed, ids, bits, dtype):
    n = np.asarray(sh_n).shape[1]
    ids = np.arange(n) if ids is None else ids
    el, _ = eligible(nrm, sh_n, d, t, active, alpha)
    w = np.ones(n, dtype) if weight is None else np.asarray(weight, dtype)
    bits = np.asarray(bits).astype(bool).reshape(K, n)
    return n, ids, el, w, bits


def forward(nrm, sh_n, d, t, active, weight, alpha, eta, K, seed, ids, data, rot, bits, spp=1, dtype=np.float64, held=None):
    """(image [n / spp], value [n]) for the visibility `bits` [K, n] (a direction counts when it is traced and its bit is
    set).  held = (sh_n0, alpha0): the draws are those of (sh_n0, alpha0) and the attached numerator is evaluated at
    (sh_n, alpha)"""
    n, ids, el, w, bits = _setup(nrm, sh_n, d, t, active, weight, alpha, K, seed, ids, bits, dtype)
    a, _, _ = roughness(alpha, n, dtype)
    acc = np.zeros(n, dtype)
    for k in range(K):
        if held is None:
            dr = draw(sh_n, d, alpha, ids, k, seed, eta, dtype)
            tr, _ = traced(nrm, dr, el)
            fg = dr.F * smith(a, dr.co, dtype)[0]
        else:
            dr = draw(held[0], d, held[1], ids, k, seed, eta, dtype)
            tr, _ = traced(nrm, dr, el)
            nn = np.asarray(sh_n, dtype)
            with np.errstate(all="ignore"):
                ci, ch, co = _dot(nn, dr.wi), _dot(nn, dr.h), _dot(nn, dr.wo)
                lnA = _lnD(a, ch) + np.log(smith(a, ci, dtype)[0]) - np.log(ci)
                lnA0 = _lnD(dr.a, dr.ch) + np.log(smith(dr.a, _dot(dr.n, dr.wi), dtype)[0]) - np.log(_dot(dr.n, dr.wi))
                fg = dr.F * smith(a, co, dtype)[0] * np.exp(lnA - lnA0)
        lit = tr & bits[k]
        L = shade(dr.wo, data, rot, dtype).L
        with np.errstate(all="ignore"):
            acc = (acc + np.where(lit, fg * L, dtype(0))).astype(dtype)
    value = (w * (dtype(1) / dtype(K)) * acc).astype(dtype)
    return value.reshape(-1, spp).mean(1, dtype=dtype), value


def _sums(nrm, sh_n, d, t, active, alpha, eta, K, seed, ids, data, rot, bits, el, dtype):
    """per sample: N [3, n], A [n], S [n] of the header's derivative and, per direction, (lit, F G1(c_o), shade)"""
    n = np.asarray(sh_n).shape[1]
    a, free, _ = roughness(alpha, n, dtype)
    one, two, four = dtype(1), dtype(2), dtype(4)
    N, A, Ssum, per = np.zeros((3, n), dtype), np.zeros(n, dtype), np.zeros(n, dtype), []
    for k in range(K):
        dr = draw(sh_n, d, alpha, ids, k, seed, eta, dtype)
        tr, _ = traced(nrm, dr, el)
        lit = tr & bits[k]
        s = shade(dr.wo, data, rot, dtype)
        with np.errstate(all="ignore"):
            ci = _dot(dr.n, dr.wi)
            Gi, Gi_c, Gi_a = smith(a, ci, dtype)
            Go, Go_c, Go_a = smith(a, dr.co, dtype)
            a2m1 = a * a - one
            q = dr.ch * dr.ch * a2m1 + one
            dDc, dDa = -four * dr.ch * a2m1 / q, two / a - four * dr.ch * dr.ch * a / q
            FL = dr.F * s.L
            Nk = (FL * Go) * (dDc * dr.h + (Gi_c / Gi - one / ci) * dr.wi) + (FL * Go_c) * dr.wo
            Ak = FL * (Go * (dDa + Gi_a / Gi) + Go_a)
            N = N + np.where(lit[None], Nk, dtype(0)); A = A + np.where(lit, Ak, dtype(0))
            Ssum = Ssum + np.where(lit, dr.F * Go * s.L, dtype(0))
        per.append((lit, dr.F * Go, s))
    return N.astype(dtype), np.where(free, A, dtype(0)).astype(dtype), Ssum.astype(dtype), per


def adjoint(nrm, sh_n, d, t, active, weight, alpha, eta, K, seed, ids, data, rot, bits, spp, grad_image, grad_value,
            dtype=np.float64):
    """(grad_sh_n [3, n], grad_weight [n], grad_alpha [n], grad_data [H, W]) for dL/dimage [n / spp] and dL/dvalue [n]"""
    n, ids, el, w, bits = _setup(nrm, sh_n, d, t, active, weight, alpha, K, seed, ids, bits, dtype)
    g = np.zeros(n, dtype)
    if grad_image is not None:
        g = g + np.repeat(np.asarray(grad_image, dtype), spp) / dtype(spp)
    if grad_value is not None:
        g = g + np.asarray(grad_value, dtype)
    N, A, Ssum, per = _sums(nrm, sh_n, d, t, active, alpha, eta, K, seed, ids, data, rot, bits, el, dtype)
    gk = (g * w) * (dtype(1) / dtype(K))
    gd = np.zeros(np.asarray(data).size, dtype)
    for lit, fg, s in per:
        with np.errstate(all="ignore"):
            np.add.at(gd, s.idx[:, lit], ((gk * fg)[None] * s.b)[:, lit])
    return N * gk, (g * (dtype(1) / dtype(K))) * Ssum, A * gk, gd.reshape(np.asarray(data).shape)


def tangent(nrm, sh_n, d, t, active, weight, alpha, eta, K, seed, ids, data, rot, bits, spp, dsh_n=None, dweight=None,
            dalpha=None, ddata=None, dtype=np.float64):
    """(dimage [n / spp], dvalue [n]) for tangents dsh_n [3, n], dweight [n], dalpha [n] and ddata [H, W] (None: zero)"""
    n, ids, el, w, bits = _setup(nrm, sh_n, d, t, active, weight, alpha, K, seed, ids, bits, dtype)
    dn = np.zeros((3, n), dtype) if dsh_n is None else np.asarray(dsh_n, dtype)
    dw = np.zeros(n, dtype) if dweight is None else np.asarray(dweight, dtype)
    da = np.zeros(n, dtype) if dalpha is None else np.broadcast_to(np.asarray(dalpha, dtype), (n,))
    N, A, Ssum, per = _sums(nrm, sh_n, d, t, active, alpha, eta, K, seed, ids, data, rot, bits, el, dtype)
    dv = _dot(N, dn) + A * da
    if ddata is not None:
        dd = np.asarray(ddata, dtype).ravel()
        for lit, fg, s in per:
            with np.errstate(all="ignore"):
                dv = dv + np.where(lit, fg * (s.b * dd[s.idx]).sum(0), dtype(0))
    ik = dtype(1) / dtype(K)
    dv = (dw * ik * Ssum + w * ik * dv).astype(dtype)
    return dv.reshape(-1, spp).mean(1, dtype=dtype), dv


def unpack(words, K):
    """[K, n] bits of the [n] visibility words"""
    w = np.asarray(words).view(np.uint32)
    return ((w[None, :] >> np.arange(K, dtype=np.uint32)[:, None]) & 1).astype(bool)


def pdf(h, wi, n, a):
    """the density of the draw over the solid angle of h: D G1(c_i) <wi, h> / c_i (microfacet.h:219-228)"""
    ch, ci = _dot(n, h), _dot(n, wi)
    q = ch * ch * (a * a - 1) + 1
    D = a * a / (np.pi * q * q)
    return np.where(ch > 0, D * smith(a, ci)[0] * np.maximum(_dot(wi, h), 0) / ci, 0.0)


# ---- the scenes of tests/test_gpu_glossy.py, shared with scripts/glossy_f32_error.py ---------------------------------
FILM, SPP = (25, 23, 4), 4                      # 2300 samples: nine workgroups, the last one partial
ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
ROT2 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) @ \
    np.array([[np.cos(0.7), 0.0, np.sin(0.7)], [0.0, 1.0, 0.0], [-np.sin(0.7), 0.0, np.cos(0.7)]])
ROTS = {"identity": np.eye(3), "rotated": ROT2}
MAP_SIZES = {"sun": (17, 9), "gradient": (9, 5)}
SEED = 5
# (num_rays, alpha, map, rotation): every value of every factor, and each num_rays with two kinds of roughness
COMBOS = ((1, 0.3, "sun", "identity"), (3, "row", "gradient", "rotated"), (32, 0.05, "sun", "rotated"),
          (3, 0.05, "gradient", "identity"), (32, "row", "sun", "identity"), (1, "row", "gradient", "rotated"),
          (32, 0.3, "gradient", "rotated"))


def alpha_row(kind, n):
    """the roughness of a scene as an [n] float32 row: a constant, or uniform in [0.05, 0.6]"""
    if kind == "row":
        return np.random.default_rng(17).uniform(0.05, 0.6, n).astype(np.float32)
    return np.full(n, kind, np.float32)


def test_inputs(n, shape, spp=SPP):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    gi, gv = rng.normal(size=n // spp).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dn, dw = rng.normal(size=(3, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    da = (0.1 * rng.normal(size=n)).astype(np.float32)
    dd = rng.normal(size=shape).astype(np.float32)
    return w, gi, gv, dn, dw, da, dd


test_inputs.__test__ = False

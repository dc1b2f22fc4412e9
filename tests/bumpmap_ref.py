"""The bump map (include/hf.h hf_bumpmap_*) restated in numpy from the formulas of the header, not from the kernel: the
lookup of the one plane at pos = (u TW, v TH) (refract_ref.lookup: the bitmap's cell, its position in the cell and the
slopes under both wraps), the gradient g = scale (TW Lx, TH Ly), the projected tangents P_u = dp_du + b (g_x - <b, dp_du> /
<b, b>), P_v likewise, c = P_u x P_v, N = sigma c / |c| with sigma the sign of <n_geo, c>, the perturbed / pass-through decision, the
tangent with respect to the texels, uv, sh_n, dp_du and dp_dv -- the derivative of the SLOPES: the texels enter with
-+(1 - f), -+f and uv through the cross difference C = v11 - v10 - v01 + v00 -- and an adjoint written on its own as a
reverse sweep.  float64 by default; `dtype=np.float32` evaluates the same text in float32.  All arrays are [3, n] / [2, n]
/ [n]; tex is [TH, TW].  A helper module."""
import types

import numpy as np

import refract_ref as RR
from normalmap_ref import MARGIN, err_abs, err_l2, positions  # noqa: F401
from refract_ref import CLAMP, REPEAT  # noqa: F401

WRAPS = {"clamp": CLAMP, "repeat": REPEAT}
C2_MIN = 1e-12          # |c|^2 below it times |dp_du|^2 |dp_dv|^2: the projected tangents are parallel
SIGMA_MIN = 0.2         # |<n_geo, c / |c|>| the GPU test's inputs keep: sigma is never in doubt


def _dot(x, y):
    return (x * y).sum(0)


def _cross(x, y):
    return np.stack([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]])


def frame(Lx, Ly, read, b, n_geo, dp_du, dp_dv, TW, TH, scale, active=None, dtype=np.float64):
    """the frame algebra from the slopes (Lx, Ly) [n] of the lookup (`read`: the lookup read something): a namespace with N,
    the mask `pert`, g, P_u, P_v, ch = c / |c|, rC = 1 / |c|, sigma and the quantities the conditions are about (ratio =
    |c|^2 / (|dp_du|^2 |dp_dv|^2), cosine = <n_geo, ch> / |n_geo|)"""
    Lx, Ly, b, ng, u, v = (np.asarray(x, dtype) for x in (Lx, Ly, b, n_geo, dp_du, dp_dv))
    n = b.shape[1]
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    s = types.SimpleNamespace(b=b, u=u, v=v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        finite = np.isfinite(b).all(0) & np.isfinite(u).all(0) & np.isfinite(v).all(0) & np.isfinite(ng).all(0)
        s.g = np.stack([dtype(scale) * (dtype(TW) * Lx), dtype(scale) * (dtype(TH) * Ly)])
        B2 = _dot(b, b)
        s.k = dtype(1) / np.where(B2 > 0, B2, dtype(1))            # the projection is exact for the b that arrives
        s.bu, s.bv = _dot(b, u) * s.k, _dot(b, v) * s.k
        s.Pu = u + b * (s.g[0] - s.bu)
        s.Pv = v + b * (s.g[1] - s.bv)
        c = _cross(s.Pu, s.Pv)
        C2, U2, V2 = _dot(c, c), _dot(u, u), _dot(v, v)
        s.ratio = C2 / np.where((U2 > 0) & (V2 > 0), U2 * V2, dtype(1))
        s.pert = act & finite & np.asarray(read, bool) & (B2 > 0) & (U2 > 0) & (V2 > 0) & (C2 >= dtype(C2_MIN) * U2 * V2)
        s.rC = dtype(1) / np.sqrt(np.where(s.pert, C2, dtype(1)))
        s.ch = np.where(s.pert, c * s.rC, dtype(0))
        nc = _dot(ng, c)
        s.sigma = np.where(nc < 0, dtype(-1), dtype(1))
        s.cosine = _dot(ng, s.ch) / np.sqrt(np.where(_dot(ng, ng) > 0, _dot(ng, ng), dtype(1)))
        N = s.sigma * s.ch
    s.N = np.where(s.pert, N, b)
    return s


def _state(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, dtype):
    tex = np.asarray(tex, dtype)
    TH, TW = tex.shape
    pos = positions(uv, TW, TH, dtype)
    e = RR.lookup(tex, pos, wrap, dtype)
    with np.errstate(invalid="ignore"):
        read = e.ok & np.isfinite(np.asarray(uv, np.float64)).all(0)
    s = frame(e.Lx, e.Ly, read, b, n_geo, dp_du, dp_dv, TW, TH, scale, active, dtype)
    s.e, s.pos, s.tex, s.scale = e, pos, tex, dtype(scale)
    v00, v10, v01, v11 = (tex.ravel()[j] for j in e.idx)
    s.C = (v11 - v10) - (v01 - v00)
    one = dtype(1)
    # the slopes' weights of the texels v00, v10, v01, v11
    s.wx = np.stack([-(one - e.fy), one - e.fy, -e.fy, e.fy])
    s.wy = np.stack([-(one - e.fx), -e.fx, one - e.fx, e.fx])
    return s


def forward(tex, uv, b, n_geo, dp_du, dp_dv, active=None, wrap=REPEAT, scale=1.0, dtype=np.float64):
    """(N [3, n], mask [n] bool, the state)"""
    s = _state(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, dtype)
    return s.N, s.pert, s


@np.errstate(invalid="ignore", over="ignore")      # (the pass-through lanes: their numbers are not used)
def tangent(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, dtex=None, duv=None, db=None, ddu=None, ddv=None,
            dtype=np.float64):
    """dN [3, n] with the cell, the decision and sigma held; a tangent that is None is zero"""
    s = _state(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, dtype)
    n = s.b.shape[1]
    TH, TW = s.tex.shape
    z3 = np.zeros((3, n), dtype)
    db, ddu, ddv = (z3 if x is None else np.asarray(x, dtype) for x in (db, ddu, ddv))
    dLx, dLy = np.zeros(n, dtype), np.zeros(n, dtype)
    if dtex is not None:
        dt = np.asarray(dtex, dtype).ravel()[s.e.idx]
        dLx += (s.wx * dt).sum(0)
        dLy += (s.wy * dt).sum(0)
    if duv is not None:
        duv = np.asarray(duv, dtype)
        dLx += s.C * (dtype(TH) * duv[1])
        dLy += s.C * (dtype(TW) * duv[0])
    dg = np.stack([s.scale * (dtype(TW) * dLx), s.scale * (dtype(TH) * dLy)])
    # d(k <b, u>) = k (<db, u> + <b, du> - 2 (k <b, u>) <b, db>), k = 1 / <b, b>
    bdb = dtype(2) * _dot(s.b, db)
    dPu = ddu + db * (s.g[0] - s.bu) + s.b * (dg[0] - s.k * (_dot(db, s.u) + _dot(s.b, ddu) - s.bu * bdb))
    dPv = ddv + db * (s.g[1] - s.bv) + s.b * (dg[1] - s.k * (_dot(db, s.v) + _dot(s.b, ddv) - s.bv * bdb))
    dc = _cross(dPu, s.Pv) + _cross(s.Pu, dPv)
    dN = s.sigma * (dc - s.ch * _dot(s.ch, dc)) * s.rC
    return np.where(s.pert, dN, db)


@np.errstate(invalid="ignore", over="ignore")      # (the pass-through lanes: their numbers are not used)
def adjoint(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, gout, dtype=np.float64):
    """the reverse sweep from gout = dL/dN [3, n]: a namespace with gtex [TH, TW], guv [2, n], gn, gpu, gpv [3, n] and
    q [2, n] = dL/d(Lx, Ly), what the texel scatter multiplies its weights by"""
    s = _state(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, dtype)
    TH, TW = s.tex.shape
    g = np.where(s.pert, np.asarray(gout, dtype), dtype(0))
    # N = sigma c / |c|
    c_bar = s.sigma * (g - s.ch * _dot(s.ch, g)) * s.rC
    # c = P_u x P_v
    Pu_bar, Pv_bar = _cross(s.Pv, c_bar), _cross(c_bar, s.Pu)
    # P_u = u + b (g_x - beta_u), beta_u = <b, u> / B2, B2 = <b, b>
    hu, hv = _dot(Pu_bar, s.b), _dot(Pv_bar, s.b)            # the adjoints of the two scalars g - beta
    b_bar = Pu_bar * (s.g[0] - s.bu) + Pv_bar * (s.g[1] - s.bv)
    # beta = <b, .> / B2, with beta_bar = -h: first the numerator, then B2_bar = -beta_bar beta / B2 and B2 = <b, b>
    num_u, num_v = -hu * s.k, -hv * s.k
    u_bar, v_bar = Pu_bar + s.b * num_u, Pv_bar + s.b * num_v
    B2_bar = (hu * s.bu + hv * s.bv) * s.k
    b_bar = b_bar + s.u * num_u + s.v * num_v + dtype(2) * s.b * B2_bar
    # g = scale (TW Lx, TH Ly)
    Lx_bar, Ly_bar = s.scale * dtype(TW) * hu, s.scale * dtype(TH) * hv
    Lx_bar, Ly_bar = np.where(s.pert, Lx_bar, dtype(0)), np.where(s.pert, Ly_bar, dtype(0))
    out = types.SimpleNamespace(gtex=np.zeros(TH * TW, dtype), q=np.stack([Lx_bar, Ly_bar]))
    for j in range(4):
        np.add.at(out.gtex, s.e.idx[j], np.where(s.pert, s.wx[j] * Lx_bar + s.wy[j] * Ly_bar, dtype(0)))
    out.gtex = out.gtex.reshape(TH, TW)
    out.guv = np.where(s.pert, np.stack([dtype(TW) * s.C * Ly_bar, dtype(TH) * s.C * Lx_bar]), dtype(0))
    out.gn = np.where(s.pert, b_bar, np.asarray(gout, dtype))
    out.gpu = np.where(s.pert, u_bar, dtype(0))
    out.gpv = np.where(s.pert, v_bar, dtype(0))
    return out


def near_edge(state, margin=MARGIN):
    """lanes whose position in the cell is within `margin` of a cell edge on either axis: the slopes jump there"""
    fx, fy = np.asarray(state.e.fx, np.float64), np.asarray(state.e.fy, np.float64)
    return (np.minimum(fx, 1 - fx) < margin) | (np.minimum(fy, 1 - fy) < margin)


def near_threshold(state):
    """lanes within a factor of two of the pass-through threshold on |c|^2"""
    with np.errstate(invalid="ignore"):
        return (state.ratio > 0.5 * C2_MIN) & (state.ratio < 2 * C2_MIN)


def texture(TW, TH, seed=0, amplitude=0.04):
    """[TH, TW] float32: a smooth random relief -- two waves of about `amplitude` with random phases, periodic over the
    unit square so that the repeat wrap meets no cliff at the seam -- plus a little texel noise; its uv gradient is of the
    order 2 pi amplitude"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid((np.arange(TH) + 0.5) / TH, (np.arange(TW) + 0.5) / TW, indexing="ij")
    p = rng.uniform(0, 2 * np.pi, 2)
    f = amplitude * (np.sin(2 * np.pi * (x + y) + p[0]) + 0.7 * np.cos(2 * np.pi * (2 * y - x) + p[1]))
    f += 0.02 * amplitude * rng.normal(size=x.shape)
    return f.astype(np.float32)


def inputs(n, tex_shape, seed=3):
    """upstream gradients and tangents: gout, dtex, duv, db, ddu, ddv (float32)"""
    rng = np.random.default_rng(seed)
    x = types.SimpleNamespace()
    x.gout = rng.normal(size=(3, n)).astype(np.float32)
    x.dtex = rng.normal(size=tex_shape).astype(np.float32)
    x.duv = (0.01 * rng.normal(size=(2, n))).astype(np.float32)
    x.db, x.ddu, x.ddv = (rng.normal(size=(3, n)).astype(np.float32) for _ in range(3))
    return x


TEXTURES = ((37, 29), (16, 8))          # (TW, TH): not commensurate with the film of the scenes
SCALES = (1.0, 2.5)
KEYS = ("N", "dN", "grad_sh_n", "grad_dp_du", "grad_dp_dv", "grad_uv", "grad_tex")
# the maxima of profiles/bumpmap/f32_error.json (scripts/bumpmap_f32_error.py: this restatement in float32 against itself
# in float64 on the scenes of tests/test_gpu_bumpmap.py) per texture and scale -- the slopes are multiplied by TW, TH and
# scale, and the figures grow with them --, the third digit rounded up; the GPU is allowed four times that, the project's
# standing margin for another operation order.  tests/test_bumpmap_ref.py holds them to the record
F32 = {
    "37x29/1": {"N": 1.80e-7, "dN": 1.43e-6, "grad_sh_n": 2.69e-7, "grad_dp_du": 2.37e-7, "grad_dp_dv": 2.76e-7, "grad_uv": 1.99e-7,
                "grad_tex": 7.77e-7},
    "37x29/2.5": {"N": 3.62e-7, "dN": 1.46e-6, "grad_sh_n": 3.01e-7, "grad_dp_du": 3.57e-7, "grad_dp_dv": 3.54e-7, "grad_uv": 2.47e-7,
                  "grad_tex": 7.77e-7},
    "16x8/1": {"N": 1.82e-7, "dN": 2.21e-7, "grad_sh_n": 3.33e-7, "grad_dp_du": 3.34e-7, "grad_dp_dv": 2.73e-7, "grad_uv": 2.46e-7,
               "grad_tex": 2.00e-7},
    "16x8/2.5": {"N": 1.85e-7, "dN": 2.02e-7, "grad_sh_n": 2.75e-7, "grad_dp_du": 2.58e-7, "grad_dp_dv": 2.62e-7, "grad_uv": 3.01e-7,
                 "grad_tex": 2.08e-7},
}
TOL = {k: {q: 4 * v for q, v in d.items()} for k, d in F32.items()}


def table_key(TW, TH, scale):
    return "%dx%d/%g" % (TW, TH, scale)


def oracle_records(sc, oracle, face_normals):
    """the oracle's records of a scene of tests/row_scenes.py that the map reads: a dict with uv, sh_n, n, dp_du, dp_dv
    (float32) and the hit mask; smooth shading normals from smooth_ref (lighting_scenes.smooth_normals)"""
    import lighting_scenes as LS
    f = LS.oracle_field(sc, oracle)
    t, u, v, prim = f.ray_intersect_preliminary(sc.rays)
    rec = f.compute_surface_interaction(sc.rays, t, u, v, prim, oracle.RAY_ALL)
    hit = np.isfinite(t)
    sh = rec["sh_n"] if face_normals else LS.smooth_normals(sc, sc.rays, prim, hit).astype(np.float32)
    return {"uv": rec["uv"], "sh_n": sh, "n": rec["n"], "dp_du": rec["dp_du"], "dp_dv": rec["dp_dv"], "hit": hit}


def record_args(rec):
    return rec["uv"], rec["sh_n"], rec["n"], rec["dp_du"], rec["dp_dv"]


def shares(state, hit):
    """what the tests assert before anything is compared: the share of hit samples near a cell edge, the samples within a
    factor of two of the pass-through threshold, the share of perturbed hits, the smallest |<n_geo, c / |c|>| and how many
    hits have sigma = -1"""
    return {"near_edge": float(near_edge(state)[hit].mean()), "near_threshold": int(near_threshold(state)[hit].sum()),
            "perturbed_of_hits": float(state.pert[hit].mean()), "min_cosine": float(np.abs(state.cosine[hit]).min()),
            "sigma_negative": int((state.sigma[hit] < 0).sum())}


def conditions(sh, cap):
    """the conditions on the GPU test's inputs (asserted on the oracle's records on the CPU and on the GPU's own there)"""
    assert sh["near_edge"] <= cap, sh
    assert sh["near_threshold"] == 0 and sh["perturbed_of_hits"] == 1.0 and sh["min_cosine"] >= SIGMA_MIN, sh


def evaluate(tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale, x, keep, dtype=np.float64):
    """forward, tangent and adjoint under the inputs x: a dict in errors()' names.  `keep`: the lanes that are compared (a
    lane near a cell edge, where the slopes jump, gets zero tangents and a zero upstream gradient)"""
    a = (tex, uv, b, n_geo, dp_du, dp_dv, active, wrap, scale)
    N, mask, _ = forward(*a, dtype)
    dN = tangent(*a, x.dtex, x.duv * keep, x.db * keep, x.ddu * keep, x.ddv * keep, dtype)
    g = adjoint(*a, x.gout * keep, dtype)
    return {"N": N, "mask": mask, "dN": dN, "grad_uv": g.guv, "grad_sh_n": g.gn, "grad_dp_du": g.gpu, "grad_dp_dv": g.gpv,
            "grad_tex": g.gtex}


def errors(got, ref, keep):
    """per component as err_abs on the kept lanes, grad_tex as a relative L2"""
    out = {k: err_abs(np.asarray(got[k])[:, keep], np.asarray(ref[k])[:, keep]) for k in KEYS[:-1]}
    out["grad_tex"] = err_l2(got["grad_tex"], ref["grad_tex"])
    return out

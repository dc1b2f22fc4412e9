"""The normal map (include/hf.h hf_normalmap_*) restated in numpy from the formulas of the header, not from the kernel: the
lookup of the three planes at pos = (u TW, v TH) (refract_ref.lookup: the bitmap's cell, weights and slopes under both
wraps), the tangent-space normal m = (2 c - 1) / |2 c - 1|, the base frame s0 = normalize(dp_du - b <b, dp_du>),
t0 = b x s0, the result N = s0 m_x + t0 m_y + b m_z, the perturbed / pass-through decision, the tangent with respect to
the texels, uv, sh_n and dp_du, and an adjoint written on its own as a reverse sweep.  float64 by default;
`dtype=np.float32` evaluates the same text in float32.  All arrays are [3, n] / [2, n] / [n]; tex is [3, TH, TW].  A
helper module."""
import types

import numpy as np

import refract_ref as RR
from refract_ref import CLAMP, REPEAT  # noqa: F401

WRAPS = {"clamp": CLAMP, "repeat": REPEAT}
M2_MIN = 1e-12          # |2 c - 1|^2 below it: a texel that names no direction
A2_MIN = 1e-12          # |a|^2 below it times |dp_du|^2: dp_du parallel to b
MARGIN = 1e-5           # a position in the cell within it of a cell edge: another rounding of pos may read the next cell


def _dot(x, y):
    return (x * y).sum(0)


def _cross(x, y):
    return np.stack([x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]])


def positions(uv, TW, TH, dtype=np.float64):
    """pos [2, n] = (u TW, v TH)"""
    uv = np.asarray(uv, dtype)
    return np.stack([uv[0] * dtype(TW), uv[1] * dtype(TH)])


def cells(tex, uv, wrap, dtype=np.float64):
    """the three planes' lookups (refract_ref.lookup) at the positions of uv"""
    TH, TW = tex.shape[1:]
    pos = positions(uv, TW, TH, dtype)
    return [RR.lookup(tex[k], pos, wrap, dtype) for k in range(3)], pos


def shade(c, read, b, dp_du, active=None, dtype=np.float64):
    """the frame algebra from the three lookups c [3, n] (`read`: the lookup read something): a namespace with N, the mask
    `pert`, the frame and the two quantities the pass-through thresholds are about (M2 = |2 c - 1|^2, ratio = |a|^2 / |dp_du|^2)"""
    c, b, u = (np.asarray(x, dtype) for x in (c, b, dp_du))
    n = b.shape[1]
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    s = types.SimpleNamespace(b=b, u=u)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        finite = np.isfinite(b).all(0) & np.isfinite(u).all(0)
        mt = dtype(2) * c - dtype(1)
        s.M2 = _dot(mt, mt)
        s.bu = _dot(b, u)
        a = u - b * s.bu
        A2, U2 = _dot(a, a), _dot(u, u)
        s.ratio = A2 / np.where(U2 > 0, U2, dtype(1))
        s.pert = act & finite & np.asarray(read, bool) & (s.M2 >= dtype(M2_MIN)) & (U2 > 0) & (A2 >= dtype(A2_MIN) * U2)
        safe = lambda x: np.where(s.pert, x, dtype(1))
        s.M, s.A = np.sqrt(safe(s.M2)), np.sqrt(safe(A2))
        s.m = np.where(s.pert, mt / s.M, dtype(0))
        s.s0 = np.where(s.pert, a / s.A, dtype(0))
        s.t0 = _cross(b, s.s0)
        N = s.s0 * s.m[0] + s.t0 * s.m[1] + b * s.m[2]
    s.N = np.where(s.pert, N, b)
    return s


def _state(tex, uv, b, dp_du, active, wrap, dtype):
    tex = np.asarray(tex, dtype)
    e, pos = cells(tex, uv, wrap, dtype)
    with np.errstate(invalid="ignore"):
        read = e[0].ok & np.isfinite(np.asarray(uv, np.float64)).all(0)
    s = shade(np.stack([q.L for q in e]), read, b, dp_du, active, dtype)
    s.e, s.pos, s.tex = e, pos, tex
    return s


def forward(tex, uv, b, dp_du, active=None, wrap=REPEAT, dtype=np.float64):
    """(N [3, n], mask [n] bool, the state)"""
    s = _state(tex, uv, b, dp_du, active, wrap, dtype)
    return s.N, s.pert, s


@np.errstate(invalid="ignore", over="ignore")      # (the pass-through lanes: their numbers are not used)
def tangent(tex, uv, b, dp_du, active, wrap, dtex=None, duv=None, db=None, ddp=None, dtype=np.float64):
    """dN [3, n] with the cell and the decision held; a tangent that is None is zero"""
    s = _state(tex, uv, b, dp_du, active, wrap, dtype)
    n = s.b.shape[1]
    TH, TW = s.tex.shape[1:]
    z3 = np.zeros((3, n), dtype)
    db = z3 if db is None else np.asarray(db, dtype)
    ddp = z3 if ddp is None else np.asarray(ddp, dtype)
    dc = np.zeros((3, n), dtype)
    for k in range(3):
        if dtex is not None:
            dc[k] += (s.e[k].b * np.asarray(dtex, dtype)[k].ravel()[s.e[k].idx]).sum(0)
        if duv is not None:
            dc[k] += s.e[k].Lx * (dtype(TW) * np.asarray(duv, dtype)[0]) + s.e[k].Ly * (dtype(TH) * np.asarray(duv, dtype)[1])
    dmt = dtype(2) * dc
    dm = (dmt - s.m * _dot(s.m, dmt)) / s.M
    da = ddp - db * s.bu - s.b * (_dot(db, s.u) + _dot(s.b, ddp))
    ds0 = (da - s.s0 * _dot(s.s0, da)) / s.A
    dt0 = _cross(db, s.s0) + _cross(s.b, ds0)
    dN = ds0 * s.m[0] + dt0 * s.m[1] + db * s.m[2] + s.s0 * dm[0] + s.t0 * dm[1] + s.b * dm[2]
    return np.where(s.pert, dN, db)


@np.errstate(invalid="ignore", over="ignore")      # (the pass-through lanes: their numbers are not used)
def adjoint(tex, uv, b, dp_du, active, wrap, gout, dtype=np.float64):
    """the reverse sweep from gout = dL/dN [3, n]: a namespace with gtex [3, TH, TW], guv [2, n], gn, gp [3, n]"""
    s = _state(tex, uv, b, dp_du, active, wrap, dtype)
    TH, TW = s.tex.shape[1:]
    g = np.where(s.pert, np.asarray(gout, dtype), dtype(0))
    # N = s0 m_x + t0 m_y + b m_z
    s0_bar, t0_bar, b_bar = g * s.m[0], g * s.m[1], g * s.m[2]
    m_bar = np.stack([_dot(s.s0, g), _dot(s.t0, g), _dot(s.b, g)])
    # t0 = b x s0
    b_bar = b_bar + _cross(s.s0, t0_bar)
    s0_bar = s0_bar + _cross(t0_bar, s.b)
    # s0 = a / |a|
    a_bar = (s0_bar - s.s0 * _dot(s.s0, s0_bar)) / s.A
    # a = u - b <b, u>
    ab = _dot(a_bar, s.b)
    u_bar = a_bar - s.b * ab
    b_bar = b_bar - a_bar * s.bu - s.u * ab
    # m = mt / |mt|, mt = 2 c - 1
    c_bar = dtype(2) * (m_bar - s.m * _dot(s.m, m_bar)) / s.M
    out = types.SimpleNamespace(gtex=np.zeros((3, TH * TW), dtype), guv=np.zeros((2, b_bar.shape[1]), dtype))
    for k in range(3):
        for j in range(4):
            np.add.at(out.gtex[k], s.e[k].idx[j], np.where(s.pert, s.e[k].b[j] * c_bar[k], dtype(0)))
        out.guv[0] += dtype(TW) * s.e[k].Lx * c_bar[k]
        out.guv[1] += dtype(TH) * s.e[k].Ly * c_bar[k]
    out.gtex = out.gtex.reshape(3, TH, TW)
    out.guv = np.where(s.pert, out.guv, dtype(0))
    out.gn = np.where(s.pert, b_bar, np.asarray(gout, dtype))
    out.gp = np.where(s.pert, u_bar, dtype(0))
    return out


def near_edge(state, margin=MARGIN):
    """lanes whose position in the cell is within `margin` of a cell edge on either axis"""
    e = state.e[0]
    fx, fy = np.asarray(e.fx, np.float64), np.asarray(e.fy, np.float64)
    return (np.minimum(fx, 1 - fx) < margin) | (np.minimum(fy, 1 - fy) < margin)


def near_threshold(state):
    """lanes within a factor of two of either pass-through threshold"""
    with np.errstate(invalid="ignore"):
        return ((state.M2 > 0.5 * M2_MIN) & (state.M2 < 2 * M2_MIN)) | ((state.ratio > 0.5 * A2_MIN) & (state.ratio < 2 * A2_MIN))


def encode(m):
    return 0.5 * (np.asarray(m, np.float64) + 1.0)


def decode(tex):
    mt = 2.0 * np.asarray(tex, np.float64) - 1.0
    return mt / np.linalg.norm(mt, axis=0, keepdims=True)


def texture(TW, TH, seed=0, tilt=0.6):
    """[3, TH, TW] float32: a smooth field of unit normals tilted by up to about `tilt` plus a little noise, encoded"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid((np.arange(TH) + 0.5) / TH, (np.arange(TW) + 0.5) / TW, indexing="ij")
    mx = tilt * np.sin(2 * np.pi * (x + 0.3 * y)) + 0.1 * rng.normal(size=x.shape)
    my = tilt * np.cos(2 * np.pi * (1.5 * y - 0.2 * x)) + 0.1 * rng.normal(size=x.shape)
    m = np.stack([mx, my, np.ones_like(mx)])
    return encode(m / np.linalg.norm(m, axis=0)).astype(np.float32)


def flat(TW, TH):
    t = np.empty((3, TH, TW), np.float32)
    t[0:2], t[2] = 0.5, 1.0
    return t


def inputs(n, tex_shape, seed=3):
    """upstream gradients and tangents: gout, dtex, duv, db, ddp (float32)"""
    rng = np.random.default_rng(seed)
    x = types.SimpleNamespace()
    x.gout = rng.normal(size=(3, n)).astype(np.float32)
    x.dtex = rng.normal(size=tex_shape).astype(np.float32)
    x.duv = (0.01 * rng.normal(size=(2, n))).astype(np.float32)
    x.db, x.ddp = rng.normal(size=(3, n)).astype(np.float32), rng.normal(size=(3, n)).astype(np.float32)
    return x


TEXTURES = ((37, 29), (16, 8))          # (TW, TH): not commensurate with the film of the scenes
# the maxima of profiles/normalmap/f32_error.json (scripts/normalmap_f32_error.py: this restatement in float32 against
# itself in float64 on the scenes of tests/test_gpu_normalmap.py), the fourth digit rounded up; the GPU is allowed four
# times that, the project's standing margin for another operation order.  tests/test_normalmap_ref.py holds them to the record
F32 = {"N": 1.03e-6, "dN": 1.97e-6, "grad_sh_n": 6.69e-7, "grad_dp_du": 3.55e-7, "grad_uv": 1.50e-6, "grad_tex": 1.14e-6}
TOL = {k: 4 * v for k, v in F32.items()}


def oracle_records(sc, oracle, face_normals):
    """the oracle's records of a scene of tests/row_scenes.py that the map reads: a dict with uv, sh_n, dp_du (float32)
    and the hit mask; smooth shading normals from smooth_ref (lighting_scenes.smooth_normals)"""
    import lighting_scenes as LS
    f = LS.oracle_field(sc, oracle)
    t, u, v, prim = f.ray_intersect_preliminary(sc.rays)
    rec = f.compute_surface_interaction(sc.rays, t, u, v, prim, oracle.RAY_ALL)
    hit = np.isfinite(t)
    sh = rec["sh_n"] if face_normals else LS.smooth_normals(sc, sc.rays, prim, hit).astype(np.float32)
    return {"uv": rec["uv"], "sh_n": sh, "dp_du": rec["dp_du"], "hit": hit}


def shares(state, hit):
    """the shares the tests assert before anything is compared: hit samples near a cell edge, and samples within a factor
    of two of a pass-through threshold"""
    return {"near_edge": float(near_edge(state)[hit].mean()), "near_threshold": int(near_threshold(state)[hit].sum()),
            "perturbed_of_hits": float(state.pert[hit].mean())}


def err_abs(got, ref):
    """the largest difference over max(1, the largest value)"""
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def err_l2(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / np.linalg.norm(ref))


def evaluate(tex, uv, b, dp_du, active, wrap, x, keep, dtype=np.float64):
    """forward, tangent and adjoint under the inputs x: a dict in errors()' names.  `keep`: the lanes whose duv enters dN
    (a lane near a cell edge gets a zero duv)"""
    N, mask, _ = forward(tex, uv, b, dp_du, active, wrap, dtype)
    dN = tangent(tex, uv, b, dp_du, active, wrap, x.dtex, x.duv * keep, x.db, x.ddp, dtype)
    g = adjoint(tex, uv, b, dp_du, active, wrap, x.gout, dtype)
    return {"N": N, "mask": mask, "dN": dN, "grad_uv": g.guv, "grad_sh_n": g.gn, "grad_dp_du": g.gp, "grad_tex": g.gtex}


def errors(got, ref, keep):
    """per component as err_abs (grad_uv on the kept lanes only), grad_tex as a relative L2"""
    out = {k: err_abs(got[k], ref[k]) for k in ("N", "dN", "grad_sh_n", "grad_dp_du")}
    out["grad_uv"] = err_abs(np.asarray(got["grad_uv"])[:, keep], np.asarray(ref["grad_uv"])[:, keep])
    out["grad_tex"] = err_l2(got["grad_tex"], ref["grad_tex"])
    return out

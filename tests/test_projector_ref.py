"""The projector row's restatement (tests/projector_ref.py) held against itself and against what it must reduce to, on the
CPU: the header's closed form G = <sh_n, c - p> / ref.z^3 against sample_direction's steps, the closed tangents against
extrapolated central differences in every variable and (for the directions that keep to_world rigid) against the chain
rule through the steps, the reverse sweep against the tangent, the irradiance on the axis, uv against the perspective
sensor's sample_direction and the value against a point light of the direction-dependent intensity pi scale I |ref|^3 /
ref.z^3."""
import numpy as np
import pytest

import projector_ref as P
import sensor_ref as SR
from oracle import hf_oracle as O

TW, TH = P.TEX
N = 96


def _points(pr, n=N, seed=3):
    """points inside the frustum (uv in [0.05, 0.95]^2, depth 0.8 .. 2.5), away from the borders of the lookup's cells,
    unit normals that face the projector, float32 values"""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, [[TW], [TH]], (2, n))
    uv = (cell + rng.uniform(0.55, 1.45, (2, n))) / np.array([[TW], [TH]])   # texel coordinate = cell + 0.5 + (0.05 .. 0.95)
    uv = np.clip(uv, 0.05, 0.95)
    z = rng.uniform(0.8, 2.5, n)
    tau, a = np.tan(pr.fov * np.pi / 360), TW / TH
    ref = np.stack([(1 - 2 * uv[0]) * tau, (1 - 2 * uv[1]) * tau / a, np.ones(n)]) * z
    p = (pr.to_world[:, :3] @ ref + pr.to_world[:, 3:4]).astype(np.float32)
    u = pr.to_world[:, 3:4] - p
    sn = u / np.linalg.norm(u, axis=0) + 0.4 * rng.standard_normal((3, n))
    sn = (sn / np.linalg.norm(sn, axis=0)).astype(np.float32)
    keep = ((sn * u).sum(0) > 0.05) & ~P.near_border(np.stack([uv[0] * TW, uv[1] * TH]), 0.02)
    return p[:, keep], sn[:, keep]


@pytest.fixture(scope="module", params=sorted(P.PROJECTORS))
def case(request):
    pr = P.PROJECTORS[request.param]()
    p, sn = _points(pr)
    tex = P.textures(TW, TH)["random"]
    x = P.inputs(p.shape[1], 1, (TH, TW))
    return pr, p, sn, np.asarray(tex, np.float32), x


@pytest.mark.parametrize("wrap", (P.CLAMP, P.REPEAT))
def test_closed_form_is_the_steps_value(case, wrap):
    pr, p, sn, tex, x = case
    vis = np.ones(p.shape[1], bool)
    for t in (tex, None):
        value, _, uv = P.steps(pr, p, sn, x.w, t, wrap, P.ALBEDO)
        _, closed, cuv = P.forward(pr, p, sn, x.w, t, wrap, P.ALBEDO, vis)
        assert P.mapping(pr, p).lit.all()
        assert np.abs(closed / value - 1).max() <= 1e-13
        assert np.array_equal(uv, cuv)


def _rigid(pr, seed):
    """a tangent of to_world that keeps it rigid: dA = [w]x A, any dc"""
    rng = np.random.default_rng(seed)
    w, dc = rng.standard_normal(3), rng.standard_normal(3)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.concatenate([W @ pr.to_world[:, :3], dc[:, None]], axis=1).reshape(-1)


def test_tangent_in_rigid_directions_is_the_chain_rule_through_the_steps(case):
    pr, p, sn, tex, x = case
    vis = np.ones(p.shape[1], bool)
    for seed in (1, 2):
        kw = dict(dn=x.dn, dp=x.dp, dw=x.dw, dtex=x.dtex, d_to_world=_rigid(pr, seed), d_fov=0.7, d_scale=-0.4)
        _, dv, _ = P.steps(pr, p, sn, x.w, tex, P.REPEAT, P.ALBEDO, **kw)
        _, closed = P.tangent(pr, p, sn, x.w, tex, P.REPEAT, P.ALBEDO, vis, **kw)
        assert np.abs(closed - dv).max() <= 1e-12 * max(1.0, np.abs(dv).max())


def _extrapolated(f, h=1e-3):
    """central differences at h and h / 2, Richardson-extrapolated: the error is O(h^4)"""
    d1, d2 = (f(h) - f(-h)) / (2 * h), (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


def test_tangent_against_central_differences_in_every_variable(case):
    pr, p, sn, tex, x = case
    n = p.shape[1]
    vis = np.ones(n, bool)
    p64, sn64, w64, tex64 = (np.asarray(a, np.float64) for a in (p, sn, x.w, tex))
    rng = np.random.default_rng(9)
    dirs = {"dn": rng.standard_normal((3, n)), "dp": 0.2 * rng.standard_normal((3, n)), "dw": rng.standard_normal(n),
            "dtex": rng.standard_normal((TH, TW)), "d_to_world": 0.3 * rng.standard_normal(12), "d_fov": 0.7, "d_scale": -0.4}

    def value(name, s):
        q = P.projector(pr.to_world + (s * dirs["d_to_world"].reshape(3, 4) if name == "d_to_world" else 0),
                        pr.fov + (s * dirs["d_fov"] if name == "d_fov" else 0), 1.0, pr.res)
        q.scale = pr.scale + (s * dirs["d_scale"] if name == "d_scale" else 0)
        return P.forward(q, p64 + (s * dirs["dp"] if name == "dp" else 0), sn64 + (s * dirs["dn"] if name == "dn" else 0),
                         w64 + (s * dirs["dw"] if name == "dw" else 0), tex64 + (s * dirs["dtex"] if name == "dtex" else 0),
                         P.REPEAT, P.ALBEDO, vis)[1]

    for name, direction in dirs.items():
        _, dv = P.tangent(pr, p64, sn64, w64, tex64, P.REPEAT, P.ALBEDO, vis, **{name: direction})
        fd = _extrapolated(lambda s: value(name, s), 2e-4)
        assert np.abs(dv - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), name


@pytest.mark.parametrize("textured", (True, False))
def test_adjoint_is_the_transpose_of_the_tangent(case, textured):
    pr, p, sn, tex, x = case
    n = p.shape[1]
    vis = np.random.default_rng(4).random(n) < 0.8
    t = tex if textured else None
    spp = 1
    _, dv = P.tangent(pr, p, sn, x.w, t, P.CLAMP, P.ALBEDO, vis, spp, dn=x.dn, dp=x.dp, dw=x.dw, dtex=x.dtex if textured else None,
                      d_to_world=x.dtw, d_fov=x.dfov, d_scale=x.dscale)
    g = P.adjoint(pr, p, sn, x.w, t, P.CLAMP, P.ALBEDO, vis, spp, grad_image=x.gi, grad_value=x.gv)
    f64 = lambda a: np.asarray(a, np.float64)
    lhs = (dv * (f64(x.gi) + f64(x.gv))).sum()
    rhs = (g.gn * f64(x.dn)).sum() + (g.gp * f64(x.dp)).sum() + (g.gw * f64(x.dw)).sum() + \
        g.g14 @ np.concatenate([f64(x.dtw), [float(x.dfov), float(x.dscale)]])
    if textured:
        rhs += (g.gtex * f64(x.dtex)).sum()
    scale = np.abs(dv * (f64(x.gi) + f64(x.gv))).sum()
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert not g.gn[:, ~vis].any() and not g.gp[:, ~vis].any() and not g.gw[~vis].any()
    # the sums over a slice of the rows are the slice's own
    part = P.adjoint(pr, p[:, :40], sn[:, :40], x.w[:40], t, P.CLAMP, P.ALBEDO, vis[:40], spp, grad_image=x.gi[:40], grad_value=x.gv[:40])
    rows = P.adjoint(pr, p, sn, x.w, t, P.CLAMP, P.ALBEDO, vis, spp, grad_image=x.gi, grad_value=x.gv, rows=slice(0, 40))
    assert np.allclose(part.g14, rows.g14, rtol=1e-12, atol=1e-14)


def test_irradiance_on_the_axis_at_distance_one():
    """a surface at z = 1 on the axis that faces the projector receives the irradiance scale I(1/2, 1/2): its value is
    albedo / pi times pi scale I"""
    for name in sorted(P.PROJECTORS):
        pr = P.PROJECTORS[name]()
        A, c = pr.to_world[:, :3], pr.to_world[:, 3]
        p = (c + A[:, 2])[:, None]
        sn = -A[:, 2:3]
        tex = np.arange(TW * TH, dtype=np.float64).reshape(TH, TW) / 10 + 1
        I = P.R.lookup(tex, np.array([[TW / 2], [TH / 2]]), P.CLAMP).L[0]
        value, _, uv = P.steps(pr, p, sn, None, tex, P.CLAMP, P.ALBEDO)
        assert np.allclose(uv[:, 0], 0.5, atol=1e-14)
        assert abs(value[0] - P.ALBEDO * pr.scale * I) <= 1e-13 * abs(value[0])
        assert abs(P.steps(pr, p, sn, None, None, P.CLAMP, 1.0)[0][0] - pr.scale) <= 1e-13


def test_uv_is_the_perspective_sensors_film_position(case):
    pr, p, _, _, _ = case
    s = SR.sensor(SR.PERSPECTIVE, pr.to_world, pr.fov, (TW, TH), None, 1e-2, 1e4)
    film = SR.project(s, p).uv
    closed, _ = SR.closed_project(s, np.asarray(p, np.float64))
    uv = P.mapping(pr, p).uv
    assert np.abs(uv * np.array([[TW], [TH]]) - film).max() <= 1e-12
    assert np.abs(uv * np.array([[TW], [TH]]) - closed).max() <= 1e-12


def test_value_is_a_point_lights_of_the_direction_dependent_intensity(case):
    """exact, not a bound: albedo / pi (intensity / r^2) <sh_n, u> / r with intensity = pi scale I |ref|^3 / ref.z^3"""
    pr, p, sn, tex, _ = case
    n = p.shape[1]
    vis = np.ones(n, bool)
    _, value, _ = P.forward(pr, p, sn, None, tex, P.REPEAT, P.ALBEDO, vis)
    m = P.mapping(pr, p)
    I = P.texel(pr, m, tex, P.REPEAT, np.float64).L
    intensity = np.pi * pr.scale * I * np.linalg.norm(m.ref, axis=0) ** 3 / m.ref[2] ** 3
    d, t = -np.asarray(sn, np.float64), np.ones(n)
    for i in range(0, n, 7):
        light = np.append(pr.to_world[:, 3], intensity[i])
        ref = O.point_lighting(sn[:, i:i + 1], p[:, i:i + 1], d[:, i:i + 1], t[i:i + 1], light, albedo=P.ALBEDO)[0, 0]
        assert abs(value[i] - ref) <= 1e-13 * abs(ref)


def test_masks_and_rays_of_a_handful_of_lanes():
    """lanes behind the projector, outside the frustum, facing away and missed are not traced; a traced lane's ray ends just
    short of the pinhole"""
    pr = P.PROJECTORS["above"]()
    A, c = pr.to_world[:, :3], pr.to_world[:, 3]
    inside = c + 1.5 * A[:, 2]
    p = np.stack([inside, c - 1.0 * A[:, 2], c + 1.5 * A[:, 2] + 2.0 * A[:, 0], inside, inside], axis=1).astype(np.float32)
    to_c = (c - inside) / np.linalg.norm(c - inside)
    sn = np.stack([to_c, to_c, to_c, -to_c, to_c], axis=1).astype(np.float32)
    d = -sn
    d[:, 3] = sn[:, 3]          # (seen from the front, but the normal faces away from the projector)
    t = np.array([1, 1, 1, 1, np.inf], np.float32)
    tr, unsure = P.traced(pr, p, sn, d, t)
    assert tr.tolist() == [True, False, False, False, False] and not unsure.any()
    o, w, maxt, tr2 = P.rays(pr, p, sn, sn, d, t)
    assert np.array_equal(tr, tr2) and (maxt[1:] == -1).all() and not o[:, 1:].any() and not w[:, 1:].any()
    assert abs(np.linalg.norm(o[:, 0] + w[:, 0] * maxt[0] / (1 - P.SHADOW_EPSILON) - c.astype(np.float32))) <= 1e-12
    uv = P.forward(pr, p, sn, None, None, P.CLAMP, 1.0, tr)[2]
    assert not uv[:, 1].any() and np.allclose(uv[:, 0], 0.5, atol=1e-6)

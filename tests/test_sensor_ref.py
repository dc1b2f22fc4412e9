"""The sensor's restatement (tests/sensor_ref.py) on the CPU: the header's closed forms against the reference's route
through the five matrices and numpy.linalg.inv, the tangents against extrapolated central differences, the way back
against the way out, the geometry of the field of view, the normalisation of the importance, and the orthographic
restatement against workload.ortho_rays bit for bit; the restated adjoints, reverse sweeps written on their own, against
the restated tangents (transposition, 1e-12)."""
import numpy as np
import pytest
import torch

import sensor_ref as R

FILM, CROP = (13, 7), (3, 2, 5, 4)
POSE = R.look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0))
ORTHO_POSE = POSE @ np.diag([0.9, 0.7, 1.0, 1.0])
FOV = 38.0


def _sensor(type_, crop=CROP, **kw):
    return R.sensor(type_, ORTHO_POSE if type_ == R.ORTHOGRAPHIC else POSE, None if type_ == R.ORTHOGRAPHIC else FOV, FILM, crop, **kw)


def _pos(s, spp=5, seed=3, count=1000):
    n = s.crop[2] * s.crop[3] * spp
    return R.film_positions(s, np.arange(n, dtype=np.uint64)[:count], spp, seed)


def _direction(rng):
    return rng.standard_normal(12) * 0.3, 0.7


@pytest.mark.parametrize("type_", [R.PERSPECTIVE, R.ORTHOGRAPHIC])
@pytest.mark.parametrize("crop", [CROP, None])
def test_closed_forms_equal_the_matrices(type_, crop):
    s = _sensor(type_, crop)
    pos = _pos(s, spp=50 if crop else 11)
    assert pos.shape[1] == 1000
    assert pos[0].min() >= s.crop[0] and pos[0].max() < s.crop[0] + s.crop[2] and pos[1].min() >= s.crop[1]
    o, d, maxt, _, _ = R.rays(s, pos)
    co, cd, cm = R.closed_rays(s, pos)
    gaps = np.abs(o - co).max(), np.abs(d - cd).max(), np.abs(maxt / cm - 1).max()
    print("closed form against matrices (o, d, maxt relative):", gaps)
    assert max(gaps) <= 1e-13, gaps


@pytest.mark.parametrize("type_", [R.PERSPECTIVE, R.ORTHOGRAPHIC])
def test_ray_tangent_equals_central_differences(type_):
    s = _sensor(type_)
    pos = _pos(s, count=200)
    dtw, dfov = _direction(np.random.default_rng(1))
    _, _, _, do, dd = R.rays(s, pos, np.float64, dtw, dfov)
    h = 1e-3

    def step(k):
        t = R.sensor(type_, s.to_world + k * h * dtw.reshape(3, 4), None if s.fov is None else s.fov + k * h * dfov, FILM, CROP)
        o, d, _, _, _ = R.rays(t, pos)
        return np.concatenate([o, d])
    fd = (4 * (step(1) - step(-1)) / (2 * h) - (step(2) - step(-2)) / (4 * h)) / 3
    got = np.concatenate([do, dd])
    assert np.abs(got - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), np.abs(got - fd).max()
    assert np.abs(do).max() > 1e-2 and np.abs(dd).max() > 1e-2
    if type_ == R.PERSPECTIVE:   # fov alone moves the rays; the orthographic type does not read it
        assert np.abs(R.rays(s, pos, np.float64, None, 1.0)[4]).max() > 1e-3
    else:
        assert not np.abs(R.rays(s, pos, np.float64, None, 1.0)[3]).any()


@pytest.mark.parametrize("type_", [R.PERSPECTIVE, R.ORTHOGRAPHIC])
@pytest.mark.parametrize("crop", [CROP, None])
def test_ray_adjoint_is_the_transpose_of_the_tangent(type_, crop):
    s = _sensor(type_, crop)
    pos = _pos(s, count=200)
    rng = np.random.default_rng(4)
    dtw, dfov = _direction(rng)
    go, gd = rng.standard_normal((3, pos.shape[1])), rng.standard_normal((3, pos.shape[1]))
    _, _, _, do, dd = R.rays(s, pos, np.float64, dtw, dfov)
    g12, gf = R.rays_adjoint(s, pos, go, gd)
    lhs, rhs = (do * go).sum() + (dd * gd).sum(), g12 @ dtw + gf * dfov
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    assert np.abs(g12).min() > 0 or type_ == R.ORTHOGRAPHIC
    assert (gf != 0) == (type_ == R.PERSPECTIVE)          # the orthographic type does not read x_fov


@pytest.mark.parametrize("crop", [CROP, None])
def test_project_adjoint_is_the_transpose_of_the_tangent(crop):
    s = _sensor(R.PERSPECTIVE, crop, near=0.05, far=50.0)
    rng = np.random.default_rng(5)
    p, _ = _points(s, rng)
    active = rng.random(p.shape[1]) < 0.9
    dtw, dfov = _direction(rng)
    dp = rng.standard_normal(p.shape) * 0.2
    r = R.project(s, p, active, np.float64, dp, dtw, dfov)
    assert r.valid.any() and (r.inside & ~r.valid).any() and (~r.inside).any()
    guv, gw = rng.standard_normal(r.uv.shape), rng.standard_normal(p.shape[1]) / r.weight
    gp, g12, gf = R.project_adjoint(s, p, active, guv, gw)
    lhs = (r.duv * guv * r.inside).sum() + (r.dweight * gw * r.valid).sum()
    rhs = (gp * dp).sum() + g12 @ dtw + gf * dfov
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    assert not gp[:, ~r.inside].any() and gf != 0 and np.abs(g12).min() > 0


def _points(s, rng, n=300):
    """world points in front of the sensor, some outside the crop window and the clip range"""
    pos = np.stack([rng.uniform(-2, FILM[0] + 2, n), rng.uniform(-2, FILM[1] + 2, n)])
    o, d, maxt, _, _ = R.rays(s, pos)
    return o + d * rng.uniform(-0.04, 1.0, n), pos


def test_project_tangent_equals_central_differences():
    s = _sensor(R.PERSPECTIVE, near=0.05, far=50.0)
    rng = np.random.default_rng(2)
    p, _ = _points(s, rng)
    dtw, dfov = _direction(rng)
    dp = rng.standard_normal(p.shape) * 0.2
    r = R.project(s, p, None, np.float64, dp, dtw, dfov)
    assert r.inside.any() and (~r.inside).any() and r.valid.any() and (r.inside & ~r.valid).any()
    h = 1e-3

    def step(k):
        t = R.sensor(R.PERSPECTIVE, s.to_world + k * h * dtw.reshape(3, 4), s.fov + k * h * dfov, FILM, CROP, 0.05, 50.0)
        q = R.project(t, p + k * h * dp)
        return np.concatenate([q.uv, q.weight[None]])
    fd = (4 * (step(1) - step(-1)) / (2 * h) - (step(2) - step(-2)) / (4 * h)) / 3
    got = np.concatenate([r.duv, r.dweight[None]])
    # the differences' own truncation is h^4 f^(5) / 30 with f ~ z^-3 and steps of 2 h |dp| = 4e-4 in z: at z >= 0.3 that
    # is (4e-4 / 0.3)^4 = 3e-12 of the value; nearer to the pinhole the differences, not the tangent, lose the digits
    m = r.ref[2] >= 0.3
    assert m.sum() > 150 and (m & r.valid).any() and (m & ~r.valid).any()
    scale = np.maximum(1.0, np.abs(fd[:, m]).max(1, keepdims=True))
    assert (np.abs(got - fd)[:, m] <= 1e-8 * scale).all(), (np.abs(got - fd)[:, m] / scale).max()
    m = r.ref[2] > 0.02
    cu, cw = R.closed_project(s, p)
    assert np.abs(cu - r.uv)[:, m].max() <= 1e-11 and np.abs(cw / r.weight - 1)[m].max() <= 1e-11


@pytest.mark.parametrize("crop", [CROP, None])
def test_projecting_a_point_of_a_ray_returns_its_film_position(crop):
    s = _sensor(R.PERSPECTIVE, crop)
    pos = _pos(s, spp=50 if crop else 11)
    o, d, maxt, _, _ = R.rays(s, pos)
    for t in (0.0, 0.37, 2.5):
        r = R.project(s, o + d * t)
        assert np.abs(r.uv - pos).max() <= 1e-12 * max(FILM), np.abs(r.uv - pos).max()
        assert r.valid.all()
    assert not R.project(s, o - d * 1e-3).inside.any()     # in front of the near plane


def test_field_of_view():
    """the centre of the film looks along A e_z; the rays through the middle of the film's right and top edges make
    atan(tau) and atan(tau / a) with it"""
    s = _sensor(R.PERSPECTIVE, None)
    W, H = FILM
    _, d, _, _, _ = R.rays(s, np.array([[W / 2, W, W / 2], [H / 2, H / 2, 0.0]]))
    z = s.to_world[:, 2]
    assert np.abs(d[:, 0] - z).max() <= 1e-14
    tau = np.tan(np.deg2rad(FOV / 2))
    ang = np.arccos(np.clip(z @ d[:, 1:], -1, 1))
    assert np.abs(ang - np.arctan([tau, tau / (W / H)])).max() <= 1e-12
    assert np.abs(np.linalg.norm(d, axis=0) - 1).max() <= 1e-14


@pytest.mark.parametrize("crop", [CROP, None])
def test_importance_integrates_to_one_over_the_crop_window(crop):
    """int importance(omega) d omega over the directions of the crop window = 1: on the plane at distance 1 d omega =
    cos^3 dA, so the integrand is the constant 1 / A' and the midpoint rule over the window is exact to rounding"""
    s = _sensor(R.PERSPECTIVE, crop)
    m = 64
    u = (np.arange(m) + 0.5) / m
    pos = np.stack([s.crop[0] + s.crop[2] * np.repeat(u, m), s.crop[1] + s.crop[3] * np.tile(u, m)])
    o, d, _, _, _ = R.rays(s, pos)
    r = R.project(s, o + d * 1.7)
    assert r.valid.all()
    imp = r.weight * np.linalg.norm(r.ref, axis=0) ** 2          # importance(local_d)
    corners = np.stack([[s.crop[0], s.crop[0] + s.crop[2]], [s.crop[1], s.crop[1] + s.crop[3]]])
    c = R.project(s, s.to_world[:, 3:4] + R.rays(s, corners)[1] * 2.0).ref
    area = abs(np.diff(c[0] / c[2])[0] * np.diff(c[1] / c[2])[0])      # the window on the plane at distance 1
    cos3 = (r.ref[2] / np.linalg.norm(r.ref, axis=0)) ** 3
    assert abs((imp * cos3).sum() * area / m ** 2 - 1.0) <= 1e-12


def test_orthographic_restatement_is_ortho_rays_bit_for_bit():
    import hf_amd
    W, H, spp, seed = 13, 7, 3, 5
    kw = dict(origin=(1.5, 1.2, 1.1), target=(0.0, 0.1, 0.125), up=(0.0, 0.0, 1.0), scale=(1.6, 1.3, 1.0))
    want = hf_amd.workload.ortho_rays(W, H, spp, "cpu", seed=seed, **kw).numpy()
    s = R.sensor(R.ORTHOGRAPHIC, R.look_at(kw["origin"], kw["target"], kw["up"]) @ np.diag(kw["scale"] + (1.0,)), None, (W, H))
    pos = R.film_positions(s, np.arange(W * H * spp, dtype=np.uint64), spp, seed)
    assert np.array_equal(pos.astype(np.float32), hf_amd.workload.film_positions(W, H, spp, "cpu", seed=seed).numpy())
    o, d, maxt = R.ortho_closed(s, pos)
    got = np.concatenate([o, d, maxt[None]]).astype(np.float32)
    assert np.array_equal(got, want), int((got != want).sum())
    # a shuffled pixel list draws the same samples
    pix = torch.randperm(W * H, generator=torch.Generator().manual_seed(0))[:20]
    ids = hf_amd.workload.ray_indices(W, H, spp, "cpu", pix).numpy().astype(np.uint64)
    sub = hf_amd.workload.ortho_rays(W, H, spp, "cpu", seed=seed, pixels=pix, **kw).numpy()
    o, d, maxt = R.ortho_closed(s, R.film_positions(s, ids, spp, seed))
    assert np.array_equal(np.concatenate([o, d, maxt[None]]).astype(np.float32), sub)

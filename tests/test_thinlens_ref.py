"""The thin lens's restatement (tests/thinlens_ref.py) on the CPU: the header's closed forms against the reference's
steps (the five matrices, numpy.linalg.inv, the concentric disk), the tangents against extrapolated central differences
in all 15 variables, the restated adjoints against the restated tangents, the way back against the way out, the focus
property, the pinhole limit against sensor_ref, and the disk's first two moments."""
import numpy as np
import pytest

import sensor_ref as R
import thinlens_ref as T

FILM, CROP, FOV, POSE = T.FILM, T.CROP, T.FOV, T.POSE


def _lens(crop=CROP, radius=0.3, focus=2.0, **kw):
    return T.lens(POSE, FOV, radius, focus, FILM, crop, **kw)


def _wave(s, spp=5, seed=3, count=1000):
    ids = np.arange(s.crop[2] * s.crop[3] * spp, dtype=np.uint64)[:count]
    return R.film_positions(s, ids, spp, seed), T.disk(T.aperture_samples(ids, seed))


def _direction(rng):
    return rng.standard_normal(12) * 0.3, 0.7, 0.4, -0.6


def _moved(s, k, h, dtw, dfov, dr, df, **kw):
    return T.lens(s.to_world + k * h * np.asarray(dtw).reshape(3, 4), s.fov + k * h * dfov, s.radius + k * h * dr,
                  s.focus + k * h * df, FILM, s.crop, s.near, s.far)


def _richardson(step, h):
    return (4 * (step(1) - step(-1)) / (2 * h) - (step(2) - step(-2)) / (4 * h)) / 3


@pytest.mark.parametrize("crop", [CROP, None])
@pytest.mark.parametrize("radius,focus", [(0.3, 2.0), (0.05, 0.5)])
def test_closed_forms_equal_the_steps(crop, radius, focus):
    s = _lens(crop, radius, focus)
    pos, D = _wave(s, spp=50 if crop else 11)
    assert pos.shape[1] == 1000
    o, d, maxt, _, _ = T.rays(s, pos, D)
    co, cd, cm = T.closed_rays(s, pos, D)
    gaps = np.abs(o - co).max(), np.abs(d - cd).max(), np.abs(maxt / cm - 1).max()
    print("closed form against the steps (o, d, maxt relative):", gaps)
    assert max(gaps) <= 1e-13, gaps
    p = o + d * np.random.default_rng(0).uniform(0.05, 3.0, pos.shape[1])
    r = T.project(s, p, D)
    cu, cw = T.closed_project(s, p, D)
    gaps = np.abs(cu - r.uv).max() / max(FILM), np.abs(cw / r.weight - 1).max()
    print("closed projection against the steps (uv over the film, weight relative):", gaps)
    assert max(gaps) <= 1e-13, gaps


def test_ray_tangent_equals_central_differences_in_every_variable():
    s = _lens()
    pos, D = _wave(s, count=200)
    h = 1e-3
    for j in range(15):
        dtw, dfov, dr, df = np.zeros(12), 0.0, 0.0, 0.0
        if j < 12:
            dtw[j] = 1.0
        else:
            dfov, dr, df = float(j == 12), float(j == 13), float(j == 14)
        _, _, _, do, dd = T.rays(s, pos, D, np.float64, dtw, dfov, dr, df)

        def step(k):
            o, d, _, _, _ = T.rays(_moved(s, k, h, dtw, dfov, dr, df), pos, D)
            return np.concatenate([o, d])
        fd = _richardson(step, h)
        got = np.concatenate([do, dd])
        assert np.abs(got - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), (j, np.abs(got - fd).max())
        assert np.abs(got).max() > 1e-4, j                 # every variable moves the rays


@pytest.mark.parametrize("crop", [CROP, None])
def test_ray_adjoint_is_the_transpose_of_the_tangent(crop):
    s = _lens(crop)
    pos, D = _wave(s, count=200)
    rng = np.random.default_rng(4)
    dtw, dfov, dr, df = _direction(rng)
    go, gd = rng.standard_normal((3, pos.shape[1])), rng.standard_normal((3, pos.shape[1]))
    _, _, _, do, dd = T.rays(s, pos, D, np.float64, dtw, dfov, dr, df)
    g12, gf, gr, gfo = T.rays_adjoint(s, pos, D, go, gd)
    lhs, rhs = (do * go).sum() + (dd * gd).sum(), g12 @ dtw + gf * dfov + gr * dr + gfo * df
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    assert np.abs(g12).min() > 0 and gf != 0 and gr != 0 and gfo != 0


def _points(s, rng, n=300):
    """world points on rays of the lens, lane i through ITS aperture point; some outside the window and the clip range"""
    pos = np.stack([rng.uniform(-2, FILM[0] + 2, n), rng.uniform(-2, FILM[1] + 2, n)])
    D = T.disk(T.aperture_samples(np.arange(n, dtype=np.uint64), 9))
    o, d, _, _, _ = T.rays(s, pos, D)
    return o + d * rng.uniform(-0.04, 1.0, n), D


def test_project_tangent_equals_central_differences_in_every_variable():
    s = _lens(near=0.05, far=50.0)
    rng = np.random.default_rng(2)
    p, D = _points(s, rng)
    dp0 = rng.standard_normal(p.shape) * 0.2
    h = 1e-3
    for j in range(16):                                    # 15 variables and p
        dtw, dfov, dr, df, dp = np.zeros(12), 0.0, 0.0, 0.0, np.zeros_like(p)
        if j < 12:
            dtw[j] = 1.0
        elif j < 15:
            dfov, dr, df = float(j == 12), float(j == 13), float(j == 14)
        else:
            dp = dp0
        r = T.project(s, p, D, None, np.float64, dp, dtw, dfov, dr, df)

        def step(k):
            q = T.project(_moved(s, k, h, dtw, dfov, dr, df), p + k * h * dp, D)
            return np.concatenate([q.uv, q.weight[None]])
        fd = _richardson(step, h)
        got = np.concatenate([r.duv, r.dweight[None]])
        # (as tests/test_sensor_ref.py: nearer than 0.3 the differences, not the tangent, lose the digits)
        m = r.ref[2] >= 0.3
        assert m.sum() > 150 and (m & r.valid).any() and (m & ~r.valid).any()
        scale = np.maximum(1.0, np.abs(fd[:, m]).max(1, keepdims=True))
        assert (np.abs(got - fd)[:, m] <= 1e-8 * scale).all(), (j, (np.abs(got - fd)[:, m] / scale).max())
        assert np.abs(got[:, m]).max() > 1e-4, j


@pytest.mark.parametrize("crop", [CROP, None])
def test_project_adjoint_is_the_transpose_of_the_tangent(crop):
    s = _lens(crop, near=0.05, far=50.0)
    rng = np.random.default_rng(5)
    p, D = _points(s, rng)
    active = rng.random(p.shape[1]) < 0.9
    dtw, dfov, dr, df = _direction(rng)
    dp = rng.standard_normal(p.shape) * 0.2
    r = T.project(s, p, D, active, np.float64, dp, dtw, dfov, dr, df)
    assert r.valid.any() and (r.inside & ~r.valid).any() and (~r.inside).any()
    guv, gw = rng.standard_normal(r.uv.shape), rng.standard_normal(p.shape[1]) / r.weight
    gp, g12, gf, gr, gfo = T.project_adjoint(s, p, D, active, guv, gw)
    lhs = (r.duv * guv * r.inside).sum() + (r.dweight * gw * r.valid).sum()
    rhs = (gp * dp).sum() + g12 @ dtw + gf * dfov + gr * dr + gfo * df
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    assert not gp[:, ~r.inside].any() and gf != 0 and gr != 0 and gfo != 0 and np.abs(g12).min() > 0


@pytest.mark.parametrize("crop", [CROP, None])
@pytest.mark.parametrize("radius,focus", T.LENSES)
def test_projecting_a_point_of_a_ray_returns_its_film_position(crop, radius, focus):
    s = _lens(crop, radius, focus)
    pos, D = _wave(s, spp=50 if crop else 11)
    o, d, _, _, _ = T.rays(s, pos, D)
    for t in (0.0, 0.37, 2.5):
        r = T.project(s, o + d * t, D)
        assert np.abs(r.uv - pos).max() <= 1e-12 * max(FILM), np.abs(r.uv - pos).max()
        assert r.valid.all()
    assert not T.project(s, o - d * 1e-3, D).inside.any()  # in front of the near plane


def test_every_aperture_draw_of_a_film_position_meets_the_focal_plane_in_one_point():
    s = _lens(None, 0.3, 2.0)
    pos = np.repeat(np.array([[4.3], [5.6]]), 64, axis=1)
    D = T.disk(T.aperture_samples(np.arange(64, dtype=np.uint64), 7))
    assert np.abs(D[:2]).max() > 0.8                       # the draws cover the aperture
    o, d, _, _, _ = T.rays(s, pos, D)
    A, c = s.to_world[:, :3], s.to_world[:, 3]
    oc, dc = A.T @ (o - c[:, None]), A.T @ d               # camera space (A is a rotation)
    hit = oc + dc * (s.focus - oc[2]) / dc[2]
    assert np.abs(hit - hit[:, :1]).max() <= 1e-12, np.abs(hit - hit[:, :1]).max()
    assert np.abs(hit[2] - s.focus).max() <= 1e-12
    away = oc + dc * (0.5 * s.focus - oc[2]) / dc[2]       # ... and in no other plane
    assert np.abs(away - away[:, :1]).max() > 0.1


@pytest.mark.parametrize("crop", [CROP, None])
def test_aperture_radius_zero_is_the_perspective_sensor(crop):
    s = _lens(crop, 0.0, 0.5, near=0.05, far=50.0)
    pos, D = _wave(s)
    dtw, dfov, _, _ = _direction(np.random.default_rng(6))
    got = T.rays(s, pos, D, np.float64, dtw, dfov)
    want = R.rays(T.pinhole(s), pos, np.float64, dtw, dfov)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-13 * max(1.0, np.abs(w).max())
    p, D = _points(s, np.random.default_rng(7))
    dp = np.random.default_rng(8).standard_normal(p.shape) * 0.2
    g = T.project(s, p, D, None, np.float64, dp, dtw, dfov)
    w = R.project(T.pinhole(s), p, None, np.float64, dp, dtw, dfov)
    assert np.array_equal(g.valid, w.valid) and np.array_equal(g.inside, w.inside)
    assert np.abs(g.uv - w.uv)[:, w.inside].max() <= 1e-13 * max(FILM)
    assert np.abs(g.weight / w.weight - 1)[w.inside].max() <= 1e-13
    assert np.abs(g.duv - w.duv)[:, w.inside].max() <= 1e-13 * max(1.0, np.abs(w.duv[:, w.inside]).max())


def test_disk_points_are_uniform_in_the_unit_disk():
    n = 100000
    D = T.disk(T.aperture_samples(np.arange(n, dtype=np.uint64), 1))
    r2 = D[0] ** 2 + D[1] ** 2
    assert r2.max() <= 1.0 and not D[2].any()
    # uniform in the disk: E x = 0, var x = 1/4; E r^2 = 1/2, var r^2 = 1/12; E xy = 0, var xy = E x^2 y^2 = 1/24
    for v, mean, var in ((D[0], 0.0, 0.25), (D[1], 0.0, 0.25), (r2, 0.5, 1 / 12), (D[0] * D[1], 0.0, 1 / 24),
                         (D[0] ** 2, 0.25, 1 / 8 - 1 / 16)):
        assert abs(v.mean() - mean) <= 4 * np.sqrt(var / n), (v.mean(), mean)
    # the samples are multiples of 2^-23 in [0, 1) and differ from the film jitter's
    smp = T.aperture_samples(np.arange(64, dtype=np.uint64), 3)
    assert smp.min() >= 0 and smp.max() < 1 and np.array_equal(smp * 2 ** 23, np.round(smp * 2 ** 23))
    s = _lens()
    jit = R.film_positions(s, np.arange(64, dtype=np.uint64), 1, 3) % 1.0
    assert not np.isclose(smp, jit).any()

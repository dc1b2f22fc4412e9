"""tests/medium_ref.py against itself (CPU, float64, no library): the derivatives of the restatement against central
differences with the bits held -- every parameter, t and weight, over both branches of u_out, u_in > 0 and u_in = 0 and
S = inf --, the known answer of a ray straight down under an overhead light, the exact zeros of a light that does not
shine in, and the transposition of tangent and adjoint."""
import copy

import numpy as np
import pytest

import medium_ref as R

K, SEED, SPP = 5, 3, 2
LIGHTS = [R.light((0.2, -0.1, 1.0), 2.0), R.light((1.0, 0.3, 0.4), 1.5)]


def _scene(n=96, seed=0):
    """samples of every kind: rays that enter from above (u_in > 0, u_out = t), start inside and go down (u_in = 0), start
    inside and go up and leave through the top (u_out = -h / c) or end before it (u_out = t), and misses (t = inf)"""
    rng = np.random.default_rng(seed)
    M = R.medium(0.7, 0.8, 0.35, top_origin=(0.1, -0.2, 1.0), top_normal=(0.1, 0.05, 1.0))
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.zeros(n)])
    d = rng.normal(size=(3, n)); d[2] = -np.abs(d[2]) - 0.3
    kind = np.arange(n) % 6
    o[2] = np.where(kind <= 1, rng.uniform(1.4, 2.0, n), rng.uniform(-0.5, 0.6, n))
    d[2] = np.where(kind >= 3, -d[2], np.where(kind <= 1, d[2] - 2.0, d[2]))   # kinds 3, 4, 5 go up; 0, 1 enter steeply
    d /= np.sqrt((d * d).sum(0))
    t = rng.uniform(2.5, 4.0, n)                                   # kinds 0, 2: a hit well inside
    t = np.where(kind == 4, 0.2, t)                                # up, ends before the top
    t = np.where((kind == 1) | (kind == 5), np.inf, t)             # misses: S = inf going down, the top going up
    q = R.segment(M, o, d, t)
    assert q.elig.all()
    assert ((q.u_in > 0) & q.at_t).any() and ((q.u_in == 0) & q.at_t & (q.c < 0)).any()
    assert (~q.at_t).any() and (q.at_t & (q.c > 0)).any() and np.isinf(q.S).any()
    bits = rng.integers(0, 1 << K, size=(len(LIGHTS), n)).astype(np.uint32)
    x = R.inputs(n, SPP, len(LIGHTS), seed=seed + 1)
    return M, o, d, t, bits, x


def _loss(M, lights, o, d, t, w, bits, x):
    image, value = R.forward(M, lights, o, d, t, w, bits, K, SEED, spp=SPP)
    return (image * x.gi).sum() + (value * x.gv).sum()


def _perturbed(M, lights, dp, eps):
    M2 = copy.deepcopy(M)
    M2.sigma_t += eps * dp[0]; M2.albedo += eps * dp[1]; M2.g += eps * dp[2]
    L2 = [R.light(L.to_light, 1.0) for L in lights]
    for j, (L, src) in enumerate(zip(L2, lights)):
        L.irradiance = src.irradiance + eps * dp[R.PARAMS + j]
    return M2, L2


def test_adjoint_matches_central_differences_of_every_input():
    M, o, d, t, bits, x = _scene()
    w = x.w.astype(np.float64)
    g = R.adjoint(M, LIGHTS, o, d, t, w, bits, K, SEED, spp=SPP, grad_image=x.gi, grad_value=x.gv)
    eps = 1e-6
    for j in range(R.PARAMS + len(LIGHTS)):
        e = np.zeros(R.PARAMS + len(LIGHTS)); e[j] = 1.0
        hi, lo = (_loss(*_perturbed(M, LIGHTS, e, s), o, d, t, w, bits, x) for s in (eps, -eps))
        assert g.gp[j] == pytest.approx((hi - lo) / (2 * eps), rel=1e-7, abs=1e-9), j
    assert np.abs(g.gp).min() > 1e-3                                # every parameter is exercised
    rng = np.random.default_rng(9)
    for _ in range(3):
        v = rng.normal(size=len(t))
        hi, lo = (_loss(M, LIGHTS, o, d, t + s * v, w, bits, x) for s in (eps, -eps))
        assert (g.gt * v).sum() == pytest.approx((hi - lo) / (2 * eps), rel=1e-7, abs=1e-9)
        hi, lo = (_loss(M, LIGHTS, o, d, t, w + s * v, bits, x) for s in (eps, -eps))
        assert (g.gw * v).sum() == pytest.approx((hi - lo) / (2 * eps), rel=1e-7, abs=1e-9)
    q = R.segment(M, o, d, t)
    assert (g.gt[~q.at_t] == 0).all() and (g.gt[np.isinf(t)] == 0).all()      # the top plane and a miss hold t's gradient at 0
    assert (g.gt[q.at_t & np.isfinite(t) & (bits != 0).any(0)] != 0).all()


def test_tangent_matches_central_differences():
    M, o, d, t, bits, x = _scene(seed=4)
    w = x.w.astype(np.float64)
    dimage, dvalue = R.tangent(M, LIGHTS, o, d, t, w, bits, K, SEED, spp=SPP, dw=x.dw, dt=x.dt, d_params=x.dp)
    eps = 1e-6
    out = []
    for s in (eps, -eps):
        M2, L2 = _perturbed(M, LIGHTS, x.dp.astype(np.float64), s)
        out.append(R.forward(M2, L2, o, d, t + s * x.dt, w + s * x.dw, bits, K, SEED, spp=SPP))
    for got, hi, lo in zip((dimage, dvalue), out[0], out[1]):
        np.testing.assert_allclose(got, (hi - lo) / (2 * eps), rtol=1e-6, atol=1e-9)
    assert np.abs(dvalue).max() > 1e-3


def test_known_answer_straight_down_under_an_overhead_light():
    """D = 0, c = -1, nu = 1, all bits set: E[value] = albedo p E (1 - exp(-2 sigma_t S)) / 2"""
    n, Kk, Sd = 50000, 4, 1.3
    M = R.medium(0.9, 0.8, 0.4, top_origin=(0.0, 0.0, 1.0))
    L = R.light((0.0, 0.0, 3.0), 2.5)
    o = np.stack([np.linspace(-1, 1, n), np.zeros(n), np.ones(n)])
    d = np.repeat(np.array([[0.0], [0.0], [-1.0]]), n, 1)
    t = np.full(n, Sd)
    q = R.segment(M, o, d, t)
    assert (q.D == 0).all() and (q.c == -1).all() and (q.u_in == 0).all() and R.nu(M, L) == 1.0
    p = R.phase(M, L, d)[0][0]
    want = M.albedo * p * L.irradiance * (1.0 - np.exp(-2.0 * M.sigma_t * Sd)) / 2.0
    # every point is a draw of its own: K single-point evaluations give the draws' own variance
    per = np.stack([R.forward(M, [L], o, d, t, None, [np.full(n, 1 << k, np.uint32)], Kk, SEED)[1][0] * Kk for k in range(Kk)])
    _, value = R.forward(M, [L], o, d, t, None, [np.full(n, (1 << Kk) - 1, np.uint32)], Kk, SEED)
    np.testing.assert_allclose(value[0], per.mean(0), rtol=1e-12)
    se = per.std(ddof=1) / np.sqrt(per.size)
    print("mean", value.mean(), "want", want, "standard error", se)
    assert abs(value.mean() - want) <= 5.0 * se and se < 1e-3 * want


def test_a_light_that_does_not_shine_in_gives_exact_zeros():
    M, o, d, t, bits, x = _scene(seed=2)
    lights = [LIGHTS[0], R.light(*R.BELOW), R.light((1.0, 0.0, -0.3), 1.0)]
    bits = np.concatenate([bits, bits[:1]])
    assert R.nu(M, lights[1]) < 0 and R.nu(M, lights[2]) <= 0
    x = R.inputs(len(t), SPP, 3)
    image, value = R.forward(M, lights, o, d, t, x.w, bits, K, SEED, spp=SPP)
    dimage, dvalue = R.tangent(M, lights, o, d, t, x.w, bits, K, SEED, spp=SPP, dw=x.dw, dt=x.dt, d_params=x.dp)
    g = R.adjoint(M, lights, o, d, t, x.w, bits, K, SEED, spp=SPP, grad_image=x.gi, grad_value=x.gv)
    for a in (image, value, dimage, dvalue):
        assert (a[1:] == 0).all() and (a[0] != 0).any()
    assert (g.gp[R.PARAMS + 1:] == 0).all() and g.gp[R.PARAMS] != 0
    for k in range(K):
        for L in lights[1:]:
            ro, w, maxt, tr = R.rays(M, L, o, d, t, k, SEED)
            assert not tr.any() and (ro == 0).all() and (w == 0).all() and (maxt == -1).all()


def test_tangent_and_adjoint_are_transposes():
    M, o, d, t, bits, x = _scene(seed=6)
    for w in (x.w.astype(np.float64), None):
        dimage, dvalue = R.tangent(M, LIGHTS, o, d, t, w, bits, K, SEED, spp=SPP, dw=x.dw if w is not None else None, dt=x.dt,
                                   d_params=x.dp)
        g = R.adjoint(M, LIGHTS, o, d, t, w, bits, K, SEED, spp=SPP, grad_image=x.gi, grad_value=x.gv)
        lhs = (dimage * x.gi).sum() + (dvalue * x.gv).sum()
        rhs = (g.gt * x.dt).sum() + (g.gp * x.dp).sum() + ((g.gw * x.dw).sum() if w is not None else 0.0)
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_rays_start_on_the_primary_ray_inside_the_segment():
    M, o, d, t, bits, x = _scene(seed=8)
    q = R.segment(M, o, d, t)
    for k in range(K):
        ro, w, maxt, tr = R.rays(M, LIGHTS[1], o, d, t, k, SEED)
        assert tr.all() and (maxt == np.inf).all()
        u = ((ro - o) * d).sum(0)
        assert (u >= q.u_in - 1e-12).all() and (u <= q.u_in + q.S + 1e-12).all()
        np.testing.assert_allclose(ro, o + u[None] * d, atol=1e-12)
        # below the top plane, and the float32 form is the same point to a rounding
        assert (((ro - M.top_origin[:, None]) * R.normal(M)[:, None]).sum(0) <= 1e-12).all()
        r32 = R.rays(M, LIGHTS[1], o.astype(np.float32), d.astype(np.float32), t, k, SEED, dtype=np.float32)[0]
        r64 = R.rays(M, LIGHTS[1], o.astype(np.float32), d.astype(np.float32), t, k, SEED)[0]
        assert np.abs(r32 - r64).max() < 1e-5
        assert (w == R.unit(LIGHTS[1])[0].astype(np.float32).astype(np.float64)[:, None]).all()

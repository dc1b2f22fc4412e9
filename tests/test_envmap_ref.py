"""The float64 restatement of the environment-map row (tests/envmap_ref.py) on its own, on the CPU: its density integrates
to one, its estimator is unbiased against a quadrature of the bilinear map, its adjoint agrees with central differences
of its own forward, its tangent is the transpose of its adjoint, and a constant map lights a plane with albedo * L."""
import numpy as np
import pytest

import envmap_ref as E
import sky_ref as S


@pytest.fixture(scope="module", params=[("sun", 0.0), ("sun", 0.25), ("gradient", 0.0), ("2x2", 0.5)],
                ids=lambda p: f"{p[0]}-u{p[1]}")
def env(request, oracle):
    name, u = request.param
    data = E.MAPS[name]()
    return name, u, data, E.build_table(data, u)


def _sphere_grid(W, H, sub):
    """midpoints of sub x sub sub-cells of every cell in (theta, phi), as world directions under DEFAULT_ROT, and their
    solid angles"""
    uy = (np.arange((H - 1) * sub) + 0.5) / ((H - 1) * sub)
    ux = (np.arange((W - 1) * sub) + 0.5) / ((W - 1) * sub) + 0.5 / (W - 1)
    th, ph = np.meshgrid(np.pi * uy, 2.0 * np.pi * ux, indexing="ij")
    local = np.stack([np.sin(th) * np.sin(ph), np.cos(th), -np.sin(th) * np.cos(ph)]).reshape(3, -1)
    dw = (np.sin(th) * (np.pi / len(uy)) * (2.0 * np.pi / len(ux))).ravel()
    return E.DEFAULT_ROT @ local, dw


def test_table_layout(env):
    name, u, data, table = env
    H, W = data.shape
    sigma, mbar, uu, M, C = E.split_table(table, W, H)
    assert np.array_equal(data[:, -1], data[:, 0])
    assert sigma == M[-1] and uu == np.float32(u) and table[3] == 0 and sigma > 0
    assert np.all(np.diff(M) >= 0) and np.all(np.diff(C, axis=1) >= 0)
    w = E.cell_weight(data, u, mbar)
    assert abs(float(M[-1]) - w.astype(np.float64).sum()) <= 4e-7 * float(M[-1])
    if name == "sun" and u == 0:
        assert (w == 0).sum() >= 16 * 3                                    # the rows below the horizon
    if u > 0:
        assert (w > 0).all()                                               # the defensive share reaches every cell


def test_pdf_integrates_to_one(env):
    name, u, data, table = env
    H, W = data.shape
    d, dw = _sphere_grid(W, H, 8)
    total = (E.pdf_direction(data, table, d, E.DEFAULT_ROT) * dw).sum()
    print(name, u, "integral of pdf_omega", total)
    assert abs(total - 1.0) <= 1e-4                                        # midpoint rule of sin over 8 sub-rows of a cell: (pi / (8 (H - 1)))^2 / 24 relative


def test_sampled_pdf_and_eval_agree_with_the_draw(env):
    """pdf_direction and eval_map of a drawn direction are 1 / G and L of that draw (away from the cell borders)"""
    name, u, data, table = env
    rng = np.random.default_rng(5)
    sx, sy = (rng.integers(0, 1 << 23, 4000) * 2.0 ** -23 for _ in range(2))
    cx, cy, fx, fy, wc, valid = E.draw(data, table, sx, sy)
    assert valid.all() and cx.max() <= data.shape[1] - 2 and cy.max() <= data.shape[0] - 2
    assert fx.min() >= 0 and fx.max() < 1 and fy.min() >= 0 and fy.max() < 1
    w, L, G, _ = E.shade(data, table, cx, cy, fx, fy, wc, valid, E.DEFAULT_ROT)
    inner = (np.minimum(fx, 1 - fx) > 1e-3) & (np.minimum(fy, 1 - fy) > 1e-3)
    assert inner.mean() > 0.9
    assert np.allclose(E.eval_map(data, w, E.DEFAULT_ROT)[inner], L[inner], rtol=1e-9, atol=1e-12)
    assert np.allclose(E.pdf_direction(data, table, w, E.DEFAULT_ROT)[inner] * G[inner], 1.0, rtol=1e-9)
    # the cells are drawn in proportion to their weights: 4 sigma of a binomial count on the heaviest cell
    wcell = E.cell_weight(data, u, table[1]).astype(np.float64)
    top = int(np.argmax(wcell)); share = wcell.ravel()[top] / wcell.sum()
    got = ((cy * (data.shape[1] - 1) + cx) == top).mean()
    assert abs(got - share) <= 4.0 * np.sqrt(share * (1 - share) / 4000) + 1e-12, (got, share)


def test_estimator_against_the_quadrature(env):
    """mean of E_k <n, w_k>+ / pi over 2^18 draws on an unoccluded plane = the quadrature of L <n, w>+ / pi; the bound is 4
    standard errors of the draws themselves"""
    name, u, data, table = env
    n, K = 1 << 15, 8
    dr = E.draws(data, table, np.arange(n), K, 7, E.DEFAULT_ROT)
    assert dr["valid"].all()
    co = np.maximum(dr["w"][:, 2, :], 0.0)
    x = (co * dr["L"] * dr["G"] / np.pi).ravel()
    d, dw = _sphere_grid(data.shape[1], data.shape[0], 32)
    ref = (E.eval_map(data, d, E.DEFAULT_ROT) * np.maximum(d[2], 0.0) / np.pi * dw).sum()
    se = x.std() / np.sqrt(x.size)
    print(name, u, "mean", x.mean(), "quadrature", ref, "standard error", se)
    assert ref > 0 and abs(x.mean() - ref) <= 4.0 * se


def test_constant_map_lights_a_plane_with_albedo_times_radiance(oracle):
    data = np.full((9, 17), 2.5, np.float32)
    table = E.build_table(data, 1.0)
    n, K, albedo = 1 << 14, 8, 0.6
    dr = E.draws(data, table, np.arange(n), K, 9, E.DEFAULT_ROT)
    sh_n = np.zeros((3, n)); sh_n[2] = 1.0
    d = -sh_n; t = np.ones(n)
    bits, _ = E.traced(sh_n, d, t, dr)
    image, value, _ = E.forward(sh_n, d, t, None, bits, dr, albedo, 4)
    se = value.std() / np.sqrt(n)
    print("plane mean", value.mean(), "expected", albedo * 2.5, "standard error", se)
    assert image.shape == (n // 4,) and abs(value.mean() - albedo * 2.5) <= 4.0 * se
    assert E.forward(sh_n, -d, t, None, bits, dr, albedo, 4)[0].max() == 0   # seen from behind: dark


def _case(rng, data, table, n, K, spp):
    sh_n = rng.normal(size=(3, n)); sh_n[2] = np.abs(sh_n[2]) + 0.2; sh_n /= np.linalg.norm(sh_n, axis=0)
    d = rng.normal(size=(3, n)); d[2] = -np.abs(d[2]) - 0.1
    d[:, ::7] *= -1.0
    t = rng.uniform(0.5, 3.0, n); t[rng.uniform(size=n) < 0.2] = np.inf
    dr = E.draws(data, table, np.arange(n), K, 3, E.DEFAULT_ROT)
    tr, _ = E.traced(sh_n, d, t, dr)
    bits = tr & (rng.uniform(size=(K, n)) < 0.7)
    return sh_n, d, t, rng.uniform(0.5, 1.5, n), bits, dr, rng.normal(size=n // spp)


def test_adjoint_matches_central_differences_of_the_forward(env):
    name, u, data, table = env
    rng = np.random.default_rng(3)
    n, K, spp = 48, 4, 4
    sh_n, d, t, weight, bits, dr, gi = _case(rng, data, table, n, K, spp)
    gn, gw, gd, cnt, _ = E.adjoint(sh_n, d, t, weight, bits, dr, 0.7, spp, gi, data.shape)
    f = lambda x, q, m: (E.forward(x, d, t, q, bits, dr, 0.7, spp, data=m)[0] * gi).sum()
    d64 = data.astype(np.float64)
    scale = np.abs(gn).max()
    assert scale > 0 and cnt.sum() == 4 * (bits & S.eligible(sh_n, d, t)[0][None]).sum()
    for i in range(n):
        for c in range(3):
            e = np.zeros_like(sh_n); e[c, i] = 1e-4
            fd = (f(sh_n + e, weight, d64) - f(sh_n - e, weight, d64)) / 2e-4
            assert abs(fd - gn[c, i]) <= 1e-6 * max(abs(gn[c, i]), scale), (c, i, fd, gn[c, i])
        e = np.zeros(n); e[i] = 1e-4
        fd = (f(sh_n, weight + e, d64) - f(sh_n, weight - e, d64)) / 2e-4
        assert abs(fd - gw[i]) <= 1e-6 * max(abs(gw[i]), np.abs(gw).max()), (i, fd, gw[i])
    for j in range(data.size):
        e = np.zeros(data.size); e[j] = 1e-4
        e = e.reshape(data.shape)
        fd = (f(sh_n, weight, d64 + e) - f(sh_n, weight, d64 - e)) / 2e-4
        assert abs(fd - gd.ravel()[j]) <= 1e-6 * max(abs(gd.ravel()[j]), np.abs(gd).max()), (j, fd, gd.ravel()[j])
        assert (cnt.ravel()[j] == 0) == (gd.ravel()[j] == 0)


@pytest.mark.parametrize("which", ["sh_n", "weight", "data", "all"])
@pytest.mark.parametrize("spp", [1, 4, 3])
def test_tangent_is_the_transpose_of_the_adjoint(env, spp, which):
    name, u, data, table = env
    rng = np.random.default_rng(23)
    n, K = 300, 4
    sh_n, d, t, weight, bits, dr, gi = _case(rng, data, table, n, K, spp)
    dn = rng.normal(size=(3, n)) if which in ("sh_n", "all") else None
    dw = rng.normal(size=n) if which in ("weight", "all") else None
    dd = rng.normal(size=data.shape) if which in ("data", "all") else None
    dimage = E.tangent(sh_n, d, t, weight, bits, dr, 0.8, spp, dn, dw, dd)
    gn, gw, gd, _, _ = E.adjoint(sh_n, d, t, weight, bits, dr, 0.8, spp, gi, data.shape)
    lhs = (dimage * gi).sum()
    parts = [(gn * dn) if dn is not None else 0.0, (gw * dw) if dw is not None else 0.0, (gd * dd) if dd is not None else 0.0]
    rhs = sum(np.sum(x) for x in parts)
    absum = sum(np.abs(x).sum() for x in parts)
    assert absum > 1e-6 and abs(lhs - rhs) <= 1e-12 * absum, (lhs, rhs)


def test_eval_adjoint_is_the_transpose_of_eval(env):
    name, u, data, table = env
    rng = np.random.default_rng(8)
    d = rng.normal(size=(3, 500)); d /= np.linalg.norm(d, axis=0)
    act = rng.uniform(size=500) < 0.8
    go = rng.normal(size=500)
    gd, cnt, _ = E.eval_adjoint(d, data.shape, go, E.DEFAULT_ROT, act)
    dd = rng.normal(size=data.shape)
    lhs = (E.eval_map(dd, d, E.DEFAULT_ROT, act) * go).sum()
    assert abs(lhs - (gd * dd).sum()) <= 1e-12 * np.abs(gd * dd).sum() and cnt.sum() == 4 * act.sum()
    # the poles and the seam: continuous across the seam, the north pole's row at theta = 0
    top = E.eval_map(data, E.DEFAULT_ROT @ np.array([[0.0], [1.0], [0.0]]), E.DEFAULT_ROT)
    assert np.isclose(top[0], data.astype(np.float64)[0].min(), atol=np.ptp(data[0]) + 1e-12)
    # the seam lies at phi = pi / (W - 1) (uv.x = 1/2 / (W - 1)): cell W - 2 on one side, cell 0 on the other, one value
    phi = np.pi / (data.shape[1] - 1) + np.array([-1e-9, 1e-9])
    seam = E.DEFAULT_ROT @ np.stack([0.8 * np.sin(phi), np.full(2, 0.6), -0.8 * np.cos(phi)])
    cx = E.lookup(seam, data.shape[1], data.shape[0], E.DEFAULT_ROT)[0]
    a, b = E.eval_map(data, seam, E.DEFAULT_ROT)
    assert tuple(cx) == (data.shape[1] - 2, 0) and abs(a - b) <= 1e-6 * max(abs(a), 1.0)

"""The specular row's restatement (tests/specular_ref.py) held against itself and against what it must reduce to, on the
CPU: the closed tangents against extrapolated central differences in every variable for each light of the rig, the
reverse sweep against the tangent, the known answers (a flat field seen from and lit from the zenith, the length of
to_light, the orthogonality of its gradient, the clamp of alpha), the exact zeros, and two quadratures that guard the
transcription of D and G1 themselves: the normalisation of the distribution and of its visible normals."""
import numpy as np
import pytest

import directional_ref as D
import specular_ref as R

N = 96


def _samples(L, n=N, seed=3):
    """unit normals around the half vector of the light and a viewer near the zenith, unit view directions, float32
    values; both cosines at least 0.05"""
    rng = np.random.default_rng(seed)
    l, _ = D.unit(L)
    wi = np.array([0.15, -0.1, 1.0])[:, None] + 0.25 * rng.standard_normal((3, n))
    wi = wi / np.linalg.norm(wi, axis=0)
    h = wi + l[:, None]
    sn = h / np.linalg.norm(h, axis=0) + 0.25 * rng.standard_normal((3, n))
    sn = (sn / np.linalg.norm(sn, axis=0)).astype(np.float32)
    wi = wi.astype(np.float32)
    keep = ((sn * l[:, None]).sum(0) > 0.05) & ((sn * wi).sum(0) > 0.05)
    return sn[:, keep], -wi[:, keep]


@pytest.fixture(scope="module", params=D.NAMES)
def case(request):
    L = D.rig((request.param,))[0]
    sn, d = _samples(L)
    n = sn.shape[1]
    assert n >= 20, (request.param, n)
    return request.param, L, sn, d, R.inputs(n, 1, 1), R.alpha_row("row", n).astype(np.float64)


def _extrapolated(f, h):
    """central differences at h and h / 2, Richardson-extrapolated: the error is O(h^4)"""
    d1, d2 = (f(h) - f(-h)) / (2 * h), (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


# test_directional_ref.py's bound for this comparison.  The lobe is sharp in sh_n where the directional value is linear:
# with a direction of sh_n of unit size the extrapolated difference's own O(h^4) error reaches 4e-7 at a = 0.05, so the
# direction of sh_n is a tenth of that (the step in sh_n is 1e-5).  Measured over the 8 lights x 5 variables: at most
# 1.4e-10 (sh_n), 8e-10 (to_light), 2e-11 (weight, alpha, irradiance) of the largest derivative.
FD_BOUND = 1e-8


def test_tangent_against_central_differences_in_every_variable(case):
    name, L, sn, d, x, alpha = case
    n = sn.shape[1]
    vis = np.ones((1, n), bool)
    sn64, w64 = np.asarray(sn, np.float64), np.asarray(x.w, np.float64)
    rng = np.random.default_rng(9)
    d4 = np.zeros((2, D.PARAMS))
    d4[0, :3], d4[1, 3] = 0.3 * rng.standard_normal(3), -0.4
    dirs = {"dn": 0.1 * rng.standard_normal((3, n)), "dw": rng.standard_normal(n), "da": 0.1 * rng.standard_normal(n),
            "to_light": d4[0], "irradiance": d4[1]}

    def value(key, s):
        row = D.row4(L) + (s * dirs[key] if key in ("to_light", "irradiance") else 0)
        q = D.light(row[:3])
        q.irradiance = row[3]
        step = lambda k: s * dirs[k] if key == k else 0
        return R.forward([q], sn64 + step("dn"), d, w64 + step("dw"), alpha + step("da"), R.ETA, vis)[1][0]

    worst = 0.0
    for key, direction in dirs.items():
        kw = {key: direction} if key in ("dn", "dw", "da") else {"d_lights": direction[None]}
        dv = R.tangent([L], sn64, d, w64, alpha, R.ETA, vis, **kw)[1][0]
        fd = _extrapolated(lambda s: value(key, s), 1e-4)
        err = np.abs(dv - fd).max() / max(1.0, np.abs(fd).max())
        worst = max(worst, err)
        print(name, key, "tangent against differences", err)
        assert err <= FD_BOUND, (name, key, err)
        assert np.abs(dv).max() > 0, (name, key)


def _rig_samples(K=8, per=24):
    """the whole rig on the union of the samples drawn for each light, a random visibility"""
    lights = D.rig()
    parts = [_samples(L, per, seed=11 + k) for k, L in enumerate(lights)]
    sn, d = (np.concatenate([p[j] for p in parts], 1) for j in (0, 1))
    n = sn.shape[1] - sn.shape[1] % 2
    sn, d = sn[:, :n], d[:, :n]
    vis = np.random.default_rng(4).random((K, n)) < 0.6
    vis[:, ::7] = False                 # (samples no light reaches)
    return lights, sn, d, vis


@pytest.mark.parametrize("spp", (1, 2))
def test_adjoint_is_the_transpose_of_the_tangent(spp):
    lights, sn, d, vis = _rig_samples()
    n, K = sn.shape[1], len(lights)
    x = R.inputs(n, spp, K)
    alpha = R.alpha_row("row", n)
    dimg, dv = R.tangent(lights, sn, d, x.w, alpha, R.ETA, vis, spp, dn=x.dn, dw=x.dw, da=x.da, d_lights=x.dl)
    g = R.adjoint(lights, sn, d, x.w, alpha, R.ETA, vis, spp, grad_image=x.gi, grad_value=x.gv)
    f64 = lambda a: np.asarray(a, np.float64)
    lhs = (dv * f64(x.gv)).sum() + (dimg * f64(x.gi)).sum()
    rhs = (g.gn * f64(x.dn)).sum() + (g.gw * f64(x.dw)).sum() + (g.ga * f64(x.da)).sum() + (g.g4 * f64(x.dl)).sum()
    scale = np.abs(dv * f64(x.gv)).sum() + np.abs(dimg * f64(x.gi)).sum()
    print("transposition", abs(lhs - rhs) / scale)
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale
    # exact zeros where no bit is set, or where a set bit meets a cosine that is not positive
    value = R.forward(lights, sn, d, x.w, alpha, R.ETA, vis, spp)[1]
    facing = np.stack([(f64(sn) * D.unit(L)[0][:, None]).sum(0) > 0 for L in lights])
    assert (vis & ~facing).any() and not value[~(vis & facing)].any() and (value[vis & facing] > 0).all()
    assert not dv[~(vis & facing)].any()
    dark = ~(vis & facing).any(0)
    assert dark.any() and not g.gn[:, dark].any() and not g.gw[dark].any() and not g.ga[dark].any()
    # a light's numbers do not depend on its neighbours
    alone = R.adjoint(lights[2:3], sn, d, x.w, alpha, R.ETA, vis[2:3], spp, grad_image=x.gi[2:3], grad_value=x.gv[2:3])
    assert np.array_equal(alone.g4[0], g.g4[2])
    assert np.array_equal(R.forward(lights[2:3], sn, d, x.w, alpha, R.ETA, vis[2:3], spp)[1][0], value[2])
    # the sums over a slice of the rows are the slice's own, and parts add up to the whole
    rows = R.adjoint(lights, sn, d, x.w, alpha, R.ETA, vis, 1, grad_value=x.gv, rows=slice(0, 40))
    part = R.adjoint(lights, sn[:, :40], d[:, :40], x.w[:40], alpha[:40], R.ETA, vis[:, :40], 1, grad_value=x.gv[:, :40])
    rest = R.adjoint(lights, sn, d, x.w, alpha, R.ETA, vis, 1, grad_value=x.gv, rows=slice(40, None))
    whole = R.adjoint(lights, sn, d, x.w, alpha, R.ETA, vis, 1, grad_value=x.gv)
    assert np.allclose(part.g4, rows.g4, rtol=1e-12, atol=1e-14)
    assert np.allclose(rows.g4 + rest.g4, whole.g4, rtol=1e-12, atol=1e-12 * np.abs(whole.g4).max())


@pytest.mark.parametrize("eta", (1.5, 0.0))
def test_a_flat_field_seen_and_lit_from_the_zenith_has_the_known_value(eta):
    L = D.rig(("zenith",))[0]
    n = 5
    sn = np.tile(np.array([[0.0], [0.0], [1.0]], np.float32), (1, n))
    w = np.linspace(0.5, 1.5, n)
    for a in (0.1, 0.3, 0.6):
        image, value = R.forward([L], sn, -sn, w, a, eta, np.ones((1, n), bool))
        F = ((eta - 1) / (eta + 1)) ** 2 if eta else 1.0
        assert np.abs(value[0] / (w * L.irradiance * F / (4 * np.pi * a * a)) - 1).max() <= 1e-14 and np.array_equal(image, value)


def test_the_length_of_to_light_changes_no_output_and_divides_its_gradient(case):
    name, L, sn, d, x, alpha = case
    n = sn.shape[1]
    vis = np.random.default_rng(2).random((1, n)) < 0.7
    twice = D.light(2 * L.to_light, L.irradiance)
    a, b = (R.evaluate([q], sn, d, x, alpha, R.ETA, vis, 1) for q in (L, twice))
    for k in ("image", "value", "gn", "gw", "ga"):
        assert np.allclose(getattr(a, k), getattr(b, k), rtol=1e-15, atol=0), k
    assert np.allclose(a.g4[0, :3], 2 * b.g4[0, :3], rtol=1e-13, atol=0) and np.allclose(a.g4[0, 3], b.g4[0, 3], rtol=1e-15)
    l, _ = D.unit(L)
    assert np.abs(a.g4[0, :3]).max() > 0
    print(name, "<grad_to_light, l>", abs(a.g4[0, :3] @ l) / np.abs(a.g4[0, :3]).max())
    assert abs(a.g4[0, :3] @ l) <= 1e-13 * np.abs(a.g4[0, :3]).max()      # orthogonal to l, to rounding
    # a tangent along to_light moves nothing
    along = np.append(L.to_light, 0.0)[None]
    dv = R.tangent([L], sn, d, x.w, alpha, R.ETA, vis, d_lights=along)[1]
    assert np.abs(dv).max() <= 1e-13 * np.abs(a.dvalue).max()


def test_alpha_below_the_clamp_gives_the_clamped_value_and_no_alpha_derivative(case):
    _, L, sn, d, x, _ = case
    n = sn.shape[1]
    vis = np.ones((1, n), bool)
    low = np.where(np.arange(n) % 2 == 0, 1e-5, -3.0)
    a, b = (R.evaluate([L], sn, d, x, al, R.ETA, vis, 1) for al in (low, np.full(n, R.ALPHA_MIN)))
    assert np.array_equal(a.value, b.value) and np.array_equal(a.gn, b.gn) and np.array_equal(a.g4, b.g4)
    assert not a.ga.any()
    only_da = R.tangent([L], sn, d, x.w, low, R.ETA, vis, da=x.da)[1]
    assert not only_da.any()
    # (at the clamp itself the derivative is held too: alpha > 1e-4 is strict)
    assert not b.ga.any()
    # a roughness that is not finite lights nothing
    bad = np.where(np.arange(n) % 2 == 0, np.inf, np.nan)
    c = R.evaluate([L], sn, d, x, bad, R.ETA, vis, 1)
    assert not c.value.any() and not c.gn.any() and not c.ga.any() and not c.g4.any() and not c.dvalue.any()


def _sphere(nt=2400, nphi=64):
    """a midpoint rule over the upper hemisphere of h: (h [3, m], the solid angle of each cell [m]); fine in theta near
    the pole, where D is concentrated (theta = t^2 pi / 2)"""
    t = (np.arange(nt) + 0.5) / nt
    theta, dtheta = t * t * (np.pi / 2), 2 * t * (np.pi / 2) / nt
    phi = (np.arange(nphi) + 0.5) * (2 * np.pi / nphi)
    T, P = np.meshgrid(theta, phi, indexing="ij")
    h = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)]).reshape(3, -1)
    return h, (np.sin(T) * dtheta[:, None] * (2 * np.pi / nphi)).reshape(-1)


@pytest.mark.parametrize("a", (0.1, 0.3, 0.6))
def test_quadratures_of_the_distribution_and_of_its_visible_normals(a):
    """int D(h) <n, h> dh = 1 (microfacet.h:185-207) and int D(h) G1(wi) max(<wi, h>, 0) dh = <n, wi> (the visible-normal
    normalisation behind microfacet.h:341-365), n the z axis.  Both guard the transcription of D and G1 themselves"""
    h, dw = _sphere()
    Dh = R.ggx(h[2], np.float64(a))[0]
    one = (Dh * h[2] * dw).sum()
    print("a", a, "int D <n, h>", one)
    assert abs(one - 1) <= 1e-6                     # (the midpoint rule on this grid: 5e-8 at a = 0.6)
    for wi in (np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, 0.8]), np.array([-0.3, 0.9, np.sqrt(0.1)])):
        ci = wi[2]
        G = R.smith(np.float64(a), np.float64(ci))[0]
        got = (Dh * G * np.maximum(wi @ h, 0) * dw).sum()
        print("a", a, "c_i", ci, "int D G1 <wi, h>", got)
        assert abs(got / ci - 1) <= 1e-6

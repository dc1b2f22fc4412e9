"""The float64 restatement of the glossy row (tests/glossy_ref.py) checked against itself, against closed forms and
against the density it claims to draw from, on the CPU: transposition, central differences with the draws held,
linearity in the texels, bounds, the draw's histogram, the detached estimator against the attached one, the clamp of
the roughness, the masks and the Fresnel term.  The GPU tests (tests/test_gpu_glossy.py) then hold the kernels against
this restatement."""
import numpy as np
import pytest

import envmap_ref as E
import glossy_ref as G

ROT = E.DEFAULT_ROT
ROT2 = ROT @ np.array([[np.cos(0.7), 0.0, np.sin(0.7)], [0.0, 1.0, 0.0], [-np.sin(0.7), 0.0, np.cos(0.7)]])
K, SEED = 3, 7


def _unit(x):
    return x / np.linalg.norm(x, axis=0)


def _wavefront(n=4000, seed=5, spread=0.35):
    """random shading normals around +Z, geometric normals near them, view directions from above, a roughness row in
    [0.05, 0.6]; some lanes miss, some are seen from behind"""
    rng = np.random.default_rng(seed)
    g = _unit(np.stack([rng.normal(0, spread, n), rng.normal(0, spread, n), np.ones(n)]))
    m = _unit(g + rng.normal(0, 0.25, (3, n)))
    d = _unit(np.stack([rng.normal(0, 0.8, n), rng.normal(0, 0.8, n), -np.ones(n)]))
    t = np.where(rng.random(n) < 0.1, np.inf, 1.0)
    w = rng.uniform(0.5, 1.5, n)
    al = rng.uniform(0.05, 0.6, n)
    bits = rng.random((K, n)) < 0.8
    return g, m, d, t, w, al, bits


def _args(g, m, d, t, w, al, eta, data, rot, bits, spp):
    return (g, m, d, t, None, w, al, eta, K, SEED, None, data, rot, bits, spp)


@pytest.mark.parametrize("eta", [0.0, 1.5])
@pytest.mark.parametrize("name,rot", [("sun", ROT), ("gradient", ROT2)])
def test_adjoint_and_tangent_are_transposes(eta, name, rot):
    data = E.MAPS[name]().astype(np.float64)
    g, m, d, t, w, al, bits = _wavefront()
    n, spp = m.shape[1], 4
    rng = np.random.default_rng(1)
    gi, gv = rng.normal(size=n // spp), rng.normal(size=n)
    dn, dw, da, dd = rng.normal(size=(3, n)), rng.normal(size=n), rng.normal(size=n), rng.normal(size=data.shape)
    args = _args(g, m, d, t, w, al, eta, data, rot, bits, spp)
    gm, gw, ga, gd = G.adjoint(*args, gi, gv)
    dimg, dval = G.tangent(*args, dn, dw, da, dd)
    lhs = (dimg * gi).sum() + (dval * gv).sum()
    rhs = (gm * dn).sum() + (gw * dw).sum() + (ga * da).sum() + (gd * dd).sum()
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    _, one = G.forward(*_args(g, m, d, t, w, al, eta, np.ones_like(data), rot, bits, spp))       # > 0 iff a direction counts
    assert 100 < (one != 0).sum() < n
    assert not gm[:, one == 0].any() and not dval[one == 0].any() and not ga[one == 0].any() and not gw[one == 0].any()


@pytest.mark.parametrize("eta", [0.0, 1.5])
@pytest.mark.parametrize("name,rot", [("sun", ROT), ("gradient", ROT2)])
def test_tangent_matches_central_differences_with_the_draws_held(eta, name, rot):
    """step h = 1e-6 along (dsh_n tangential, dweight, dalpha) in float64 with the draws of the unperturbed (sh_n, alpha)
    held: the held forward is a smooth function (no mask, no cell of the lookup moves), so the only errors are
    h^2 |f'''| / 6 and eps |f| / h = 2e-16 / 1e-6 |f|; the criteria are the reflect row's: 1e-6 of the largest |dvalue|
    per lane, 1e-7 in the relative L2 norm"""
    data = E.MAPS[name]().astype(np.float64)
    g, m, d, t, w, al, bits = _wavefront(seed=9)
    n = m.shape[1]
    rng = np.random.default_rng(2)
    dn, dw, da = rng.normal(size=(3, n)), rng.normal(size=n), 0.1 * rng.normal(size=n)
    dn = dn - m * (m * dn).sum(0)                                   # tangential
    h = 1e-6
    _, dval = G.tangent(*_args(g, m, d, t, w, al, eta, data, rot, bits, 1), dn, dw, da, None)
    f = lambda s: G.forward(*_args(g, m + s * h * dn, d, t, w + s * h * dw, al + s * h * da, eta, data, rot, bits, 1),
                            held=(m, al))[1]
    _, f0 = G.forward(*_args(g, m, d, t, w, al, eta, data, rot, bits, 1))
    assert np.abs(f(0.0) - f0).max() <= 1e-14 * np.abs(f0).max()     # held at its own draws: the forward itself
    cd = (f(1.0) - f(-1.0)) / (2 * h)
    # grazing lanes: the cosines c_i, c_o enter as 1 / c^3; leave out where one is below 0.05
    cmin = np.full(n, np.inf)
    for k in range(K):
        dr = G.draw(m, d, al, np.arange(n), k, SEED)
        cmin = np.minimum(cmin, np.where(bits[k], np.minimum(np.abs(dr.co), np.abs(dr.cwh)), np.inf))
    keep = (f0 != 0) & (cmin > 0.05) & (-(m * d).sum(0) > 0.05)
    assert keep.sum() > 0.3 * n, keep.sum()
    err = np.abs(cd - dval)[keep]
    print("lanes", int(keep.sum()), "largest |dvalue|", np.abs(dval[keep]).max(), "largest difference", err.max(),
          "relative L2", np.linalg.norm(err) / np.linalg.norm(dval[keep]))
    assert err.max() <= 1e-6 * np.abs(dval[keep]).max()
    assert np.linalg.norm(err) <= 1e-7 * np.linalg.norm(dval[keep])


def test_forward_is_linear_in_the_texels_and_bounded():
    g, m, d, t, w, al, bits = _wavefront()
    a, b = E.map_sun().astype(np.float64), np.random.default_rng(4).normal(size=(9, 17))
    f = lambda data: G.forward(*_args(g, m, d, t, w, al, 1.5, data, ROT2, bits, 4))
    (ia, va), (ib, vb), (ic, vc) = f(a), f(b), f(2.0 * a - 3.0 * b)
    assert np.abs(vc - (2.0 * va - 3.0 * vb)).max() <= 1e-12 * np.abs(vc).max()
    assert np.abs(ic - (2.0 * ia - 3.0 * ib)).max() <= 1e-12 * np.abs(ic).max()
    _, dv = G.tangent(*_args(g, m, d, t, w, al, 1.5, a, ROT2, bits, 4), None, None, None, b)
    assert np.abs(dv - vb).max() <= 1e-12 * np.abs(vb).max()
    # F <= 1, G1 <= 1 and the lookup is a convex combination of texels: 0 <= value <= weight max(data)
    for eta in (0.0, 1.5):
        _, v = G.forward(*_args(g, m, d, t, w, al, eta, a, ROT2, bits, 4))
        assert np.all(v >= 0) and np.all(v <= w * a.max() * (1 + 1e-15)) and v.max() > 0


def test_every_draw_faces_wi_and_has_unit_length():
    g, m, d, t, w, al, bits = _wavefront(n=20000)
    el, _ = G.eligible(g, m, d, t, None, al)
    for k in range(K):
        dr = G.draw(m, d, al, np.arange(m.shape[1]), k, SEED)
        ok = el & dr.valid
        assert ok.sum() > 10000
        assert np.all(dr.cwh[ok] > 0)
        assert np.abs(np.linalg.norm(dr.h[:, ok], axis=0) - 1).max() <= 1e-14
        assert np.abs(np.linalg.norm(dr.wo[:, ok], axis=0) - 1).max() <= 1e-14


# the 0.999 quantile of the chi-square distribution with 19 degrees of freedom (20 bins, the total fixed); from its
# tables (scipy.stats.chi2.ppf(0.999, 19) = 43.8202)
CHI2_999_19 = 43.8202


@pytest.mark.parametrize("alpha,tilt", [(0.3, 0.6), (0.6, 1.1), (0.1, 0.3)])
def test_histogram_of_the_draw_matches_its_density(alpha, tilt):
    """c_h = <n, h> of N draws for one (n, wi), binned into 20 bins of equal expected mass +- the quadrature; the
    expected counts integrate D G1(c_i) <wi, h> / c_i over the hemisphere of h numerically (midpoint rule on a
    4000 x 720 grid in (cos theta, phi) of the local frame)"""
    N = 200000
    n = np.repeat(_unit(np.array([[0.2], [-0.1], [1.0]])), N, 1)
    s, t = G._coordinate_system(n[:, :1], np.float64)
    wi = (np.sin(tilt) * (0.8 * s + 0.6 * t) + np.cos(tilt) * n[:, :1])
    d = np.repeat(-wi, N, 1)
    dr = G.draw(n, d, alpha, np.arange(N), 2, 11)
    assert dr.valid.all()
    # the density on a grid of the local frame
    nc, nphi = 4000, 720
    c = (np.arange(nc) + 0.5) / nc
    phi = (np.arange(nphi) + 0.5) / nphi * 2 * np.pi
    st = np.sqrt(1 - c * c)
    hl = np.stack([st[:, None] * np.cos(phi)[None], st[:, None] * np.sin(phi)[None], np.repeat(c[:, None], nphi, 1)])
    hw = s[:, 0, None, None] * hl[0] + t[:, 0, None, None] * hl[1] + n[:, 0, None, None] * hl[2]
    dens = G.pdf(hw.reshape(3, -1), np.repeat(wi, nc * nphi, 1), np.repeat(n[:, :1], nc * nphi, 1), alpha).reshape(nc, nphi)
    mass = dens.sum(1) * (2 * np.pi / nphi) / nc                     # per row of cos theta
    assert abs(mass.sum() - 1) <= 2e-3, mass.sum()                   # the density is normalised (quadrature error)
    cdf = np.cumsum(mass) / mass.sum()
    edges = np.concatenate([[0.0], np.interp(np.arange(1, 20) / 20, cdf, (np.arange(nc) + 1.0) / nc), [1.0 + 1e-12]])
    expected = np.diff(np.interp(edges, np.concatenate([[0.0], (np.arange(nc) + 1.0) / nc]), np.concatenate([[0.0], cdf]))) * N
    counts, _ = np.histogram(dr.ch, bins=edges)
    assert counts.sum() == N and expected.min() > 1000
    chi2 = ((counts - expected) ** 2 / expected).sum()
    print("alpha", alpha, "chi-square", chi2, "threshold", CHI2_999_19)
    assert chi2 <= CHI2_999_19


@pytest.mark.parametrize("alpha", [0.3, 0.6])
def test_detached_estimates_agree_with_differences_of_the_attached_estimate(alpha):
    """a constant map of 1, nothing occluded, one (n, wi) and N = 2^19 sample ids, K = 1: the mean of the detached
    derivative (draws held) against the central difference (h = 1e-3) of the attached estimate F G1(c_o), drawn again at
    the perturbed parameters from the same random numbers; per sample x_i = dvalue_i - (f_i(+) - f_i(-)) / (2 h), and
    |mean x| <= 4 standard errors of x, from the sample variance.  (G1(c_o) vanishes where the mask c_o > 0 cuts, so the
    attached estimate has no boundary term; the central difference is off by O(h^2).)"""
    N = 1 << 19
    n0 = _unit(np.array([[0.3], [0.1], [1.0]]))
    n = np.repeat(n0, N, 1)
    d = np.repeat(-_unit(np.array([[-0.5], [0.3], [1.0]])), N, 1)
    up = np.repeat(np.array([[0.0], [0.0], [1.0]]), N, 1)           # the geometric normal: masks nothing here
    data = np.ones((5, 9))
    bits = np.ones((1, N), bool)
    dnv = -d[:, :1] - n0 * (n0 * -d[:, :1]).sum()                    # tangential, towards wi: it changes all three cosines
    h = 1e-3
    f = lambda nn, al: G.forward(up, nn, d, np.ones(N), None, None, al, 0.0, 1, 3, None, data, None, bits, 1)[1]
    t = lambda dn, da: G.tangent(up, n, d, np.ones(N), None, None, alpha, 0.0, 1, 3, None, data, None, bits, 1, dn, None, da)[1]
    for what, dv, fd in (("alpha", t(None, np.ones(N)), (f(n, alpha + h) - f(n, alpha - h)) / (2 * h)),
                         ("n", t(np.repeat(dnv, N, 1), None), (f(_unit(n + h * dnv), alpha) - f(_unit(n - h * dnv), alpha)) / (2 * h))):
        x = dv - fd
        se = x.std(ddof=1) / np.sqrt(N)
        print(what, "alpha", alpha, "detached", dv.mean(), "attached difference", fd.mean(), "standard error", se)
        assert abs(dv.mean()) > 10 * se                              # the derivative is not noise
        assert abs(x.mean()) <= 4 * se, (x.mean(), se)


def test_roughness_below_the_clamp():
    g, m, d, t, w, al, bits = _wavefront(n=500)
    data = E.map_gradient().astype(np.float64)
    lo = _args(g, m, d, t, w, 1e-6, 0.0, data, ROT, bits, 1)
    at = _args(g, m, d, t, w, 1e-4, 0.0, data, ROT, bits, 1)
    assert np.array_equal(G.forward(*lo)[1], G.forward(*at)[1])
    gv = np.ones(500)
    assert not G.adjoint(*lo, None, gv)[2].any()                     # grad_alpha = 0 below the clamp
    assert G.adjoint(*_args(g, m, d, t, w, 0.3, 0.0, data, ROT, bits, 1), None, gv)[2].any()
    assert np.array_equal(G.tangent(*lo, None, None, np.ones(500), None)[1], np.zeros(500))
    # a non-finite roughness makes the sample ineligible
    bad = np.where(np.arange(500) % 2 == 0, np.nan, 0.3)
    _, v = G.forward(*_args(g, m, d, t, w, bad, 0.0, data, ROT, bits, 1))
    assert not v[::2].any() and v[1::2].any()


def test_masks():
    z = np.array([[0.0], [0.0], [1.0]])
    el = lambda g, n, d, t, act=None, al=0.3: G.eligible(g, n, d, t, act, al)[0][0]
    assert el(z, z, -z, [1.0])
    assert not el(z, z, -z, [np.inf])                                # a miss
    assert not el(z, z, z, [1.0])                                    # seen from behind
    assert not el(z, z, -z, [1.0], [0])                              # inactive
    assert not el(z, z, -z, [1.0], None, np.inf)                     # a non-finite roughness
    tilt = np.array([[np.sin(1.0)], [0.0], [np.cos(1.0)]])
    assert not el(-z, tilt, -z, [1.0])                               # the geometric normal faces away
    # a grazing view of a rough surface: some mirror directions dip below the geometric normal and are not traced
    n = 2000
    d = np.repeat(-np.array([[np.sin(1.4)], [0.0], [np.cos(1.4)]]), n, 1)
    zz = np.repeat(z, n, 1)
    tr, o, wo, maxt, h, margin, dr = G.rays(np.zeros((3, n)), zz, zz, d, np.ones(n), 0.6, 0)
    assert 0 < tr.sum() < n and np.all(wo[2, tr] > 0) and np.all(maxt[~tr] == -1) and not wo[:, ~tr].any()
    assert np.all(o[2, tr] > 0)
    # float32 runs the same text
    d32 = G.draw(zz, d, 0.6, np.arange(n), 0, 0, 1.5, np.float32)
    assert d32.h.dtype == np.float32 and d32.F.dtype == np.float32 and np.abs(d32.h - dr.h).max() < 1e-4


def test_fresnel_and_smith_known_answers():
    z = np.array([[0.0], [0.0], [1.0]])
    # alpha at the clamp and normal incidence: h = n to 1e-4, <wi, h> = 1: F(1, 1.5) = 0.04; eta = 0: F = 1
    dr = G.draw(z, -z, 1e-4, [5], 0, 0, 1.5)
    assert abs(dr.F[0] - 0.04) <= 1e-8
    assert G.draw(z, -z, 0.5, [5], 0, 0, 0.0).F[0] == 1.0
    # smith_g1 of the reference: 2 / (1 + sqrt(1 + a^2 tan^2 theta)); 1 at normal incidence
    th = 1.1
    assert abs(G.smith(0.4, np.cos(th))[0] - 2 / (1 + np.sqrt(1 + 0.16 * np.tan(th) ** 2))) <= 1e-15
    assert G.smith(0.4, 1.0)[0] == 1.0
    # its derivatives against central differences
    e = 1e-6
    Gc = (G.smith(0.4, np.cos(th) + e)[0] - G.smith(0.4, np.cos(th) - e)[0]) / (2 * e)
    Ga = (G.smith(0.4 + e, np.cos(th))[0] - G.smith(0.4 - e, np.cos(th))[0]) / (2 * e)
    _, dc, da = G.smith(0.4, np.cos(th))
    assert abs(dc - Gc) <= 1e-8 and abs(da - Ga) <= 1e-8

"""The float64 restatement of the caustic row (tests/caustic_ref.py) against closed-form answers on a flat field: normal
incidence, Snell's angle, the critical angle, the landing point of a tilted facet by hand; its adjoint and tangent against
central differences of its own forward and against each other; the recorded fresnel() values of the reference's own test."""
import json
import math
import os

import numpy as np
import pytest

import caustic_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fresnel_recorded.json")
RCV = R.plane_z(-1.0, (-2.0, 2.0), (-2.0, 2.0), 40, 40)        # 10 pixels per unit, one unit below the flat field z = 0


def _col(*v):
    return np.array(v, np.float64)[:, None]


def _flat(d, m=(0.0, 0.0, 1.0), p=(0.0, 0.0, 0.0), g=(0.0, 0.0, 1.0)):
    d = np.asarray(d, np.float64); d = d / np.linalg.norm(d)
    m = np.asarray(m, np.float64); m = m / np.linalg.norm(m)
    return _col(*p), _col(*g), m[:, None], d[:, None], np.ones(1)


@pytest.mark.parametrize("eta", [1.33, 1.5, 1 / 1.33, 1.0])
def test_normal_incidence(eta):
    p, g, m, d, t = _flat((0, 0, -1))
    v = R.vertex(p, g, m, d, t, None, eta, RCV)
    assert v.traced[0]
    assert np.allclose(v.wo[:, 0], d[:, 0], rtol=0, atol=1e-15)
    assert abs(v.F[0] - ((eta - 1) / (eta + 1)) ** 2) < 1e-15
    assert abs(v.s[0] - 1.0) < 1e-15
    pos, value = R.forward(p, g, m, d, t, None, None, eta, 2.5, RCV, np.ones(1))
    assert np.allclose(pos[:, 0], (20.0, 20.0), rtol=0, atol=1e-12)
    assert abs(value[0] - 2.5 * (1 - ((eta - 1) / (eta + 1)) ** 2)) < 1e-14
    # from below the same interface: the normal points away from the light, fresnel() serves the other sign
    up = R.plane_z(1.0, (-2.0, 2.0), (-2.0, 2.0), 40, 40)
    vb = R.vertex(p, g, m, -d, t, None, eta, up)
    assert vb.traced[0] and np.allclose(vb.wo[:, 0], -d[:, 0], rtol=0, atol=1e-15)
    assert abs(vb.F[0] - ((eta - 1) / (eta + 1)) ** 2) < 1e-15


@pytest.mark.parametrize("eta", [1.33, 1.5])
def test_snells_angle_at_45_degrees(eta):
    p, g, m, d, t = _flat((1, 0, -1))
    v = R.vertex(p, g, m, d, t, None, eta, RCV)
    assert v.traced[0]
    sin_t = math.sin(math.radians(45)) / eta
    assert abs(np.linalg.norm(v.wo[:, 0]) - 1) < 1e-15
    assert abs(v.wo[0, 0] - sin_t) < 1e-15 and abs(v.wo[2, 0] + math.sqrt(1 - sin_t ** 2)) < 1e-15 and v.wo[1, 0] == 0
    # the Fresnel equations written with the angles
    ti, tt = math.radians(45), math.asin(sin_t)
    rs = (math.sin(ti - tt) / math.sin(ti + tt)) ** 2
    rp = (math.tan(ti - tt) / math.tan(ti + tt)) ** 2
    assert abs(v.F[0] - 0.5 * (rs + rp)) < 1e-14
    pos, _ = R.forward(p, g, m, d, t, None, None, eta, 1.0, RCV, np.ones(1))
    assert abs(pos[0, 0] - (20 + 10 * math.tan(tt))) < 1e-12 and abs(pos[1, 0] - 20) < 1e-12


def test_critical_angle():
    """from the dense side (eta < 1): transmission up to asin(eta), total internal reflection beyond"""
    eta = 1 / 1.33
    crit = math.asin(eta)
    for off, want in ((-1e-6, True), (1e-6, False), (-0.2, True), (0.2, False)):
        a = crit + off
        p, g, m, d, t = _flat((math.sin(a), 0, -math.cos(a)))
        v = R.vertex(p, g, m, d, t, None, eta, RCV)
        assert bool(v.traced[0]) == want and bool(v.tir[0]) != want, (off, v.ct2)
        pos, value = R.forward(p, g, m, d, t, None, None, eta, 1.0, RCV, np.ones(1))
        if not want:
            assert value[0] == 0 and np.all(pos == R.NOWHERE)
    # eta > 1 never reflects totally
    p, g, m, d, t = _flat((math.sin(1.55), 0, -math.cos(1.55)))
    assert R.vertex(p, g, m, d, t, None, 1.33, RCV).traced[0]


def test_tilted_facet_by_hand():
    """light straight down on a facet tilted by 20 degrees about y, index 1.5: the refracted ray makes the angle
    20 - asin(sin 20 / 1.5) with the vertical, towards the side the facet faces away from"""
    tilt, eta = math.radians(20), 1.5
    m = (math.sin(tilt), 0, math.cos(tilt))
    p, g, mm, d, t = _flat((0, 0, -1), m=m, p=(0.3, -0.2, 0.1), g=m)
    v = R.vertex(p, g, mm, d, t, None, eta, RCV)
    dev = tilt - math.asin(math.sin(tilt) / eta)
    assert v.traced[0]
    assert np.allclose(v.wo[:, 0], (-math.sin(dev), 0, -math.cos(dev)), rtol=0, atol=1e-15)
    assert abs(v.s[0] - 1.1 / math.cos(dev)) < 1e-14
    pos, _ = R.forward(p, g, mm, d, t, None, None, eta, 1.0, RCV, np.ones(1))
    assert abs(pos[0, 0] - 10 * (0.3 - 1.1 * math.tan(dev) + 2)) < 1e-12 and abs(pos[1, 0] - 10 * (-0.2 + 2)) < 1e-12


def test_masks():
    p, g, m, d, t = _flat((0.2, 0.1, -1))
    ok = lambda **kw: bool(R.vertex(kw.get("p", p), kw.get("g", g), kw.get("m", m), kw.get("d", d), kw.get("t", t),
                                    kw.get("active"), 1.33, kw.get("rcv", RCV)).traced[0])
    assert ok()
    assert not ok(t=np.full(1, np.inf)) and not ok(active=np.zeros(1, bool))
    assert not ok(g=-g)                                            # the normals disagree on the side
    assert not ok(rcv=R.plane_z(1.0, (-2, 2), (-2, 2), 40, 40))    # the receiver lies behind the refracted ray
    assert not ok(d=_col(1.0, 0.0, 0.0))                           # c_i = 0
    # a shading normal bent so far that the refracted ray leaves on the light's side of the true surface
    # (grazing light at 1.5 rad from the vertical, -m at 1.7 rad, index 3: wo at 1.7 - asin(sin 0.2 / 3) = 1.634 > pi / 2)
    graze = np.array([math.sin(1.5), 0, -math.cos(1.5)])[:, None]
    bent = np.array([-math.sin(1.7), 0, math.cos(1.7)])[:, None]
    v = R.vertex(p, g, bent, graze, t, None, 3.0, RCV)
    assert v.eligible[0] and not v.tir[0] and v.wo[2, 0] > 0 and not v.consistent[0] and not v.traced[0]


def _case(rng, n, eta, wavy=0.3, below=False):
    """hits of a wavy surface lit from above (or from `below`: c_i < 0), a third of them not deposited"""
    m = rng.normal(size=(3, n)) * wavy; m[2] = 1.0; m /= np.linalg.norm(m, axis=0)
    g = m + rng.normal(size=(3, n)) * 0.05; g /= np.linalg.norm(g, axis=0)
    d = rng.normal(size=(3, n)) * 0.25; d[2] = -1.0; d /= np.linalg.norm(d, axis=0)
    p = rng.uniform(-1, 1, (3, n)); p[2] *= 0.2
    t = rng.uniform(0.5, 3, n); t[rng.uniform(size=n) < 0.1] = np.inf
    rcv = R.plane_z(-1.0, (-2.0, 2.0), (-2.0, 2.0), 40, 40)
    if below:
        d = -d; rcv = R.plane_z(1.0, (-2.0, 2.0), (-2.0, 2.0), 40, 40)
    vis = rng.uniform(size=n) < 0.7
    w = rng.uniform(0.5, 1.5, n)
    return (p, g, m, d, t, None, w, eta, 1.7, rcv, vis)


@pytest.mark.parametrize("eta", [1.33, 1 / 1.33])
def test_adjoint_and_tangent_match_central_differences(eta):
    rng = np.random.default_rng(5)
    n = 48
    args = _case(rng, n, eta)
    p, g, m, d, t, act, w, _, power, rcv, vis = args
    gpos, gv = rng.normal(size=(2, n)), rng.normal(size=n)
    v = R.vertex(p, g, m, d, t, act, eta, rcv)
    lit = v.traced & vis
    assert lit.sum() > n // 3 and (~lit).sum() > 3

    def loss(pp, mm, ww):
        pos, value = R.forward(pp, g, mm, d, t, act, ww, eta, power, rcv, lit)
        return (np.where(lit[None], pos * gpos, 0)).sum() + (value * gv).sum()
    gm, gp, gw = R.adjoint(*args, gpos, gv)
    assert not gm[:, ~lit].any() and not gp[:, ~lit].any() and not gw[~lit].any()
    h = 1e-6
    worst = 0.0
    for i in np.flatnonzero(lit):
        for c in range(3):
            e = np.zeros((3, n)); e[c, i] = h
            for got, fd in ((gm[c, i], (loss(p, m + e, w) - loss(p, m - e, w)) / (2 * h)),
                            (gp[c, i], (loss(p + e, m, w) - loss(p - e, m, w)) / (2 * h))):
                scale = max(abs(got), np.abs(gm[:, i]).max())
                worst = max(worst, abs(fd - got) / scale)
        e = np.zeros(n); e[i] = h
        fd = (loss(p, m, w + e) - loss(p, m, w - e)) / (2 * h)
        worst = max(worst, abs(fd - gw[i]) / max(abs(gw[i]), 1e-3))
    print("worst relative difference to central differences", worst)
    assert worst <= 1e-6
    # the tangent against central differences of the forward, by direction
    dn, dp, dw = rng.normal(size=(3, n)), rng.normal(size=(3, n)), rng.normal(size=n)
    dpos, dval = R.tangent(*args, dn, dp, dw)
    fp, fv = R.forward(p + h * dp, g, m + h * dn, d, t, act, w + h * dw, eta, power, rcv, lit)
    bp, bv = R.forward(p - h * dp, g, m - h * dn, d, t, act, w - h * dw, eta, power, rcv, lit)
    fdp, fdv = np.where(lit[None], (fp - bp) / (2 * h), 0), (fv - bv) / (2 * h)
    assert np.abs(fdp - dpos).max() <= 1e-6 * np.abs(dpos).max() and np.abs(fdv - dval).max() <= 1e-6 * np.abs(dval).max()


@pytest.mark.parametrize("which", ["sh_n", "p", "weight", "all"])
@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("eta", [1.33, 1 / 1.33])
def test_tangent_is_the_transpose_of_the_adjoint(eta, below, which):
    rng = np.random.default_rng(9)
    n = 500
    dense = (eta < 1) != below                                     # the light arrives in the denser medium: eta_ti > 1
    args = _case(rng, n, eta, wavy=0.6 if dense else 0.3, below=below)
    v = R.vertex(*args[:6], eta, args[9])
    assert (v.traced & args[10]).sum() > n // 4 and (v.eligible & v.tir).sum() > (10 if dense else -1)
    gpos, gv = rng.normal(size=(2, n)), rng.normal(size=n)
    dn = rng.normal(size=(3, n)) if which in ("sh_n", "all") else None
    dp = rng.normal(size=(3, n)) if which in ("p", "all") else None
    dw = rng.normal(size=n) if which in ("weight", "all") else None
    dpos, dval = R.tangent(*args, dn, dp, dw)
    gm, gp, gw = R.adjoint(*args, gpos, gv)
    lhs = (dpos * gpos).sum() + (dval * gv).sum()
    rhs = sum(0.0 if t is None else (g * t).sum() for g, t in ((gm, dn), (gp, dp), (gw, dw)))
    assert abs(lhs) > 1e-3
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_recorded_fresnel_values_of_the_reference():
    rec = json.load(open(GOLDEN))
    for c in rec["cases"]:
        F, ct, eta_it, eta_ti = R.fresnel(c["cos_theta_i"], c["eta"])
        for got, key in ((F, "F"), (ct, "cos_theta_t"), (eta_it, "eta_it"), (eta_ti, "eta_ti")):
            if c[key] is not None:
                assert abs(float(got) - c[key]) <= rec["atol"] + rec["rtol"] * abs(c[key]), (c, key, float(got))
        # refract() in the local frame (fresnel.h:293-295) has unit length: Snell's law
        s2 = (1 - c["cos_theta_i"] ** 2) * float(eta_ti) ** 2
        if s2 <= 1:
            assert abs(s2 + float(ct) ** 2 - 1) < 1e-12
    # fresnel() is what vertex() evaluates
    ci = np.linspace(-1, 1, 41); ci = ci[ci != 0]
    m = np.zeros((3, ci.size)); m[2] = 1
    d = np.stack([-np.sqrt(1 - ci ** 2), 0 * ci, -ci])
    for eta in (1.5, 1 / 1.5, 1.0):
        v = R.vertex(np.zeros((3, ci.size)), np.sign(ci) * m, m, d, np.ones(ci.size), None, eta, RCV)
        F, ct, _, e = R.fresnel(ci, eta)
        ok = ~v.tir
        assert np.allclose(v.F[ok], F[ok], rtol=0, atol=1e-15) and np.allclose(v.wo[2][ok], ct[ok], rtol=0, atol=1e-15)


def test_filter_mass_and_flat_film():
    """the film's constant in closed form, and the physical check of the GPU test on the restatement's own film: a dense
    regular grid at normal incidence fills the lit footprint with power (1 - F) samples-per-pixel to within 3 %
    (the lattice ripple of a Gaussian of sigma 0.5 px, 2 exp(-2 pi^2 sigma^2) = 1.4 %, doubled)"""
    closed = (0.5 * (math.sqrt(2 * math.pi) * math.erf(2 * math.sqrt(2)) - 8 * math.exp(-8))) ** 2
    assert abs(R.filter_mass(0.5) - closed) < 1e-9
    k = 2                                                          # samples per pixel and axis
    xs = (np.arange(16 * k) + 0.5) / k + 8                         # pixels 8 .. 24 of a 32 x 32 film
    px, py = (a.ravel() for a in np.meshgrid(xs, xs))
    n = px.size
    rcv = R.plane_z(-0.5, (-1.0, 1.0), (-1.0, 1.0), 32, 32)
    p = np.stack([px / 16 - 1, py / 16 - 1, np.zeros(n)])
    up = np.zeros((3, n)); up[2] = 1
    pos, value = R.forward(p, up, up, -up, np.ones(n), None, None, 1.33, 0.25, rcv, np.ones(n))
    assert np.allclose(pos, np.stack([px, py]), rtol=0, atol=1e-12)
    img = R.film(pos, value, 32, 32)
    want = 0.25 * (1 - (0.33 / 2.33) ** 2) * k * k
    inner = img[11:21, 11:21]
    print("film inside the footprint", inner.min(), inner.max(), "expected", want)
    assert np.abs(inner / want - 1).max() < 0.03
    assert abs(img.sum() / value.sum() - 1) < 0.03                # a pixel holds flux: the film sums to what was deposited (same ripple)

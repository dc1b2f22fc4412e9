"""The float64 restatement of the reflection row (tests/reflect_ref.py) checked against itself and against closed forms
on the CPU: transposition, central differences, linearity in the texels and known answers.  The GPU tests
(tests/test_gpu_reflect.py) then hold the kernels against this restatement."""
import numpy as np
import pytest

import envmap_ref as E
import reflect_ref as R

ROT = E.DEFAULT_ROT
A = 0.7
ROT2 = ROT @ np.array([[np.cos(A), 0.0, np.sin(A)], [0.0, 1.0, 0.0], [-np.sin(A), 0.0, np.cos(A)]])


def _wavefront(n=4000, seed=5, spread=0.35):
    """random shading normals around +Z, geometric normals near them, view directions from above; some lanes miss, some
    are seen from behind, some reflect below the true surface"""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=0)
    g = unit(np.stack([rng.normal(0, spread, n), rng.normal(0, spread, n), np.ones(n)]))
    m = unit(g + rng.normal(0, 0.25, (3, n)))
    d = unit(np.stack([rng.normal(0, 0.8, n), rng.normal(0, 0.8, n), -np.ones(n)]))
    t = np.where(rng.random(n) < 0.1, np.inf, 1.0)
    w = rng.uniform(0.5, 1.5, n)
    vis = rng.random(n) < 0.8
    return g, m, d, t, w, vis


@pytest.mark.parametrize("eta", [0.0, 1.5])
@pytest.mark.parametrize("name,rot", [("sun", ROT), ("gradient", ROT2)])
def test_adjoint_and_tangent_are_transposes(eta, name, rot):
    data = E.MAPS[name]().astype(np.float64)
    g, m, d, t, w, vis = _wavefront()
    n, spp = m.shape[1], 4
    rng = np.random.default_rng(1)
    gi, gv = rng.normal(size=n // spp), rng.normal(size=n)
    dn, dw, dd = rng.normal(size=(3, n)), rng.normal(size=n), rng.normal(size=data.shape)
    args = (g, m, d, t, None, w, eta, data, rot, vis, spp)
    v = R.vertex(g, m, d, t, None, eta)
    assert 100 < (v.traced & vis).sum() < n and (~v.eligible).sum() > 100 and (v.eligible & ~v.consistent).sum() > 10
    gm, gw, gd = R.adjoint(*args, gi, gv)
    dimg, dval = R.tangent(*args, dn, dw, dd)
    lhs = (dimg * gi).sum() + (dval * gv).sum()
    rhs = (gm * dn).sum() + (gw * dw).sum() + (gd * dd).sum()
    assert abs(lhs) > 0 and abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    assert not gm[:, ~(v.traced & vis)].any() and not dval[~(v.traced & vis)].any()


@pytest.mark.parametrize("eta", [0.0, 1.5, 1 / 1.5])
@pytest.mark.parametrize("name,rot", [("sun", ROT), ("gradient", ROT2)])
def test_tangent_matches_central_differences(eta, name, rot):
    """step h = 1e-6 along (dsh_n, dweight) in float64, on lanes at least 1e-3 of a cell away from a cell border and with
    s2, q >= 1e-2 (away from the poles), and away from the critical angle (cos_theta_t^2 >= 1e-2).  The map coordinate
    moves by at most K h |dsh_n| cells with K = 2 (W - 1) / (2 pi sin theta) <= 51 cells per unit of sh_n, so for
    |dsh_n| <= 6 no compared lane crosses a border (3e-4 < 1e-3).  A central difference is off by h^2 |f'''| / 6 +
    eps |f| / h: relative to |f'| ~ K |dsh_n| |f| that is (K |dsh_n| h)^2 / 6 + eps / (K |dsh_n| h) <= 2e-8 + 1e-9 where
    the derivative is large, and eps |f| / h <= 2e-16 * 75 / 1e-6 = 2e-8 absolutely; the bound below is 1e-6 of the
    largest |dvalue| per lane and 1e-7 in the relative L2 norm"""
    data = E.MAPS[name]().astype(np.float64)
    H, W = data.shape
    g, m, d, t, w, vis = _wavefront(seed=9)
    n = m.shape[1]
    rng = np.random.default_rng(2)
    dn, dw = rng.normal(size=(3, n)), rng.normal(size=n)
    h = 1e-6
    assert np.abs(dn).max() < 6
    args = lambda mm, ww: (g, mm, d, t, None, ww, eta, data, rot, vis, 1)
    _, dval = R.tangent(*args(m, w), dn, dw, None)
    _, fp = R.forward(*args(m + h * dn, w + h * dw))
    _, fm = R.forward(*args(m - h * dn, w - h * dw))
    cd = (fp - fm) / (2 * h)
    v = R.vertex(g, m, d, t, None, eta)
    _, _, _, _, vv, _ = R.lookup(v.wr, W, H, rot)
    ct2 = 1 - (1 - v.c * v.c) / (eta * eta) if eta else np.ones(n)
    keep = v.traced & vis & R.smooth_lanes(v.wr, W, H, rot, 1e-3) & (vv[0] ** 2 + vv[2] ** 2 >= 1e-2) & (1 - vv[1] ** 2 >= 1e-2) & \
        (v.margin > 1e-3) & ((ct2 >= 1e-2) | (ct2 <= -1e-2))
    assert keep.sum() > 0.3 * n, keep.sum()
    err = np.abs(cd - dval)[keep]
    print("lanes", int(keep.sum()), "largest |dvalue|", np.abs(dval[keep]).max(), "largest difference", err.max(),
          "relative L2", np.linalg.norm(err) / np.linalg.norm(dval[keep]))
    assert err.max() <= 1e-6 * np.abs(dval[keep]).max()
    assert np.linalg.norm(err) <= 1e-7 * np.linalg.norm(dval[keep])


def test_forward_is_linear_in_the_texels():
    g, m, d, t, w, vis = _wavefront()
    a, b = E.map_sun().astype(np.float64), np.random.default_rng(4).normal(size=(9, 17))
    f = lambda data: R.forward(g, m, d, t, None, w, 1.5, data, ROT2, vis, 4)
    (ia, va), (ib, vb), (ic, vc) = f(a), f(b), f(2.0 * a - 3.0 * b)
    assert np.abs(vc - (2.0 * va - 3.0 * vb)).max() <= 1e-12 * np.abs(vc).max()
    assert np.abs(ic - (2.0 * ia - 3.0 * ib)).max() <= 1e-12 * np.abs(ic).max()
    # and the texel tangent is the forward of the tangent
    _, dv = R.tangent(g, m, d, t, None, w, 1.5, a, ROT2, vis, 4, None, None, b)
    assert np.abs(dv - vb).max() <= 1e-12 * np.abs(vb).max()


def test_lookup_is_envmap_refs():
    w = np.random.default_rng(6).normal(size=(3, 1000))
    w /= np.linalg.norm(w, axis=0)
    for rot in (None, ROT, ROT2):
        cx, cy, fx, fy, _, _ = R.lookup(w, 17, 9, rot)
        ex, ey, gx, gy = E.lookup(w, 17, 9, rot)
        assert np.array_equal(cx, ex) and np.array_equal(cy, ey) and np.array_equal(fx, gx) and np.array_equal(fy, gy)
        s = R.shade(w, E.map_sun(), rot)
        assert np.abs(s.L - E.eval_map(E.map_sun(), w, rot)).max() <= 1e-13


@pytest.mark.parametrize("name", ["sun", "gradient"])
def test_flat_field_seen_straight_down_reflects_straight_up(name):
    data = E.MAPS[name]().astype(np.float64)
    up = np.array([[0.0], [0.0], [1.0]])
    tr, o, wr, maxt, v = R.rays(np.zeros((3, 1)), up, up, -up, [1.0])
    assert tr[0] and np.array_equal(wr, up) and maxt[0] == np.inf and o[2, 0] > 0
    env_up = E.eval_map(data, up, ROT)[0]
    assert abs(env_up - data[0, 0]) <= 1e-15          # the map's +Y is world +Z: row 0, which is constant
    for eta, F in ((0.0, 1.0), (1.5, 0.04)):
        img, val = R.forward(up, up, -up, [1.0], None, None, eta, data, ROT, [True])
        assert abs(val[0] - env_up * F) <= 1e-15 and img[0] == val[0]
    # at the pole the direction derivative is exactly zero
    assert not R.shade(up, data, ROT).G.any()


def test_fresnel_known_answers():
    z = np.array([[0.0], [0.0], [1.0]])
    assert abs(R.vertex(z, z, -z, [1.0], None, 1.5).F[0] - 0.04) <= 1e-16
    c = np.linspace(0.05, 1.0, 20)
    d = -np.stack([np.sqrt(1 - c * c), 0 * c, c])
    zz = np.repeat(z, 20, 1)
    v0 = R.vertex(zz, zz, d, np.ones(20), None, 0.0)
    assert np.all(v0.F == 1.0) and not v0.dF.any()
    v1 = R.vertex(zz, zz, d, np.ones(20), None, 1.0)
    assert not v1.F.any() and not v1.dF.any()
    # F' against a central difference of fresnel() itself
    h = 1e-6
    v = R.vertex(zz, zz, d, np.ones(20), None, 1.5)
    cd = (R.fresnel(c[:-1] + h, 1.5)[0] - R.fresnel(c[:-1] - h, 1.5)[0]) / (2 * h)
    assert np.abs(v.dF[:-1] - cd).max() <= 1e-8
    # total internal reflection: F = 1, a constant
    vt = R.vertex(zz, zz, d, np.ones(20), None, 1 / 1.5)
    tir = 1 - (1 - c * c) * 2.25 <= 0
    assert tir.sum() > 3 and np.all(vt.F[tir] == 1.0) and not vt.dF[tir].any()


def test_rotation_by_a_quarter_turn_about_y_moves_the_column_by_a_quarter_of_the_map():
    w = np.random.default_rng(7).normal(size=(3, 500))
    w /= np.linalg.norm(w, axis=0)
    W, H = 17, 9
    Ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    cx0, cy0, fx0, fy0, _, _ = R.lookup(w, W, H, ROT)
    cx1, cy1, fx1, fy1, _, _ = R.lookup(w, W, H, ROT @ Ry)
    shift = ((cx1 + fx1) - (cx0 + fx0)) % (W - 1)
    assert np.abs(shift - (W - 1) / 4).max() <= 1e-9
    assert np.abs((cy1 + fy1) - (cy0 + fy0)).max() <= 1e-9


def test_masks_and_margin():
    z = np.array([[0.0], [0.0], [1.0]])
    tilt = np.array([[np.sin(1.0)], [0.0], [np.cos(1.0)]])                      # 57 degrees from +Z
    graze = -np.array([[-np.sin(0.17)], [0.0], [np.cos(0.17)]])                 # wi: 10 degrees from +Z, towards -X
    # seen from the front of both normals, but the mirror direction about the tilted shading normal (2 * 57 + 10 = 124
    # degrees from +Z) dips below g = +Z
    m = tilt
    v = R.vertex(z, m, graze, [1.0], None, 0.0)
    assert v.eligible[0] and not v.consistent[0] and not v.traced[0]
    assert not R.vertex(z, z, -z, [np.inf], None, 0.0).traced[0]                # a miss
    assert not R.vertex(z, z, z, [1.0], None, 0.0).traced[0]                    # seen from behind
    assert not R.vertex(z, z, -z, [1.0], [0], 0.0).traced[0]                    # inactive
    assert R.vertex(z, z, -z, [1.0], None, 0.0).margin[0] == 1.0
    # float32 runs the same text
    v32 = R.vertex(z, m, graze, [1.0], None, 1.5, np.float32)
    assert v32.F.dtype == np.float32 and v32.wr.dtype == np.float32

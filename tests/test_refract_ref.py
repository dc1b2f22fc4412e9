"""The float64 restatement of the refraction view (tests/refract_ref.py): the bitmap lookup against a direct per-texel
loop for both wraps, positions outside the texture, not finite and beyond 2^23 included; closed-form values on a flat
field; its adjoint and tangent against central differences of its own forward on lanes away from cell borders, and
against each other."""
import math

import numpy as np
import pytest

import refract_ref as R

RCV = R.plane_z(-1.0, (-2.0, 2.0), (-2.0, 2.0), 12, 7)         # 3 x 1.75 texels per unit, one unit below the field z = 0
BORDER = 5e-3


def _texel(tex, ix, iy, wrap):
    TH, TW = tex.shape
    if wrap == R.CLAMP:
        return tex[min(max(iy, 0), TH - 1), min(max(ix, 0), TW - 1)]
    return tex[iy % TH, ix % TW]


@pytest.mark.parametrize("wrap", [R.CLAMP, R.REPEAT])
def test_bitmap_lookup_against_a_per_texel_loop(wrap):
    rng = np.random.default_rng(2)
    tex = rng.uniform(-1, 2, (5, 9))
    pos = rng.uniform(-5, 14, (2, 400))
    pos[:, :9] = np.array([[0.5, 8.5, 0.0, 9.0, -0.5, 9.5, 4.5, -16.0, 3.25], [0.5, 4.5, 0.0, 5.0, -0.5, 5.5, 2.5, -16.0, 7.0]])
    e = R.lookup(tex, pos, wrap)
    inside = outside = 0
    for k in range(pos.shape[1]):
        qx, qy = pos[0, k] - 0.5, pos[1, k] - 0.5
        ix, iy = math.floor(qx), math.floor(qy)
        fx, fy = qx - ix, qy - iy
        v = [_texel(tex, ix + a, iy + b, wrap) for b in (0, 1) for a in (0, 1)]
        L = (1 - fy) * ((1 - fx) * v[0] + fx * v[1]) + fy * ((1 - fx) * v[2] + fx * v[3])
        assert abs(e.L[k] - L) <= 1e-14, (k, pos[:, k])
        assert abs(e.Lx[k] - ((1 - fy) * (v[1] - v[0]) + fy * (v[3] - v[2]))) <= 1e-14
        assert abs(e.Ly[k] - ((1 - fx) * (v[2] - v[0]) + fx * (v[3] - v[1]))) <= 1e-14
        assert abs(e.b[:, k].sum() - 1) <= 1e-14 and abs((e.b[:, k] * tex.ravel()[e.idx[:, k]]).sum() - L) <= 1e-14
        if 0 <= qx <= 8 and 0 <= qy <= 4:
            inside += 1
        elif wrap == R.CLAMP and (qx < -1 or qx > 9) and (qy < -1 or qy > 5):
            outside += 1
            assert e.Lx[k] == 0 and e.Ly[k] == 0          # of its own accord
    assert inside > 20 and (wrap == R.REPEAT or outside > 20)
    # a texel centre reads the texel; the slopes are central differences of L inside a cell
    c = R.lookup(tex, np.array([[3.5, 0.5], [2.5, 4.5]]), wrap)
    assert c.L[0] == tex[2, 3] and c.L[1] == tex[4, 0]
    x = np.array([[3.2], [1.9]])
    h = 1e-6
    fd = [(R.lookup(tex, x + h * np.eye(2)[:, j:j + 1], wrap).L - R.lookup(tex, x - h * np.eye(2)[:, j:j + 1], wrap).L) / (2 * h)
          for j in range(2)]
    s = R.lookup(tex, x, wrap)
    assert abs(fd[0][0] - s.Lx[0]) < 1e-8 and abs(fd[1][0] - s.Ly[0]) < 1e-8


def test_bitmap_lookup_of_positions_without_a_cell():
    """not finite, or |q| >= 2^23: under clamp the border texel a float clamp of q to [-1, res] reads, under repeat 0"""
    tex = np.arange(15, dtype=np.float64).reshape(3, 5) + 1
    bad = np.array([np.inf, -np.inf, np.nan, 2.0 ** 23 + 0.5, -2.0 ** 23 - 0.5, 1e30])
    for k, b in enumerate(bad):
        pos = np.array([[b, 2.5], [1.5, b]])
        c = R.lookup(tex, pos, R.CLAMP)
        col = 4 if b > 0 else 0
        row = 2 if b > 0 else 0
        assert c.L[0] == tex[1, col] and c.L[1] == tex[row, 2], (b, c.L)
        assert not c.Lx[0] and not c.Ly[1]
        r = R.lookup(tex, pos, R.REPEAT)
        assert not r.L.any() and not r.Lx.any() and not r.Ly.any() and not r.b.any()
    near = R.lookup(tex, np.array([[2.0 ** 23 - 1.0], [1.5]]), R.REPEAT)      # the last coordinate that has a cell
    assert near.ok[0] and near.L[0] != 0


@pytest.mark.parametrize("sigma_t", [0.0, 0.7])
@pytest.mark.parametrize("eta", [1.33, 1.5, 1 / 1.33])
def test_flat_field_seen_straight_down(eta, sigma_t):
    """(1 - F0) eta_ti^2 exp(-sigma_t depth) c over a constant texture c, from either side of the interface"""
    up = np.array([[0.0], [0.0], [1.0]])
    p = np.zeros((3, 1))
    tex = np.full((7, 12), 0.8)
    F0 = ((eta - 1) / (eta + 1)) ** 2
    value, image, pos = R.forward(p, up, up, -up, np.ones(1), None, None, eta, sigma_t, RCV, tex, R.CLAMP, np.ones(1))
    assert abs(value[0] - (1 - F0) / eta ** 2 * math.exp(-sigma_t) * 0.8) < 1e-15 and image[0] == value[0]
    assert np.allclose(pos[:, 0], (6.0, 3.5), rtol=0, atol=1e-12)
    above = R.plane_z(1.0, (-2.0, 2.0), (-2.0, 2.0), 12, 7)
    value, _, _ = R.forward(p, up, up, up, np.ones(1), None, None, eta, sigma_t, above, tex, R.CLAMP, np.ones(1))
    assert abs(value[0] - (1 - F0) * eta ** 2 * math.exp(-sigma_t) * 0.8) < 1e-15
    dark, _, nowhere = R.forward(p, up, up, -up, np.ones(1), None, None, eta, sigma_t, RCV, tex, R.CLAMP, np.zeros(1))
    assert dark[0] == 0 and np.all(nowhere == R.NOWHERE)


def test_flat_field_seen_at_40_degrees_shows_the_ramp_at_the_snell_displaced_point():
    eta, a = 1.33, math.radians(40)
    up = np.array([[0.0], [0.0], [1.0]])
    d = np.array([[math.sin(a)], [0.0], [-math.cos(a)]])
    tex = np.tile(np.arange(12, dtype=np.float64) * 0.25 + 1, (7, 1))      # L = 1 + 0.25 (x - 0.5) in texel coordinates
    tt = math.asin(math.sin(a) / eta)
    x = 3 * (0.2 + math.tan(tt) + 2)
    value, _, pos = R.forward(np.array([[0.2], [0.1], [0.0]]), up, up, d, np.ones(1), None, None, eta, 0.0, RCV, tex, R.CLAMP, np.ones(1))
    assert abs(pos[0, 0] - x) < 1e-12 and 0.5 < x < 11.5
    rs = (math.sin(a - tt) / math.sin(a + tt)) ** 2
    rp = (math.tan(a - tt) / math.tan(a + tt)) ** 2
    assert abs(value[0] - (1 - 0.5 * (rs + rp)) / eta ** 2 * (1 + 0.25 * (x - 0.5))) < 1e-14


def _case(rng, n, eta, sigma_t, wrap, spp, wavy=0.3, below=False):
    """hits of a wavy surface seen from above (or from `below`: c_i < 0), a third of them occluded"""
    m = rng.normal(size=(3, n)) * wavy; m[2] = 1.0; m /= np.linalg.norm(m, axis=0)
    g = m + rng.normal(size=(3, n)) * 0.05; g /= np.linalg.norm(g, axis=0)
    d = rng.normal(size=(3, n)) * 0.25; d[2] = -1.0; d /= np.linalg.norm(d, axis=0)
    p = rng.uniform(-1, 1, (3, n)); p[2] *= 0.2
    t = rng.uniform(0.5, 3, n); t[rng.uniform(size=n) < 0.1] = np.inf
    rcv = RCV
    if below:
        d = -d; rcv = R.plane_z(1.0, (-2.0, 2.0), (-2.0, 2.0), 12, 7)
    vis = rng.uniform(size=n) < 0.7
    w = rng.uniform(0.5, 1.5, n)
    tex = rng.uniform(0.2, 1.0, (7, 12))
    return (p, g, m, d, t, None, w, eta, sigma_t, rcv, tex, wrap, vis), spp


@pytest.mark.parametrize("wrap", [R.CLAMP, R.REPEAT])
@pytest.mark.parametrize("sigma_t", [0.0, 0.7])
@pytest.mark.parametrize("eta", [1.33, 1 / 1.33])
def test_adjoint_and_tangent_match_central_differences(eta, sigma_t, wrap):
    rng = np.random.default_rng(5)
    n, h = 96, 1e-6
    args, spp = _case(rng, n, eta, sigma_t, wrap, 2)
    p, g, m, d, t, act, w, _, _, rcv, tex, _, vis = args
    _, _, pos = R.forward(*args)
    lit = pos[0] != R.NOWHERE
    # a lane within 5e-3 texel of a cell border changes its cell under a step of 1e-6 times a derivative of 1e3 at most
    far = lit & ~R.near_border(pos, BORDER)
    assert far.sum() > n // 3 and (~lit).sum() > 3 and (lit & ~far).sum() <= 0.2 * lit.sum()
    gi, gv = rng.normal(size=n // spp), rng.normal(size=n)

    def loss(pp, mm, ww, tx):
        value, image, _ = R.forward(pp, g, mm, d, t, act, ww, eta, sigma_t, rcv, tx, wrap, vis, spp)
        return (image * gi).sum() + (value * gv).sum()
    gm, gp, gw, gt = R.adjoint(*args, gi, gv, spp)
    assert not gm[:, ~lit].any() and not gp[:, ~lit].any() and not gw[~lit].any()
    # a sample's inputs move its own value only: the loss of lane i alone, so that the differences of the other lanes'
    # terms (equal, but 1e-16 of a sum of n of them) stay out of a quotient by 2e-6
    seed = np.repeat(gi, spp) / spp + gv

    def own(i, pp, mm, ww):
        value, _, _ = R.forward(pp, g, mm, d, t, act, ww, eta, sigma_t, rcv, tex, wrap, vis, spp)
        return value[i] * seed[i]
    worst = 0.0
    for i in np.flatnonzero(far):
        for c in range(3):
            e = np.zeros((3, n)); e[c, i] = h
            for got, fd, row in ((gm[c, i], (own(i, p, m + e, w) - own(i, p, m - e, w)) / (2 * h), gm),
                                 (gp[c, i], (own(i, p + e, m, w) - own(i, p - e, m, w)) / (2 * h), gp)):
                worst = max(worst, abs(fd - got) / max(abs(got), np.abs(row[:, i]).max()))
        e = np.zeros(n); e[i] = h
        fd = (own(i, p, m, w + e) - own(i, p, m, w - e)) / (2 * h)
        worst = max(worst, abs(fd - gw[i]) / max(abs(gw[i]), 1e-3))
    print("worst relative difference to central differences", worst)
    assert worst <= 1e-6
    # the texels: the value is linear in them, the cells do not move
    for j in range(tex.size):
        e = np.zeros(tex.size); e[j] = 0.5
        fd = loss(p, m, w, tex + e.reshape(tex.shape)) - loss(p, m, w, tex - e.reshape(tex.shape))
        assert abs(fd - gt.ravel()[j]) <= 1e-12 * max(1.0, abs(fd))
    assert np.count_nonzero(gt) > 10
    # the tangent against central differences of the forward, by direction, on the lanes away from the borders
    dn, dp, dw, dtex = rng.normal(size=(3, n)), rng.normal(size=(3, n)), rng.normal(size=n), rng.normal(size=tex.shape)
    dval, dimg = R.tangent(*args, dn, dp, dw, dtex, spp)
    fv, _, _ = R.forward(p + h * dp, g, m + h * dn, d, t, act, w + h * dw, eta, sigma_t, rcv, tex + h * dtex, wrap, vis, spp)
    bv, _, _ = R.forward(p - h * dp, g, m - h * dn, d, t, act, w - h * dw, eta, sigma_t, rcv, tex - h * dtex, wrap, vis, spp)
    fd = (fv - bv) / (2 * h)
    assert np.abs(fd - dval)[far].max() <= 1e-6 * np.abs(dval).max() and not dval[~lit].any()
    assert np.allclose(dimg, dval.reshape(-1, spp).mean(1), rtol=0, atol=1e-15)


@pytest.mark.parametrize("which", ["sh_n", "p", "weight", "tex", "all"])
@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("eta", [1.33, 1 / 1.33])
def test_tangent_is_the_transpose_of_the_adjoint(eta, below, which):
    rng = np.random.default_rng(9)
    n = 500
    dense = (eta < 1) != below                                     # the viewer sits in the denser medium: eta_ti > 1
    args, spp = _case(rng, n, eta, 0.7, R.REPEAT if below else R.CLAMP, 4, wavy=0.6 if dense else 0.3, below=below)
    _, _, pos = R.forward(*args)
    assert (pos[0] != R.NOWHERE).sum() > n // 4
    gi, gv = rng.normal(size=n // spp), rng.normal(size=n)
    dn = rng.normal(size=(3, n)) if which in ("sh_n", "all") else None
    dp = rng.normal(size=(3, n)) if which in ("p", "all") else None
    dw = rng.normal(size=n) if which in ("weight", "all") else None
    dtex = rng.normal(size=args[10].shape) if which in ("tex", "all") else None
    dval, dimg = R.tangent(*args, dn, dp, dw, dtex, spp)
    gm, gp, gw, gt = R.adjoint(*args, gi, gv, spp)
    lhs = (dimg * gi).sum() + (dval * gv).sum()
    rhs = sum(0.0 if t is None else (g * t).sum() for g, t in ((gm, dn), (gp, dp), (gw, dw), (gt, dtex)))
    assert abs(lhs) > 1e-3
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)

"""The restatement of the area-light row (tests/rect_ref.py) held against things that are not itself, on the CPU in float64:
central finite differences of its own forward, the transposition of its tangent and adjoint, the oracle's point light
in the small-lamp limit, the point light's gradient as the special case of dG/dp, the geometry of its shadow rays, and
the library's own n_l and A of the tests' lamps.
The GPU tests (tests/test_gpu_rect.py) then hold the kernels against the restatement."""
import numpy as np
import pytest

import rect_ref as A
from oracle import hf_oracle as O

N, K, SPP, SEED = 192, 8, 2, 11
TEX = A.textures(16, 8)


def _records(rng, n=N):
    """a synthetic wavefront: points over the unit square near the ground, shading normals within 40 degrees of +z, rays
    from above; every eighth sample a miss, every ninth seen from behind"""
    p = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0, 0.5, n)])
    sh_n = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), np.ones(n)])
    sh_n /= np.linalg.norm(sh_n, axis=0)
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), -np.ones(n)])
    d /= np.linalg.norm(d, axis=0)
    d[:, ::9] *= -1
    t = np.where(np.arange(n) % 8 == 7, np.inf, 1.0)
    return p, sh_n, d, t


@pytest.fixture(scope="module", params=["above", "side"])
def case(request):
    rng = np.random.default_rng(2)
    p, sh_n, d, t = _records(rng)
    lm = A.LAMPS[request.param](1.7)
    ids = np.arange(N, dtype=np.uint32)
    g = A.geometry(p, sh_n, A.draws(ids, K, SEED), lm)
    tr, margin = A.traced(sh_n, d, t, g)
    bits = tr & (rng.uniform(size=tr.shape) < 0.7)       # any visibility will do: it is an input
    x = A.inputs(N, SPP, TEX["smooth"].shape)
    for k, v in vars(x).items():            # (float64 steps: a float32 product h * dx would round the step itself)
        setattr(x, k, v.astype(np.float64))
    return dict(p=p, sh_n=sh_n, d=d, t=t, lm=lm, ids=ids, bits=bits, tr=tr, x=x, w=x.w.astype(np.float64), rmin=g.r[tr].min())


def _fwd(c, tex, **over):
    a = {**c, **over}
    return A.forward(a["p"], a["sh_n"], a["d"], a["t"], a["w"], c["bits"], c["ids"], SEED, c["lm"], tex, 0.8, SPP)[0]


@pytest.mark.parametrize("tex", [None, "smooth", "random"])
def test_tangent_equals_central_differences(case, tex):
    c, x = case, case["x"]
    texd = None if tex is None else TEX[tex].astype(np.float64)
    assert c["bits"].any() and c["tr"].mean() > 0.2
    dtex = None if tex is None else x.dtex.astype(np.float64)
    got = A.tangent(c["p"], c["sh_n"], c["d"], c["t"], c["w"], c["bits"], c["ids"], SEED, c["lm"], texd, 0.8, SPP,
                    x.dn, x.dp, x.dw, dtex)[0]
    h = 1e-4
    step = lambda s: _fwd(c, None if tex is None else texd + s * h * dtex, p=c["p"] + s * h * x.dp, sh_n=c["sh_n"] + s * h * x.dn,
                          w=c["w"] + s * h * x.dw)
    # central differences at h and 2 h, extrapolated: the h^2 terms cancel, what is left is h^4 f^(5) / 30 -- G falls off as
    # r^-2 with r >= 0.1 (asserted), so a fifth derivative along unit tangents is of the order 720 / r^5 = 7e7 times a value:
    # 1e-16 * 7e7 / 30 = 2e-10 -- and the rounding 1e-16 / h = 1e-12 of values of order one
    assert c["rmin"] >= 0.1, c["rmin"]
    fd = (4 * (step(1) - step(-1)) / (2 * h) - (step(2) - step(-2)) / (4 * h)) / 3
    assert np.abs(got - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), np.abs(got - fd).max()
    # every input on its own moves the image (no term is missing from both sides)
    for kw in (dict(dn=x.dn), dict(dp=x.dp), dict(dw=x.dw)) + (() if tex is None else (dict(dtex=dtex),)):
        one = A.tangent(c["p"], c["sh_n"], c["d"], c["t"], c["w"], c["bits"], c["ids"], SEED, c["lm"], texd, 0.8, SPP, **kw)[0]
        assert np.abs(one).max() > 1e-3, kw.keys()


@pytest.mark.parametrize("tex", [None, "random"])
def test_adjoint_is_the_transpose_of_the_tangent(case, tex):
    c, x = case, case["x"]
    texd = None if tex is None else TEX[tex].astype(np.float64)
    dtex = None if tex is None else x.dtex.astype(np.float64)
    args = (c["p"], c["sh_n"], c["d"], c["t"], c["w"], c["bits"], c["ids"], SEED, c["lm"], texd, 0.8, SPP)
    dimg = A.tangent(*args, x.dn, x.dp, x.dw, dtex)[0]
    gn, gp, gw, gtex = A.adjoint(*args, x.gi)
    lhs = float((dimg * x.gi).sum())
    rhs = float((gn * x.dn).sum() + (gp * x.dp).sum() + (gw * x.dw).sum() + (0.0 if tex is None else (gtex * dtex).sum()))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)
    # samples that are not eligible get exact zeros
    el, _ = A.eligible(c["sh_n"], c["d"], c["t"])
    assert (~el).any() and not gn[:, ~el].any() and not gp[:, ~el].any() and not gw[~el].any()


def test_a_lamp_that_faces_the_sample_has_the_point_lights_gradient():
    """c_l = 1 and n_l = -w: dG/dp = (3 c_s w - sh_n) / r^3 and G = c_s / r^2, the closed forms of
    oracle.point_lighting_adjoint"""
    rng = np.random.default_rng(4)
    for _ in range(8):
        p, sh_n = rng.uniform(-0.5, 0.5, (3, 1)), np.array([[0.2], [-0.1], [1.0]])
        sh_n = sh_n / np.linalg.norm(sh_n)
        q = np.array([0.3, -0.2, 1.4]) + rng.uniform(-0.1, 0.1, 3)
        w = (q[:, None] - p) / np.linalg.norm(q[:, None] - p)
        # a tiny lamp at q whose normal is -w: ex, ey span the plane across w
        a = np.cross(w[:, 0], [1.0, 0.0, 0.0]); a /= np.linalg.norm(a)
        b = np.cross(a, w[:, 0])                                  # a x b = -w
        lm = A.lamp(q, 1e-30 * a, 1e-30 * b)
        lm.center, lm.nl = q, -w[:, 0]                            # (no float32 rounding of the pose for this identity)
        g = A.geometry(p, sh_n, np.full((1, 2, 1), 0.5), lm)
        x = A._terms(p, sh_n, np.array([[0.0], [0.0], [-1.0]]), np.ones(1), None, np.ones((1, 1), bool), np.zeros(1, np.uint32), 0, lm, None,
                     np.float64)
        r, cs = g.r[0, 0], g.cs[0, 0]
        assert abs(g.cl[0, 0] - 1.0) < 1e-12
        assert np.allclose(x.Gp[0], (3 * cs * g.w[0] - sh_n) / r ** 3, rtol=1e-9, atol=0)  # (the lamp is too small for the draw to matter)
        assert np.allclose(x.G[0], cs / r ** 2, rtol=1e-9)


def test_small_lamp_limit_is_the_oracles_point_light():
    """A square lamp with half-extents e seen from r >> e is a point light of intensity L A c_l: to first order
    |G(q) - G(centre)| / G <= |grad_q log G| |q - centre| <= (4 + 1 / c_s + 1 / c_l) sqrt(2) e / r
    (grad_u log G = sh_n / <sh_n, u> - n_l / <n_l, u> - 4 u / r^2, three terms of norm 1 / (c_s r), 1 / (c_l r), 4 / r)."""
    rng = np.random.default_rng(6)
    p, sh_n, d, t = _records(rng)
    e, L = 1e-3, 2.5
    lm = A.lamp((0.1, -0.2, 1.6), (e, 0, 0), (0, -e, 0), L)        # faces down
    ids = np.arange(N, dtype=np.uint32)
    g = A.geometry(p, sh_n, A.draws(ids, K, SEED), lm)
    tr, _ = A.traced(sh_n, d, t, g)
    value = A.forward(p, sh_n, d, t, None, tr, ids, SEED, lm, None, 0.8, 1)[1]
    u = lm.center[:, None] - p
    r = np.linalg.norm(u, axis=0)
    cl, cs = -(lm.nl[:, None] * u).sum(0) / r, (sh_n * u).sum(0) / r
    ref = O.point_lighting(sh_n, p, d, t, [[*lm.center, L * lm.A]], albedo=0.8)[0] * cl
    keep = tr.all(0)                     # (a sample for which some draws are behind it is no point-light sample)
    assert keep.sum() > N // 2 and (ref[keep] > 0).all()
    bound = (4 + 1 / cs + 1 / cl) * np.sqrt(2) * e / r
    assert (np.abs(value - ref)[keep] <= bound[keep] * ref[keep] + 1e-12).all()
    assert np.abs(value[keep] / ref[keep] - 1).max() > 0               # (and they are not the same text)


def test_shadow_rays_end_just_short_of_the_lamp_and_masks_follow_the_cosines():
    rng = np.random.default_rng(8)
    p, sh_n, d, t = _records(rng)
    nrm = sh_n.copy()
    ids = np.arange(N, dtype=np.uint32)
    for name in ("above", "side"):
        lm = A.LAMPS[name]()
        assert np.dot(lm.nl, np.asarray(A.TARGET) - lm.center) > 0    # the lamp looks at the terrain
        some = 0
        for k in (0, 5):
            o, w, maxt, tr = A.rays(p, nrm, sh_n, d, t, ids, k, SEED, lm)
            s = A.draws(ids, k + 1, SEED)[k:k + 1]
            g = A.geometry(p, sh_n, s, lm)
            el, _ = A.eligible(sh_n, d, t)
            assert np.array_equal(tr, el & (g.cs[0] > 0) & (g.cl[0] > 0))
            assert np.allclose(np.linalg.norm(w[:, tr], axis=0), 1.0, atol=1e-12)
            end = o + w * (maxt / (1.0 - A.SHADOW_EPSILON))
            assert np.allclose(end[:, tr], g.q[0][:, tr], atol=1e-12)
            assert (maxt[~tr] == -1).all() and not o[:, ~tr].any() and not w[:, ~tr].any()
            # the origin is p moved along the normal by (1 + max|p|) RayEpsilon to the lamp's side
            off = np.linalg.norm(o - p, axis=0)[tr]
            assert np.allclose(off, ((1 + np.abs(p).max(0)) * A.S.RAY_EPSILON)[tr], rtol=1e-12)
            some += tr.sum()
        assert some > N // 4
        # points of the lamp: inside the rectangle, uniform in its own coordinates
        q = A.geometry(p, sh_n, A.draws(ids, 4, SEED), lm).q - lm.center[None, :, None]
        a = np.einsum("kcn,c->kn", q, lm.ex) / np.dot(lm.ex, lm.ex)
        assert np.abs(a).max() <= 1.0 + 1e-9 and abs(a.mean()) < 0.1
    # a lamp that faces away traces nothing
    away = A.lamp((0.2, -0.1, 1.1), (0.3, 0.0, 0.05), (0.0, 0.2, 0.0))
    assert away.nl[2] > 0
    g = A.geometry(p, sh_n, A.draws(ids, K, SEED), away)
    assert not A.traced(sh_n, d, t, g)[0].any()


def test_the_restatements_lamps_are_the_librarys():
    """n_l and A of the tests' lamps as the library forms them on the host (hf_rect_light_geometry, in double, rounded to
    float) against the restatement's, and the turned lamps face the terrain"""
    import hf_amd
    for name in A.LAMPS:
        lm = A.LAMPS[name](A.RADIANCE)
        area, nl = hf_amd.RectLight(lm.center, lm.ex, lm.ey, lm.radiance).geometry()
        assert area == np.float32(lm.A) and np.array_equal(np.asarray(nl, np.float32), lm.nl.astype(np.float32))
        assert np.dot(lm.nl, np.asarray(A.TARGET) - lm.center) > 0

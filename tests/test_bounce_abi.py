"""Bounce lighting (hf_bounce_rays, hf_bounce_lighting, _adjoint, _tangent) on the CPU: the four entry points are
declared, exported and bound; every bad argument is refused before anything touches a device; the float64 restatement
(tests/bounce_ref.py) draws unit cosine-weighted directions, gives weight * albedo when every direction sees a lit
facet that faces its light, its adjoint agrees with central differences of its own forward and its tangent is the
transpose of its adjoint."""
import ctypes as C

import numpy as np
import pytest

import bounce_ref as B
from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_bounce_rays", "hf_bounce_lighting", "hf_bounce_lighting_adjoint", "hf_bounce_lighting_tangent")


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS, ("bounce_lighting", "bounce_rays"))


# ---- argument checks: host addresses stand in for device pointers, every case fails before a launch ------------------
def _call(lib, fn, n=8, spp=2, num_rays=4, k=3, albedo=0.5, n_lights=2, stride=8, light=(0.0, 0.6, 0.8, 1.0), null=(),
          null_row=None):
    from hf_amd import _capi
    rows, arg = stand_ins(null, null_row)
    L = (_capi.hf_dir_light_t * 9)()
    for j in range(9):
        L[j].to_light[0], L[j].to_light[1], L[j].to_light[2], L[j].irradiance = (0.0, 0.0, 1.0, 1.0)
    L[1].to_light[0], L[1].to_light[1], L[1].to_light[2], L[1].irradiance = light
    lights = None if "lights" in null else L
    if fn == "hf_bounce_rays":
        tl = None if "to_light" in null else (C.c_float * 3)(*light[:3])
        return lib.hf_bounce_rays(arg("hf"), n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), k, 7, arg("ray_id"),
                                  tl, rows("out_o"), rows("out_d"), arg("out_maxt"), None)
    mid = (arg("weight"), num_rays, 7, arg("ray_id"), n_lights, lights, albedo)
    if fn == "hf_bounce_lighting":
        return lib.hf_bounce_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                      arg("image"), arg("hit_prim"), arg("lit_bits"), stride, None)
    head = (arg("hf"), n, spp, rows("sh_n"), rows("d"), arg("t"), *mid, arg("hit_prim"), arg("lit_bits"), stride)
    if fn == "hf_bounce_lighting_adjoint":
        return lib.hf_bounce_lighting_adjoint(*head, arg("grad_image"), rows("grad_sh_n"), arg("grad_weight"),
                                              arg("grad_heights"), None)
    return lib.hf_bounce_lighting_tangent(*head, rows("dsh_n"), arg("dweight"), arg("dheights"), arg("image"), None)


NAN, INF = float("nan"), float("inf")
LIGHTING = [{"n": 7}, {"spp": 0}, {"num_rays": 0}, {"num_rays": 33}, {"n": 1 << 32, "spp": 1, "stride": 1 << 32},
            {"n_lights": 0}, {"n_lights": 9}, {"stride": 7},
            {"albedo": NAN}, {"albedo": -INF}, {"light": (0.0, 0.6, 0.8, NAN)}, {"light": (0.0, 0.6, 0.8, INF)},
            {"light": (NAN, 0.6, 0.8, 1.0)}, {"light": (0.0, INF, 0.8, 1.0)},
            {"null": ("hf",)}, {"null": ("lights",)}, {"null": ("sh_n",)}, {"null": ("d",)}, {"null": ("t",)},
            {"null_row": "sh_n"}, {"null_row": "d"}]
CASES = {
    "hf_bounce_rays": [{"k": 32}, {"k": 0xFFFFFFFF}, {"n": 1 << 32}, {"light": (NAN, 0.0, 1.0, 1.0)}] +
                      [{"null": (x,)} for x in ("hf", "p", "nrm", "sh_n", "d", "t", "out_o", "out_d", "out_maxt")] +
                      [{"null_row": x} for x in ("p", "nrm", "sh_n", "d", "out_o", "out_d")],
    "hf_bounce_lighting": LIGHTING + [{"null": (x,)} for x in ("p", "nrm", "image")] +
                          [{"null_row": x} for x in ("p", "nrm")] + [{"stride": 7, "null": ("hit_prim",)}],
    "hf_bounce_lighting_adjoint": LIGHTING + [{"null": (x,)} for x in ("hit_prim", "lit_bits", "grad_image")] +
                                  [{"null_row": "grad_sh_n"}, {"null": ("grad_sh_n", "grad_weight", "grad_heights")}],
    "hf_bounce_lighting_tangent": LIGHTING + [{"null": (x,)} for x in ("hit_prim", "lit_bits", "image")] +
                                  [{"null_row": "dsh_n"}],
}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


def test_an_empty_wavefront_is_legal_before_any_device():
    """n == 0 returns HF_OK without reading the handle (a host stand-in here)"""
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        assert _call(lib, fn, n=0, stride=0) == _capi.HF_OK, fn


# ---- the float64 restatement ---------------------------------------------------------------------------------------
def test_directions_are_unit_cosine_weighted(oracle):
    """2^16 cosine-weighted directions: E[z] = 2/3, Var[z] = 1/2 - 4/9 = 1/18, so the mean has sigma =
    sqrt(1 / (18 * 65536)) = 0.00092; the issue's bound is 0.01"""
    n, K = 8192, 8
    rng = np.random.default_rng(0)
    sh_n = rng.normal(size=(3, n)); sh_n /= np.linalg.norm(sh_n, axis=0)
    sh_n[:, 0] = (0.0, 0.0, 1.0); sh_n[:, 1] = (0.0, 0.0, -1.0)
    wo = B.local_directions(np.arange(n), K, seed=5)
    assert np.abs(np.linalg.norm(wo, axis=1) - 1.0).max() < 1e-12 and wo[:, 2].min() >= 0
    print("mean z", wo[:, 2].mean())
    assert abs(wo[:, 2].mean() - 2.0 / 3.0) < 0.01
    assert np.abs(wo[:, :2].mean((0, 2))).max() < 0.01                    # (the disk is centred)
    w, z = B.directions(sh_n, np.arange(n), K, seed=5)
    assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() < 1e-12
    assert np.abs(np.einsum("cn,kcn->kn", sh_n, w) - z).max() < 1e-12     # the frame is orthonormal: <sh_n, w_k> = z_k
    s, t = B.coordinate_system(sh_n)
    assert np.abs((s * t).sum(0)).max() < 1e-12 and np.abs((s * sh_n).sum(0)).max() < 1e-12
    ids = rng.permutation(n)
    assert np.array_equal(B.local_directions(ids, 2, seed=5), wo[:2][:, :, ids])   # the stream follows the id
    assert not np.array_equal(B.local_directions(np.arange(n), 1, seed=6)[0], wo[0])


def test_lit_facets_facing_the_light_give_weight_times_albedo(oracle):
    """every direction hits a lit facet with n_q = l and E = pi / albedo: R = 1 and value = weight albedo exactly"""
    n, K, albedo = 64, 4, 0.6
    sh_n = np.zeros((3, n)); sh_n[2] = 1.0
    d = -sh_n; t = np.ones(n)
    l = np.array([0.0, 0.6, 0.8])
    lights = np.array([[*l, np.pi / albedo]])
    weight = np.random.default_rng(1).uniform(0.5, 1.5, n)
    hit = np.ones((K, n), bool); lit = np.ones((K, 1, n), bool)
    n_q = np.broadcast_to(l[None, :, None], (K, 3, n))
    image, value, _ = B.forward(sh_n, d, t, weight, hit, lit, n_q, lights, albedo, 4)
    assert np.allclose(value[0], weight * albedo, rtol=1e-14, atol=0)
    assert np.allclose(image[0], (weight * albedo).reshape(-1, 4).mean(1), rtol=1e-14, atol=0)
    # seen from behind, a miss at the first vertex, no hit of the bounce ray, or no light reaching it: dark
    assert B.forward(sh_n, -d, t, weight, hit, lit, n_q, lights, albedo, 4)[0].max() == 0
    assert B.forward(sh_n, d, np.full(n, np.inf), weight, hit, lit, n_q, lights, albedo, 4)[0].max() == 0
    assert B.forward(sh_n, d, t, weight, ~hit, lit, n_q, lights, albedo, 4)[0].max() == 0
    assert B.forward(sh_n, d, t, weight, hit, ~lit, n_q, lights, albedo, 4)[0].max() == 0


H, MAXH = 12, 0.5
LIGHTS = np.array([[0.3, 0.2, 0.9, 1.0], [-0.5, 0.4, 0.6, 0.7]])
LIGHTS[:, :3] /= np.linalg.norm(LIGHTS[:, :3], axis=1, keepdims=True)


def _case(rng, n, K, spp, flip=False):
    sh_n = rng.normal(size=(3, n)); sh_n[2] = np.abs(sh_n[2]) + 0.2; sh_n /= np.linalg.norm(sh_n, axis=0)
    d = rng.normal(size=(3, n)); d[2] = -np.abs(d[2]) - 0.1
    d[:, ::7] *= -1.0                                                      # some samples seen from behind
    t = rng.uniform(0.5, 3.0, n); t[rng.uniform(size=n) < 0.2] = np.inf
    w, z = B.directions(sh_n, np.arange(n), K, seed=3)
    heights = rng.uniform(0.0, 1.0, (H, H))
    prim = rng.integers(0, 2 * (H - 1) * (H - 1), (K, n))
    hit = B.traced(sh_n, d, t, z) & (rng.uniform(size=(K, n)) < 0.7)
    lit = hit[:, None, :] & (rng.uniform(size=(K, 2, n)) < 0.6)
    weight = rng.uniform(0.5, 1.5, n)
    gi = rng.normal(size=(2, n // spp))
    nq = lambda h: np.stack([B.face_normal(h, prim[k], MAXH, flip) for k in range(K)])
    return sh_n, d, t, weight, hit, lit, w, z, heights, prim, gi, nq


@pytest.mark.parametrize("flip", [False, True])
def test_adjoint_matches_central_differences_of_the_forward(oracle, flip):
    """records frozen, n_q recomputed from the perturbed heights; sh_n enters through the attached cosine"""
    rng = np.random.default_rng(3)
    n, K, spp, albedo = 32, 4, 4, 0.7
    sh_n, d, t, weight, hit, lit, w, z, heights, prim, gi, nq = _case(rng, n, K, spp, flip)
    adj = B.adjoint(sh_n, d, t, weight, hit, lit, nq(heights), LIGHTS, albedo, spp, w, z, gi)
    gh = sum(B.face_normal_vjp(heights, prim[k], MAXH, adj["grad_nq"][k], flip) for k in range(K))
    f = lambda a, q, h: (B.forward(sh_n, d, t, q, hit, lit, nq(h), LIGHTS, albedo, spp, attached=a, wz=(w, z))[0] * gi).sum()
    assert np.isclose(f(sh_n, weight, heights), (B.forward(sh_n, d, t, weight, hit, lit, nq(heights), LIGHTS, albedo, spp)[0] * gi).sum(),
                      rtol=1e-12)                                          # the attached factor is 1 at sh_n
    el, _ = B.eligible(sh_n, d, t)
    gn, gw = adj["grad_sh_n"], adj["grad_weight"]
    assert np.all(gn[:, ~el] == 0) and np.all(gw[~el] == 0) and np.abs(gn[:, el]).max() > 0 and np.abs(gh).max() > 0
    checked = 0
    for i in range(n):
        for c in range(3):
            e = np.zeros_like(sh_n); e[c, i] = 1e-6
            fd = (f(sh_n + e, weight, heights) - f(sh_n - e, weight, heights)) / 2e-6
            assert np.isclose(fd, gn[c, i], rtol=1e-6, atol=1e-9), (c, i, fd, gn[c, i])
        e = np.zeros(n); e[i] = 1e-6
        fd = (f(sh_n, weight + e, heights) - f(sh_n, weight - e, heights)) / 2e-6
        assert np.isclose(fd, gw[i], rtol=1e-6, atol=1e-9), (i, fd, gw[i])
        checked += el[i]
    assert checked > n // 3
    for i in range(H):
        for j in range(H):
            e = np.zeros_like(heights); e[i, j] = 1e-6
            fd = (f(sh_n, weight, heights + e) - f(sh_n, weight, heights - e)) / 2e-6
            assert np.isclose(fd, gh[i, j], rtol=1e-5, atol=1e-8), (i, j, fd, gh[i, j])


@pytest.mark.parametrize("which", ["sh_n", "weight", "heights", "all"])
@pytest.mark.parametrize("spp", [1, 4, 3])
def test_tangent_is_the_transpose_of_the_adjoint(oracle, spp, which):
    rng = np.random.default_rng(23)
    n, K, albedo = 300, 4, 0.8
    sh_n, d, t, weight, hit, lit, w, z, heights, prim, gi, nq = _case(rng, n, K, spp, flip=(spp == 3))
    flip = spp == 3
    dn = rng.normal(size=(3, n)) if which in ("sh_n", "all") else None
    dw = rng.normal(size=n) if which in ("weight", "all") else None
    dh = rng.normal(size=(H, H)) if which in ("heights", "all") else None
    dnq = np.stack([B.face_normal_jvp(heights, prim[k], MAXH, dh, flip) for k in range(K)]) if dh is not None else None
    dimage, _ = B.tangent(sh_n, d, t, weight, hit, lit, nq(heights), LIGHTS, albedo, spp, w, z, dn, dw, dnq)
    adj = B.adjoint(sh_n, d, t, weight, hit, lit, nq(heights), LIGHTS, albedo, spp, w, z, gi)
    lhs = (dimage * gi).sum()
    rhs = (0.0 if dn is None else (adj["grad_sh_n"] * dn).sum()) + (0.0 if dw is None else (adj["grad_weight"] * dw).sum())
    if dh is not None:
        rhs += sum((B.face_normal_vjp(heights, prim[k], MAXH, adj["grad_nq"][k], flip) * dh).sum() for k in range(K))
    assert abs(lhs) > 1e-6
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_face_normal_record_unpacking_and_origin(oracle):
    heights = np.zeros((3, 3)); heights[1, 1] = 1.0
    # tri 0 of cell 0: (v00, v10, v01) = (-1,-1,0), (0,-1,0), (-1,0,0): flat, facing +z; tri 1 holds the raised vertex
    assert np.allclose(B.face_normal(heights, np.array([0]), 0.5)[:, 0], (0, 0, 1))
    assert np.allclose(B.face_normal(heights, np.array([0]), 0.5, flip=True)[:, 0], (0, 0, -1))
    n1 = B.face_normal(heights, np.array([1]), 0.5)[:, 0]                 # (v11, v01, v10) = (0,0,.5), (-1,0,0), (0,-1,0)
    assert np.allclose(n1, np.array([-0.5, -0.5, 1.0]) / np.sqrt(1.5))
    vi, vj = B.prim_vertices(np.array([3]), 3)                            # cell (1, 0), tri 1
    assert vi[:, 0].tolist() == [1, 1, 0] and vj[:, 0].tolist() == [2, 1, 2]
    prim = np.array([[5, 0xFFFFFFFF]], np.uint32); bits = np.array([[0b101, 0]], np.uint8)
    hit, lit = B.unpack(prim, bits, 3)
    assert hit.tolist() == [[True, False]] and lit[0, :, 0].tolist() == [True, False, True] and not lit[0, :, 1].any()
    p = np.array([[0.5], [0.25], [-0.75]]); nrm = np.array([[0.0], [0.0], [1.0]])
    o = B.spawn_origin(p, nrm, np.array([[0.0], [0.6], [0.8]]))
    assert np.allclose(o[2], -0.75 + 1.75 * B.RAY_EPSILON, rtol=0, atol=1e-15)

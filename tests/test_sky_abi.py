"""Sky lighting (hf_sky_rays, hf_sky_lighting, _adjoint, _tangent) on the CPU: the four entry points are declared,
exported and bound; every bad argument is refused before anything touches a device; the float64 restatement
(tests/sky_ref.py) draws unit directions that average to zero, lights an unoccluded plane with albedo * L, its adjoint
agrees with central differences of its own forward and its tangent is the transpose of its adjoint."""
import numpy as np
import pytest

import sky_ref as S
from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_sky_rays", "hf_sky_lighting", "hf_sky_lighting_adjoint", "hf_sky_lighting_tangent")


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS, ("sky_lighting", "sky_rays"))


# ---- argument checks: host addresses stand in for device pointers, every case fails before a launch ------------------
ROWS = ("p", "nrm", "sh_n", "d", "out_o", "out_d", "grad_sh_n", "dsh_n")


def _call(lib, fn, n=8, spp=2, num_rays=8, k=3, radiance=1.0, albedo=0.5, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    mid = (arg("weight"), num_rays, 7, arg("ray_id"), radiance, albedo)
    if fn == "hf_sky_rays":
        return lib.hf_sky_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), k, 7, arg("ray_id"),
                               rows("out_o"), rows("out_d"), arg("out_maxt"), None)
    if fn == "hf_sky_lighting":
        return lib.hf_sky_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                   arg("image"), arg("vis_bits"), None)
    head = (n, spp, rows("sh_n"), rows("d"), arg("t"), *mid, arg("vis_bits"))
    if fn == "hf_sky_lighting_adjoint":
        return lib.hf_sky_lighting_adjoint(*head, arg("grad_image"), rows("grad_sh_n"), arg("grad_weight"), None)
    return lib.hf_sky_lighting_tangent(*head, rows("dsh_n"), arg("dweight"), arg("image"), None)


LIGHTING = [{"n": 7}, {"spp": 0}, {"num_rays": 0}, {"num_rays": 33}, {"n": 1 << 32, "spp": 1},
            {"radiance": float("nan")}, {"radiance": float("inf")}, {"albedo": float("nan")}, {"albedo": float("-inf")},
            {"null": ("sh_n",)}, {"null": ("d",)}, {"null": ("t",)}, {"null_row": "sh_n"}, {"null_row": "d"}]
CASES = {
    "hf_sky_rays": [{"k": 32}, {"k": 0xFFFFFFFF}, {"n": 1 << 32}] +
                   [{"null": (x,)} for x in ("p", "nrm", "sh_n", "d", "t", "out_o", "out_d", "out_maxt")] +
                   [{"null_row": x} for x in ("p", "nrm", "sh_n", "d", "out_o", "out_d")],
    "hf_sky_lighting": LIGHTING + [{"null": (x,)} for x in ("hf", "p", "nrm", "image")] +
                       [{"null_row": x} for x in ("p", "nrm")],
    "hf_sky_lighting_adjoint": LIGHTING + [{"null": (x,)} for x in ("vis_bits", "grad_image", "grad_sh_n")] +
                               [{"null_row": "grad_sh_n"}],
    "hf_sky_lighting_tangent": LIGHTING + [{"null": (x,)} for x in ("vis_bits", "image")] + [{"null_row": "dsh_n"}],
}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def test_sample_stream_is_the_oracles(oracle):
    rng = np.random.default_rng(2)
    v0 = rng.integers(0, 1 << 32, 64, dtype=np.uint64); v1 = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    v0[:3] = (0, 0xFFFFFFFF, 7); v1[:3] = (0, 0xFFFFFFFF, 0)
    r0, r1 = S.tea32(v0, v1)
    for i in range(64):
        assert (int(r0[i]), int(r1[i])) == oracle.sample_tea_32(int(v0[i]), int(v1[i]))
    sx, sy = S.samples(np.arange(1000), 3, 11)
    assert sx.min() >= 0 and sx.max() < 1 and sy.min() >= 0 and sy.max() < 1
    key = oracle.sample_tea_32(11, 3)[0]
    a, b = oracle.sample_tea_32(key, 999)
    assert sx[999] == (a >> 9) * 2.0 ** -23 and sy[999] == (b >> 9) * 2.0 ** -23


def test_directions_are_unit_and_average_to_zero(oracle):
    """2^16 uniform directions: every component has variance 1/3, so the mean has sigma = 1 / sqrt(3 * 65536) = 0.00226;
    4.5 sigma = 0.0102, rounded up to 0.02"""
    w = S.directions(np.arange(8192), 8, seed=5)                         # [8, 3, 8192]
    assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() < 1e-12
    mean = w.transpose(1, 0, 2).reshape(3, -1).mean(1)
    print("mean direction", mean)
    assert np.abs(mean).max() < 0.02
    ids = np.random.default_rng(0).permutation(8192)
    assert np.array_equal(S.directions(ids, 2, seed=5), w[:2][:, :, ids])   # the stream follows the id, not the position
    assert not np.array_equal(S.directions(np.arange(8192), 1, seed=6)[0], w[0])


def test_unoccluded_plane_averages_to_albedo_times_radiance(oracle):
    """value = 4 albedo L max(0, z) per draw: E = albedo L (E[max(0, z)] = 1/4), E[(4 z+)^2] = 16 / 6, so one draw has
    sigma = sqrt(8/3 - 1) albedo L = 1.291 albedo L and the mean of 2^16 draws 1.291 / 256 = 0.00504 albedo L;
    4.5 sigma = 0.0227, rounded up to 0.025 albedo L"""
    n, K, L, albedo = 8192, 8, 2.5, 0.6
    w = S.directions(np.arange(n), K, seed=9)
    sh_n = np.zeros((3, n)); sh_n[2] = 1.0
    d = -sh_n; t = np.ones(n)
    bits, _ = S.traced(sh_n, d, t, w)                                     # nothing occludes: every traced direction is visible
    image, value = S.forward(sh_n, d, t, None, bits, w, L, albedo, 4)
    assert image.shape == (n // 4,) and np.allclose(image, value.reshape(-1, 4).mean(1))
    print("plane mean", image.mean(), "expected", albedo * L)
    assert abs(image.mean() - albedo * L) < 0.025 * albedo * L
    # seen from behind, or a miss: dark
    assert S.forward(sh_n, -d, t, None, bits, w, L, albedo, 4)[0].max() == 0
    assert S.forward(sh_n, d, np.full(n, np.inf), None, bits, w, L, albedo, 4)[0].max() == 0


def _case(rng, n, K, spp):
    sh_n = rng.normal(size=(3, n)); sh_n[2] = np.abs(sh_n[2]) + 0.2; sh_n /= np.linalg.norm(sh_n, axis=0)
    d = rng.normal(size=(3, n)); d[2] = -np.abs(d[2]) - 0.1
    d[:, ::7] *= -1.0                                                      # some samples seen from behind
    t = rng.uniform(0.5, 3.0, n); t[rng.uniform(size=n) < 0.2] = np.inf
    w = S.directions(np.arange(n), K, seed=3)
    tr, _ = S.traced(sh_n, d, t, w)
    bits = tr & (rng.uniform(size=(K, n)) < 0.6)
    weight = rng.uniform(0.5, 1.5, n)
    gi = rng.normal(size=n // spp)
    return sh_n, d, t, weight, bits, w, gi


def test_adjoint_matches_central_differences_of_the_forward(oracle):
    rng = np.random.default_rng(3)
    n, K, spp = 64, 8, 4
    sh_n, d, t, weight, bits, w, gi = _case(rng, n, K, spp)
    gn, gw = S.adjoint(sh_n, d, t, weight, bits, w, 1.7, 0.7, spp, gi)
    f = lambda x, q: (S.forward(x, d, t, q, bits, w, 1.7, 0.7, spp)[0] * gi).sum()
    el, _ = S.eligible(sh_n, d, t)
    assert np.all(gn[:, ~el] == 0) and np.all(gw[~el] == 0) and np.abs(gn[:, el]).max() > 0
    checked = 0
    for i in range(n):
        for c in range(3):
            e = np.zeros_like(sh_n); e[c, i] = 1e-6
            fd = (f(sh_n + e, weight) - f(sh_n - e, weight)) / 2e-6
            assert np.isclose(fd, gn[c, i], rtol=1e-6, atol=1e-9), (c, i, fd, gn[c, i])
        e = np.zeros(n); e[i] = 1e-6
        fd = (f(sh_n, weight + e) - f(sh_n, weight - e)) / 2e-6
        assert np.isclose(fd, gw[i], rtol=1e-6, atol=1e-9), (i, fd, gw[i])
        checked += el[i]
    assert checked > n // 3


@pytest.mark.parametrize("which", ["sh_n", "weight", "both"])
@pytest.mark.parametrize("spp", [1, 4, 3])
def test_tangent_is_the_transpose_of_the_adjoint(oracle, spp, which):
    rng = np.random.default_rng(23)
    n, K = 300, 8
    sh_n, d, t, weight, bits, w, gi = _case(rng, n, K, spp)
    dn = rng.normal(size=(3, n)) if which in ("sh_n", "both") else None
    dw = rng.normal(size=n) if which in ("weight", "both") else None
    dimage = S.tangent(sh_n, d, t, weight, bits, w, 1.3, 0.8, spp, dn, dw)
    gn, gw = S.adjoint(sh_n, d, t, weight, bits, w, 1.3, 0.8, spp, gi)
    lhs = (dimage * gi).sum()
    rhs = (0.0 if dn is None else (gn * dn).sum()) + (0.0 if dw is None else (gw * dw).sum())
    assert abs(lhs) > 1e-6
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_spawned_origin_and_bit_packing(oracle):
    p = np.array([[0.5, -2.0], [0.25, 0.5], [-0.75, 1.0]]); nrm = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]])
    up = np.array([[0.0, 0.0], [0.6, 0.6], [0.8, -0.8]])
    o = S.spawn_origin(p, nrm, up)
    assert np.allclose(o[2], [-0.75 + 1.75 * S.RAY_EPSILON, 1.0 - 3.0 * S.RAY_EPSILON], rtol=0, atol=1e-15)
    assert np.array_equal(o[:2], p[:2])
    words = np.array([0b101, 0x80000000], np.uint32)
    b = S.unpack(words, 32)
    assert b[0, 0] and not b[1, 0] and b[2, 0] and b[31, 1] and b.sum() == 3

"""The spot row's restatement (tests/spot_ref.py) held against itself and against what it must reduce to, on the CPU: the
header's closed form against sample_direction's steps, the closed tangents against extrapolated central differences in
every variable, the reverse sweep against the tangent, a light with cutoff = beam = 180 against the oracle's point light,
a hard edge's angle gradients, the masks of a handful of lanes, and -- on the oracle's records of the GPU test's four
scenes -- the shares that tests/test_gpu_spot.py asserts before it compares anything."""
import numpy as np
import pytest

import spot_ref as P
from oracle import hf_oracle as O

N = 96
ZONED = ("above", "side", "wide", "graze", "near", "back")


def _points(L, n=N, seed=3, zone=None):
    """points inside the cone at distance 0.6 .. 2.5 (zone: True only the transition zone, False only the full beam), away
    from theta = beam and from the cutoff, unit normals that face the light, float32 values"""
    rng = np.random.default_rng(seed)
    cut, beam = np.deg2rad(L.cutoff), np.deg2rad(L.beam)
    lo, hi = 0.02, min(cut, 3.0) - 0.02
    if zone is True:
        lo = beam + 0.02
    if zone is False:
        hi = beam - 0.02
    th = rng.uniform(lo, hi, n)
    th = np.where(np.abs(th - beam) < 0.02, beam - 0.03, th) if zone is None and L.cutoff > L.beam else th
    ph, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.6, 2.5, n)
    ref = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]) * r
    p = (L.to_world[:, :3] @ ref + L.to_world[:, 3:4]).astype(np.float32)
    u = L.to_world[:, 3:4] - p
    sn = u / np.linalg.norm(u, axis=0) + 0.4 * rng.standard_normal((3, n))
    sn = (sn / np.linalg.norm(sn, axis=0)).astype(np.float32)
    keep = (sn * u).sum(0) > 0.05
    return p[:, keep], sn[:, keep]


@pytest.fixture(scope="module", params=P.NAMES)
def case(request):
    L = P.rig((request.param,))[0]
    p, sn = _points(L)
    return request.param, L, p, sn, P.inputs(p.shape[1], 1, 1)


def test_closed_form_is_the_steps_value(case):
    name, L, p, sn, x = case
    vis = np.ones((1, p.shape[1]), bool)
    value = P.steps(L, p, sn, x.w, P.ALBEDO)
    closed = P.forward([L], p, sn, x.w, P.ALBEDO, vis)[1][0]
    m = P.mapping(L, p)
    assert m.lit.all() and (name in ("hard", "point")) == (not m.zone.any())
    # (acos of a cosine near 1 loses half the digits: the zone's values agree to 1e-8 of the ramp, the beam's to rounding)
    assert np.abs(closed / value - 1)[m.full].max(initial=0) <= 1e-13 and np.abs(closed / value - 1).max() <= 1e-7


def _extrapolated(f, h=1e-3):
    """central differences at h and h / 2, Richardson-extrapolated: the error is O(h^4)"""
    d1, d2 = (f(h) - f(-h)) / (2 * h), (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


def test_tangent_against_central_differences_in_every_variable(case):
    name, L, p, sn, x = case
    n = p.shape[1]
    vis = np.ones((1, n), bool)
    p64, sn64, w64 = (np.asarray(a, np.float64) for a in (p, sn, x.w))
    rng = np.random.default_rng(9)
    d15 = np.zeros((3, P.PARAMS))
    d15[0, :12], d15[1, 12], d15[2, 13:] = 0.3 * rng.standard_normal(12), -0.4, (0.7, -0.5)
    dirs = {"dn": rng.standard_normal((3, n)), "dp": 0.2 * rng.standard_normal((3, n)), "dw": rng.standard_normal(n),
            "to_world": d15[0], "intensity": d15[1], "angles": d15[2]}

    def value(key, s):
        row = P.row15(L) + (s * dirs[key] if key in ("to_world", "intensity", "angles") else 0)
        q = P.light(row[:12].reshape(3, 4))
        q.intensity, q.cutoff, q.beam = row[12:]
        if L.cutoff == L.beam:
            q.beam = q.cutoff           # (a hard edge stays one: the derivative holds the branch)
        return P.forward([q], p64 + (s * dirs["dp"] if key == "dp" else 0), sn64 + (s * dirs["dn"] if key == "dn" else 0),
                         w64 + (s * dirs["dw"] if key == "dw" else 0), P.ALBEDO, vis)[1][0]

    for key, direction in dirs.items():
        kw = {key: direction} if key in ("dn", "dp", "dw") else {"d_lights": direction[None]}
        dv = P.tangent([L], p64, sn64, w64, P.ALBEDO, vis, **kw)[1][0]
        fd = _extrapolated(lambda s: value(key, s), 2e-4)
        assert np.abs(dv - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), (name, key)
        assert np.abs(dv).max() > 0 or (key == "angles" and name in ("hard", "point")), (name, key)


def _rig_points(K=8, per=24):
    """the whole rig on the union of points drawn for each light, a random visibility"""
    lights = P.rig()
    pts = [_points(L, per, seed=11 + k) for k, L in enumerate(lights)]
    p, sn = np.concatenate([a for a, _ in pts], 1), np.concatenate([b for _, b in pts], 1)
    n = p.shape[1] - p.shape[1] % 2
    p, sn = p[:, :n], sn[:, :n]
    vis = np.stack([P.steady(L, p, P.mapping(L, p).lit) for L in lights]) & (np.random.default_rng(4).random((K, n)) < 0.8)
    return lights, p, sn, vis


@pytest.mark.parametrize("spp", (1, 2))
def test_adjoint_is_the_transpose_of_the_tangent(spp):
    lights, p, sn, vis = _rig_points()
    n, K = p.shape[1], len(lights)
    x = P.inputs(n, spp, K)
    dimg, dv = P.tangent(lights, p, sn, x.w, P.ALBEDO, vis, spp, dn=x.dn, dp=x.dp, dw=x.dw, d_lights=x.dl)
    g = P.adjoint(lights, p, sn, x.w, P.ALBEDO, vis, spp, grad_image=x.gi, grad_value=x.gv)
    f64 = lambda a: np.asarray(a, np.float64)
    lhs = (dv * f64(x.gv)).sum() + (dimg * f64(x.gi)).sum()
    rhs = (g.gn * f64(x.dn)).sum() + (g.gp * f64(x.dp)).sum() + (g.gw * f64(x.dw)).sum() + (g.g15 * f64(x.dl)).sum()
    scale = np.abs(dv * f64(x.gv)).sum() + np.abs(dimg * f64(x.gi)).sum()
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale
    dark = ~vis.any(0)
    assert dark.any() and not g.gn[:, dark].any() and not g.gp[:, dark].any() and not g.gw[dark].any()
    assert np.abs(g.g15[[k for k, nm in enumerate(P.NAMES) if nm in ZONED]]).min() > 0
    # the sums over a slice of the rows are the slice's own
    part = P.adjoint(lights, p[:, :40], sn[:, :40], x.w[:40], P.ALBEDO, vis[:, :40], 1, grad_value=x.gv[:, :40])
    rows = P.adjoint(lights, p, sn, x.w, P.ALBEDO, vis, 1, grad_value=x.gv, rows=slice(0, 40))
    assert np.allclose(part.g15, rows.g15, rtol=1e-12, atol=1e-14)
    # a light's numbers do not depend on its neighbours
    alone = P.adjoint(lights[2:3], p, sn, x.w, P.ALBEDO, vis[2:3], spp, grad_image=x.gi[2:3], grad_value=x.gv[2:3])
    assert np.array_equal(alone.g15[0], g.g15[2])


def test_a_light_with_cutoff_and_beam_at_180_is_the_point_light():
    """exact, not a bound: the oracle's point_lighting (albedo / pi intensity <sh_n, l> / r^2) and hf_point_lighting's
    closed derivative (3 <sh_n, l> l - sh_n) / r^3 for dc = 0"""
    L = P.rig(("point",))[0]
    p, sn = _points(L)
    n = p.shape[1]
    vis = np.ones((1, n), bool)
    value = P.forward([L], p, sn, None, P.ALBEDO, vis)[1][0]
    assert P.mapping(L, p).full.all()
    d, t = -np.asarray(sn, np.float64), np.ones(n)
    row = np.append(L.to_world[:, 3], L.intensity)
    for i in range(0, n, 7):
        ref = O.point_lighting(sn[:, i:i + 1], p[:, i:i + 1], d[:, i:i + 1], t[i:i + 1], row, albedo=P.ALBEDO)[0, 0]
        assert abs(value[i] - ref) <= 1e-13 * abs(ref)
    g = P.adjoint([L], p, sn, None, P.ALBEDO, vis, grad_value=np.ones((1, n)))
    u = L.to_world[:, 3:4] - p.astype(np.float64)
    r = np.linalg.norm(u, axis=0)
    l, s = u / r, np.asarray(sn, np.float64)
    closed = P.ALBEDO / np.pi * L.intensity * (3 * (s * l).sum(0) * l - s) / r ** 3
    assert np.abs(g.gp - closed).max() <= 1e-13 * np.abs(closed).max()
    assert g.g15[0, 13] == 0 and g.g15[0, 14] == 0


@pytest.mark.parametrize("name", ("hard", "point"))
def test_a_hard_edge_has_exact_zeros_for_both_angle_gradients_and_no_nan(name):
    L = P.rig((name,))[0]
    p, sn = _points(L)
    n = p.shape[1]
    x = P.inputs(n, 1, 1)
    vis = np.ones((1, n), bool)
    for dtype in (np.float64, np.float32):
        r = P.evaluate([L], {"p": p, "sh_n": sn}, x, vis, 1, dtype)
        # (f = 1 wherever the light is seen: only c and the intensity move the value)
        assert r.g15[0, 13] == 0 and r.g15[0, 14] == 0 and np.abs(r.g15[0, [3, 7, 11, 12]]).min() > 0
        for a in (r.image, r.value, r.dimage, r.dvalue, r.gn, r.gp, r.gw, r.g15):
            assert np.isfinite(a).all()
    only = np.zeros((1, P.PARAMS))
    only[0, 13:] = (1.0, -2.0)
    assert not P.tangent([L], p, sn, None, P.ALBEDO, vis, d_lights=only)[1].any()


def test_masks_and_rays_of_a_handful_of_lanes():
    """lanes behind the light, outside the cone, facing away and missed are not traced; a traced lane's ray ends just short
    of the light; the falloff is 1 on the axis, 1/2 in the middle of the zone and 0 at the cutoff"""
    L = P.rig(("above",))[0]
    A, c = L.to_world[:, :3], L.to_world[:, 3]
    inside = c + 1.5 * A[:, 2]
    p = np.stack([inside, c - 1.0 * A[:, 2], c + 1.5 * A[:, 2] + 2.0 * A[:, 0], inside, inside], axis=1).astype(np.float32)
    to_c = (c - inside) / np.linalg.norm(c - inside)
    sn = np.stack([to_c, to_c, to_c, -to_c, to_c], axis=1).astype(np.float32)
    d = -sn
    d[:, 3] = sn[:, 3]          # (seen from the front, but the normal faces away from the light)
    t = np.array([1, 1, 1, 1, np.inf], np.float32)
    tr, unsure = P.traced(L, p, sn, d, t)
    assert tr.tolist() == [True, False, False, False, False] and not unsure.any()
    o, w, maxt, tr2 = P.rays(L, p, sn, sn, d, t)
    assert np.array_equal(tr, tr2) and (maxt[1:] == -1).all() and not o[:, 1:].any() and not w[:, 1:].any()
    assert abs(np.linalg.norm(o[:, 0] + w[:, 0] * maxt[0] / (1 - P.PR.SHADOW_EPSILON) - c.astype(np.float32))) <= 1e-12
    th = np.deg2rad([0.0, 17.5, 20.0, 14.0])
    q = (c[:, None] + A @ np.stack([np.sin(th), 0 * th, np.cos(th)]))
    f = P.mapping(L, q).f
    assert np.allclose(f[[0, 3]], 1) and abs(f[1] - 0.5) <= 1e-6 and abs(f[2]) <= 1e-6
    # value on the axis at distance 1, facing the light: albedo / pi intensity
    v = P.forward([L], q[:, :1], -A[:, 2:3], None, P.ALBEDO, np.ones((1, 1), bool))[1][0, 0]
    assert abs(v - P.ALBEDO / np.pi * L.intensity) <= 1e-13


def test_the_shares_of_the_rig_on_the_oracles_records_of_the_gpu_tests_scenes():
    lights = P.rig()
    for key, rec, r, t, field in P.oracle_scenes():
        shares, union, kink = {}, np.zeros(len(t), bool), 0.0
        for name, L in zip(P.NAMES, lights):
            q = P.probe(L, rec, r, t, field)
            shares[name], union, kink = q.shares, union | q.unsure, max(kink, q.shares["kink_share"])
        print(key, "unsure union", union.mean(), "kink", kink, {k: "%.3f %.3f %.3f" % (v["in_cone_of_eligible"], v["zone_of_traced"],
                                                                                    v["occluded_of_traced"]) for k, v in shares.items()})
        P.assert_shares(shares, float(union.mean()))
        assert kink <= 1e-3 and shares["point"]["in_cone_of_eligible"] == 1.0

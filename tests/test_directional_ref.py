"""The directional row's restatement (tests/directional_ref.py) held against itself and against what it must reduce to,
on the CPU: the closed tangents against extrapolated central differences in every variable, the reverse sweep against the
tangent, the known answers (a flat field under the zenith light, the length of to_light, the orthogonality of its
gradient, the reference's `direction`), the masks and rays of a handful of lanes, and -- on the oracle's records of the
GPU test's four scenes -- the shares that tests/test_gpu_directional.py asserts before it compares anything."""
import numpy as np
import pytest

import directional_ref as D

N = 96


def _samples(L, n=N, seed=3):
    """unit normals that face the light, float32 values"""
    rng = np.random.default_rng(seed)
    l, _ = D.unit(L)
    sn = l[:, None] + 0.6 * rng.standard_normal((3, n))
    sn = (sn / np.linalg.norm(sn, axis=0)).astype(np.float32)
    return sn[:, (sn * l[:, None]).sum(0) > 0.05]


@pytest.fixture(scope="module", params=D.NAMES)
def case(request):
    L = D.rig((request.param,))[0]
    sn = _samples(L)
    return request.param, L, sn, D.inputs(sn.shape[1], 1, 1)


def _extrapolated(f, h=1e-3):
    """central differences at h and h / 2, Richardson-extrapolated: the error is O(h^4)"""
    d1, d2 = (f(h) - f(-h)) / (2 * h), (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


def test_tangent_against_central_differences_in_every_variable(case):
    name, L, sn, x = case
    n = sn.shape[1]
    vis = np.ones((1, n), bool)
    sn64, w64 = np.asarray(sn, np.float64), np.asarray(x.w, np.float64)
    rng = np.random.default_rng(9)
    d4 = np.zeros((2, D.PARAMS))
    d4[0, :3], d4[1, 3] = 0.3 * rng.standard_normal(3), -0.4
    dirs = {"dn": rng.standard_normal((3, n)), "dw": rng.standard_normal(n), "to_light": d4[0], "irradiance": d4[1]}

    def value(key, s):
        row = D.row4(L) + (s * dirs[key] if key in ("to_light", "irradiance") else 0)
        q = D.light(row[:3])
        q.irradiance = row[3]
        return D.forward([q], sn64 + (s * dirs["dn"] if key == "dn" else 0), w64 + (s * dirs["dw"] if key == "dw" else 0),
                         D.ALBEDO, vis)[1][0]

    for key, direction in dirs.items():
        kw = {key: direction} if key in ("dn", "dw") else {"d_lights": direction[None]}
        dv = D.tangent([L], sn64, w64, D.ALBEDO, vis, **kw)[1][0]
        fd = _extrapolated(lambda s: value(key, s), 2e-4)
        assert np.abs(dv - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), (name, key)
        assert np.abs(dv).max() > 0, (name, key)


def _rig_samples(K=8, per=24):
    """the whole rig on the union of the normals drawn for each light, a random visibility"""
    lights = D.rig()
    sn = np.concatenate([_samples(L, per, seed=11 + k) for k, L in enumerate(lights)], 1)
    n = sn.shape[1] - sn.shape[1] % 2
    sn = sn[:, :n]
    facing = np.stack([(np.asarray(sn, np.float64) * D.unit(L)[0][:, None]).sum(0) > 0 for L in lights])
    return lights, sn, facing & (np.random.default_rng(4).random((K, n)) < 0.6)


@pytest.mark.parametrize("spp", (1, 2))
def test_adjoint_is_the_transpose_of_the_tangent(spp):
    lights, sn, vis = _rig_samples()
    n, K = sn.shape[1], len(lights)
    x = D.inputs(n, spp, K)
    dimg, dv = D.tangent(lights, sn, x.w, D.ALBEDO, vis, spp, dn=x.dn, dw=x.dw, d_lights=x.dl)
    g = D.adjoint(lights, sn, x.w, D.ALBEDO, vis, spp, grad_image=x.gi, grad_value=x.gv)
    f64 = lambda a: np.asarray(a, np.float64)
    lhs = (dv * f64(x.gv)).sum() + (dimg * f64(x.gi)).sum()
    rhs = (g.gn * f64(x.dn)).sum() + (g.gw * f64(x.dw)).sum() + (g.g4 * f64(x.dl)).sum()
    scale = np.abs(dv * f64(x.gv)).sum() + np.abs(dimg * f64(x.gi)).sum()
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale
    dark = ~vis.any(0)
    assert dark.any() and not g.gn[:, dark].any() and not g.gw[dark].any()
    # (zenith's l is the z axis: the component of its gradient along it is an exact zero, the orthogonality at its plainest)
    assert g.g4[0, 2] == 0 and np.abs(np.delete(g.g4.reshape(-1), 2)).min() > 0
    # the sums over a slice of the rows are the slice's own
    part = D.adjoint(lights, sn[:, :40], x.w[:40], D.ALBEDO, vis[:, :40], 1, grad_value=x.gv[:, :40])
    rows = D.adjoint(lights, sn, x.w, D.ALBEDO, vis, 1, grad_value=x.gv, rows=slice(0, 40))
    assert np.allclose(part.g4, rows.g4, rtol=1e-12, atol=1e-14)
    # adjoint rows added in parts equal the whole
    rest = D.adjoint(lights, sn, x.w, D.ALBEDO, vis, 1, grad_value=x.gv, rows=slice(40, None))
    whole = D.adjoint(lights, sn, x.w, D.ALBEDO, vis, 1, grad_value=x.gv)
    assert np.allclose(rows.g4 + rest.g4, whole.g4, rtol=1e-12, atol=1e-14)
    # a light's numbers do not depend on its neighbours
    alone = D.adjoint(lights[2:3], sn, x.w, D.ALBEDO, vis[2:3], spp, grad_image=x.gi[2:3], grad_value=x.gv[2:3])
    assert np.array_equal(alone.g4[0], g.g4[2])


def test_a_flat_field_under_the_zenith_light_has_the_known_value():
    L = D.rig(("zenith",))[0]
    n = 5
    sn = np.tile(np.array([[0.0], [0.0], [1.0]], np.float32), (1, n))
    d, t = -sn, np.ones(n, np.float32)
    tr, unsure = D.traced(L, sn, d, t)
    assert tr.all() and not unsure.any()
    image, value = D.forward([L], sn, None, D.ALBEDO, tr[None])
    assert np.abs(value - D.ALBEDO / np.pi * L.irradiance).max() <= 1e-13 and np.array_equal(image, value)


def test_the_length_of_to_light_changes_no_output_and_divides_its_gradient(case):
    name, L, sn, x = case
    n = sn.shape[1]
    vis = np.random.default_rng(2).random((1, n)) < 0.7
    twice = D.light(2 * L.to_light, L.irradiance)
    a, b = (D.evaluate([q], {"sh_n": sn}, x, vis, 1) for q in (L, twice))
    for k in ("image", "value", "gn", "gw"):
        assert np.allclose(getattr(a, k), getattr(b, k), rtol=1e-15, atol=0), k
    # (the tangent of to_light in evaluate() is the same dv for both: its effect halves as the gradient does)
    assert np.allclose(a.g4[0, :3], 2 * b.g4[0, :3], rtol=1e-13, atol=0) and np.allclose(a.g4[0, 3], b.g4[0, 3], rtol=1e-15)
    l, length = D.unit(L)
    assert np.abs(a.g4[0, :3]).max() > 0
    assert abs(a.g4[0, :3] @ l) <= 1e-13 * np.abs(a.g4[0, :3]).max()      # orthogonal to l, to rounding
    # a tangent along to_light moves nothing (dl is a few ulps of |to_light| <= 2.7, the factor before it at most 1.6)
    along = np.append(L.to_light, 0.0)[None]
    assert np.abs(D.tangent([L], sn, x.w, D.ALBEDO, vis, d_lights=along)[1]).max() <= 1e-14


def test_from_direction_is_the_light_with_the_opposite_to_light(case):
    _, L, sn, x = case
    M = D.from_direction(-L.to_light, L.irradiance)
    assert np.array_equal(M.to_light, L.to_light) and M.irradiance == L.irradiance
    vis = np.ones((1, sn.shape[1]), bool)
    assert np.array_equal(D.forward([M], sn, x.w, D.ALBEDO, vis)[1], D.forward([L], sn, x.w, D.ALBEDO, vis)[1])


def test_masks_and_rays_of_a_handful_of_lanes():
    """lanes that face away, are seen from behind or were missed are not traced; a traced lane's ray leaves from the side
    of the geometric normal that the light is on, along float32(l), and never ends"""
    L = D.rig(("unnorm",))[0]
    l, length = D.unit(L)
    assert abs(length - np.sqrt(7.25)) <= 1e-15 and abs(np.linalg.norm(l) - 1) <= 1e-15
    sn = np.stack([l, -l, l, l, l], axis=1).astype(np.float32)
    d = -sn.copy()
    d[:, 1] = sn[:, 1]          # (seen from the front, but the normal faces away from the light)
    d[:, 2] = sn[:, 2]          # (seen from behind)
    t = np.array([1, 1, 1, np.inf, 1], np.float32)
    tr, unsure = D.traced(L, sn, d, t)
    assert tr.tolist() == [True, False, False, False, True] and not unsure.any()
    p = np.array([[0.5, -2.0, 0.25]] * 5, np.float32).T
    nrm = sn.copy()
    nrm[:, 4] = -sn[:, 4]       # (the geometric normal points away from the light: the origin moves against it)
    o, w, maxt, tr2 = D.rays(L, p, nrm, sn, d, t)
    assert np.array_equal(tr, tr2) and (maxt[~tr] == -1).all() and not o[:, ~tr].any() and not w[:, ~tr].any()
    assert np.isinf(maxt[tr]).all() and np.array_equal(w[:, 0], l.astype(np.float32).astype(np.float64))
    mag = (1 + 2.0) * 1500 * 2.0 ** -24
    for i in (0, 4):
        assert np.abs(o[:, i] - (p[:, i] + mag * l.astype(np.float32))).max() <= 1e-7      # towards the light either way


def test_the_shares_of_the_rig_on_the_oracles_records_of_the_gpu_tests_scenes():
    lights = D.rig()
    for key, rec, r, t, field in D.oracle_scenes():
        shares, union = {}, np.zeros(len(t), bool)
        for name, L in zip(D.NAMES, lights):
            q = D.probe(L, rec, r, t, field)
            shares[name], union = q.shares, union | q.unsure
        print(key, "unsure union", union.mean(), {k: "%.3f %.3f" % (v["traced_of_eligible"], v["occluded_of_traced"])
                                                  for k, v in shares.items()})
        D.assert_shares(shares, float(union.mean()))

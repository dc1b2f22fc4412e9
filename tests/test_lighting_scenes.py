"""The scenes of tests/lighting_scenes.py on the CPU, with the oracle and the float64 restatements only:
  (a) the conditions that make each scene a test of the lighting kernels (tests/test_gpu_lighting_scenes.py): enough
      eligible samples, bounce rays that hit and that miss, every light both reaching and not reaching hits, no mask
      decided by rounding, coordinates small enough for the 1e-6 bound on spawned origins;
  (b) bounce_ref.face_normal under the scene's to_world and flip_normals against the oracle's geometric normal;
  (c) its VJP and JVP against central differences and against each other.
(a) is about the inputs, not the kernels: if a change to a helper moves a scene out of a range, retune the scene (the
lights' elevations), not the range."""
import numpy as np
import pytest

import bounce_ref as B
import lighting_scenes as LS


@pytest.fixture(scope="module", params=LS.NAMES)
def model(request, oracle):
    sc = LS.scene(request.param)
    return sc, LS.cpu_model(sc, oracle)


def test_scene_conditions(model):
    sc, m = model
    s = m.shares
    print(sc.name, {k: np.round(v, 4) for k, v in s.items()})
    assert sc.n == 2300 and sc.n % 64 and sc.n % 256 and LS.SPLIT % 4 == 0 and LS.SPLIT % 64 == 60
    assert sc.lights.shape == (sc.L, 4) and np.abs(np.linalg.norm(sc.lights[:, :3], axis=1) - 1.0).max() < 1e-6
    assert np.abs(np.linalg.norm(sc.rays[3:6], axis=0) - 1.0).max() < 1e-6 and np.all(np.isinf(sc.rays[6]))
    assert s["eligible"] > 0.5
    assert 0.2 <= s["bounce_hit"] <= 0.8
    assert 0.2 <= s["sky_unoccluded"] <= 0.8
    assert np.all((0.03 <= s["lit"]) & (s["lit"] <= 0.97)), s["lit"]
    assert np.all(s["lit_records"] >= 40), s["lit_records"]
    assert s["undecided"] <= 1e-3
    assert s["max_coordinate"] < 4
    if sc.L == 8:
        assert m.lit[:, 7].any()                                           # bit 7 of lit_bits is used


def test_face_normal_against_the_oracle(model):
    """2e-6 absolute: the oracle's n is a float32 unit vector computed in float32 from float32 world vertices.  On the
    first hits and on the hits of the bounce rays; the orientation under the mirror and the flip is the oracle's."""
    sc, m = model
    hit = np.isfinite(m.t)
    err = np.abs(LS.normals_of(sc, m.prim, hit) - m.n)[:, hit].max()
    errb = max(np.abs(m.nq[k] - m.nq_oracle[k])[:, m.hit[k]].max() for k in range(LS.K))
    print(sc.name, "max |n - oracle n|: first hits", err, "bounce hits", errb, "hits", int(hit.sum()), int(m.hit.sum()))
    assert hit.sum() > 1000 and m.hit.sum() > 1000
    assert err <= 2e-6 and errb <= 2e-6
    # the side the normal is on (up: the world image of object +z as a covector): a mirror turns the cross product of
    # the world edges over and flip_normals negates it, so the normal is up with neither or with both
    A = np.asarray(sc.to_world, np.float64)[:, :3]
    side = (m.n[:, hit] * (np.linalg.inv(A).T @ np.array([0.0, 0.0, 1.0]))[:, None]).sum(0)
    assert np.all(side > 0) if (np.linalg.det(A) < 0) == sc.flip else np.all(side < 0)


def test_face_normal_derivatives_against_central_differences(model):
    """step 1e-5 in float64, rtol 1e-6 per component: rounding is 1e-16 / 1e-5 and truncation (max_height step |dh| /
    edge)^2 / 6 < 1e-8 of the largest component, which is what a component near zero is allowed as its absolute part;
    the transpose identity to 1e-12 relative"""
    sc, m = model
    rng = np.random.default_rng(3)
    prim = np.unique(m.hit_prim[m.hit])[:200].astype(np.int64)             # triangles the bounce rays hit
    assert len(prim) >= 50
    args = (prim, sc.max_height)
    kw = dict(flip=sc.flip, to_world=sc.to_world)
    gn = rng.normal(size=(3, len(prim)))
    dh = rng.normal(size=sc.h64.shape)
    jvp = B.face_normal_jvp(sc.h64, *args, dh, **kw)
    vjp = B.face_normal_vjp(sc.h64, *args, gn, **kw)
    eps = 1e-5
    fd = (B.face_normal(sc.h64 + eps * dh, *args, **kw) - B.face_normal(sc.h64 - eps * dh, *args, **kw)) / (2 * eps)
    scale = np.abs(fd).max()
    assert scale > 0.1 and np.allclose(jvp, fd, rtol=1e-6, atol=1e-8 * scale), np.abs(jvp - fd).max()
    f = lambda h: (B.face_normal(h, *args, **kw) * gn).sum()
    vi, vj = B.prim_vertices(prim, sc.W)
    touched = np.zeros(sc.h64.shape, bool); touched[vi, vj] = True
    assert not vjp[~touched].any()
    gscale = np.abs(vjp).max()
    for i, j in zip(*np.nonzero(touched)):
        e = np.zeros_like(sc.h64); e[i, j] = eps
        g = (f(sc.h64 + e) - f(sc.h64 - e)) / (2 * eps)
        assert np.isclose(g, vjp[i, j], rtol=1e-6, atol=1e-8 * gscale), (i, j, g, vjp[i, j])
    lhs, rhs = (jvp * gn).sum(), (dh * vjp).sum()
    print(sc.name, "<jvp(dh), g>", lhs, "<dh, vjp(g)>", rhs)
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    # without the transform the scene's normals are other normals: the argument is used
    if not np.array_equal(sc.to_world, LS.IDENTITY):
        assert np.abs(B.face_normal(sc.h64, *args, flip=sc.flip) - B.face_normal(sc.h64, *args, **kw)).max() > 0.05

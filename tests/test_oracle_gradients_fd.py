"""Oracle surface interaction + adjoint vs float64 central finite differences (the reference's
methodology, src/integrators/tests/test_ad_integrators.py:1001-1012), all three modes, general
affine to_world, flipped normals, ray gradients.  CPU only."""
import numpy as np
import pytest

import common
import si_numpy as S


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("mode", ["default", "follow", "detach"])
def test_si_and_adjoint_vs_fd(oracle, mode, flip):
    rng = np.random.default_rng(3)
    W, H, s = 9, 7, 0.6
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
    tw = common.affine(4)
    f = oracle.OracleField(h, max_height=s, to_world=tw, flip_normals=flip)
    n = 24
    r = common.to_world_rays(common.random_rays(n, rng, s), tw)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    assert np.isfinite(t).sum() >= n // 2
    flags = S.RAY_ALL | {"default": 0, "follow": S.RAY_FOLLOWSHAPE, "detach": S.RAY_DETACHSHAPE}[mode]
    si = f.compute_surface_interaction(r, t, u, v, prim, flags)
    g = {nm: rng.normal(size=(c, n)).astype(np.float32) for nm, c in S.GRAD_FIELDS}
    gh, go, gd = f.adjoint(r, t, u, v, prim, g, flags, ray_grads=True)
    gh_fd = np.zeros((H, W))
    for k in np.where(np.isfinite(t))[0]:
        gk = {nm: (g[nm][:, k] if c > 1 else g[nm][0, k]) for nm, c in S.GRAD_FIELDS}
        ref = S.surface_interaction(h, s, tw, flip, r[0:3, k], r[3:6, k], prim[k], flags, (u[k], v[k]), h)
        for nm, _ in S.GRAD_FIELDS:   # forward values: 1e-5 relative
            assert np.allclose(si[nm][..., k], ref[nm], rtol=1e-5, atol=2e-6), (nm, k)
        for (i, j), val in S.fd_height_gradient(h, s, tw, flip, r[0:3, k], r[3:6, k], prim[k], flags, gk,
                                                (u[k], v[k])).items():
            gh_fd[i, j] += val
        fo, fdd = S.fd_ray_gradient(h, s, tw, flip, r[0:3, k], r[3:6, k], prim[k], flags, gk, (u[k], v[k]))
        assert np.allclose(go[:, k], fo, rtol=2e-4, atol=2e-4 * (1 + np.abs(fo).max()))
        assert np.allclose(gd[:, k], fdd, rtol=2e-4, atol=2e-4 * (1 + np.abs(fdd).max()))
    if mode == "detach":
        assert np.all(gh == 0)
    else:
        assert np.abs(gh - gh_fd).max() <= 1e-5 * np.abs(gh_fd).max()


def test_closed_form_dt_dh(oracle):
    """dt/dh_k = s * b_k * n_z / (n . d) in object space (to_world = I)."""
    rng = np.random.default_rng(8)
    h = rng.uniform(0.3, 0.6, (6, 6)).astype(np.float32)
    s = 0.8
    f = oracle.OracleField(h, max_height=s)
    r = common.random_rays(50, rng, s * 0.6)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    si = f.compute_surface_interaction(r, t, u, v, prim)
    for k in np.where(np.isfinite(t))[0][:20]:
        g = {"t": np.zeros((1, 50), np.float32)}; g["t"][0, k] = 1
        gh = f.adjoint(r, t, u, v, prim, g)
        ids = S.prim_vertex_ids(6, int(prim[k]))
        b = [1 - u[k] - v[k], u[k], v[k]]
        nd = float(si["n"][:, k] @ r[3:6, k])
        for (i, j), bk in zip(ids, b):
            assert abs(gh[i, j] - s * bk * si["n"][2, k] / nd) <= 1e-4 * (1 + abs(gh[i, j]))


# ---- every RayFlags set: the record's flag branches (mesh.cpp:672-903, interaction.h:257-267, 475-507) ----------------

def _mirror_shear():
    """a mirror (negative determinant) with shear: world-space normals point down (n.z < 0)"""
    S_ = np.array([[1.0, 0.35, 0.0], [0.0, 1.0, 0.25], [0.2, 0.0, 1.0]])
    return np.concatenate([np.diag([-1.0, 1.0, 1.0]) @ S_, np.array([[-0.1], [0.2], [0.1]])], 1).astype(np.float32)


TRANSFORMS = {"identity": np.eye(4)[:3].astype(np.float32), "affine": common.affine(4), "mirror_shear": _mirror_shear()}
MODE_BITS = {"default": 0, "follow": S.RAY_FOLLOWSHAPE, "detach": S.RAY_DETACHSHAPE}


def test_coordinate_system_known_answers():
    """vector.h:116-136 at the poles (dr::sign(0) = +1) and an orthonormal basis elsewhere"""
    s, t = S.coordinate_system(np.array([0.0, 0.0, 1.0]))
    assert np.array_equal(s, [1, 0, 0]) and np.array_equal(t, [0, 1, 0])
    s, t = S.coordinate_system(np.array([0.0, 0.0, -1.0]))
    assert np.array_equal(s, [1, 0, 0]) and np.array_equal(t, [0, -1, 0])
    s, t = S.coordinate_system(np.array([0.6, 0.0, 0.0]) / 0.6)        # n.z = 0 takes sign +1
    assert np.allclose(s, [0, 0, -1]) and np.allclose(t, [0, 1, 0])
    rng = np.random.default_rng(1)
    for n in rng.normal(size=(50, 3)):
        n /= np.linalg.norm(n)
        s, t = S.coordinate_system(n)
        B = np.stack([s, t, n])
        assert np.allclose(B @ B.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(B), 1.0)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("mode", list(MODE_BITS))
@pytest.mark.parametrize("xf", list(TRANSFORMS))
def test_every_flag_set_vs_fd(oracle, xf, mode, flip):
    """All 16 subsets of {UV, dPdUV, ShadingFrame, dNSdUV} (and Minimal), each with and without BoundaryTest: the
    oracle's record against the float64 restatement at 1e-5 (every row, sh_frame and wi included), its adjoint of the
    18 differentiable rows against central differences, heights and rays.  Without dPdUV, dp_du / dp_dv are
    coordinate_system of the face normal before flip_normals and carry its derivative (mesh.cpp:762).  Hits with
    |n.z| < 1e-2 stay out of the differences: the sign switch of coordinate_system is a real discontinuity."""
    rng = np.random.default_rng(17 + 3 * list(TRANSFORMS).index(xf) + flip)
    W, H, s = 9, 7, 0.6
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
    tw = TRANSFORMS[xf]
    f = oracle.OracleField(h, max_height=s, to_world=tw, flip_normals=flip)
    n = 16
    r = common.to_world_rays(common.random_rays(n, rng, s), tw)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    hits = np.where(np.isfinite(t))[0]
    assert len(hits) >= n // 2
    nz = []
    for sub in S.FLAG_SUBSETS + [S.RAY_MINIMAL]:
        flags = sub | MODE_BITS[mode]
        g = {nm: rng.normal(size=(c, n)).astype(np.float32) for nm, c in S.GRAD_FIELDS}
        si = f.compute_surface_interaction(r, t, u, v, prim, flags)
        si_bt = f.compute_surface_interaction(r, t, u, v, prim, flags | S.RAY_BOUNDARYTEST)
        for nm, _ in oracle.SI_FIELDS:      # BoundaryTest changes boundary_test alone
            if nm != "boundary_test":
                assert np.array_equal(si[nm], si_bt[nm]), (flags, nm)
        assert np.all(si["boundary_test"] == 0)
        assert np.all(si_bt["boundary_test"][hits] >= 0) and np.all(si_bt["boundary_test"][~np.isfinite(t)] == 1e8)
        gh, go, gd = f.adjoint(r, t, u, v, prim, g, flags, ray_grads=True)
        gh2, go2, gd2 = f.adjoint(r, t, u, v, prim, g, flags | S.RAY_BOUNDARYTEST, ray_grads=True)
        assert np.array_equal(go, go2) and np.array_equal(gd, gd2)   # (the heights' sums run in any thread order)
        assert np.allclose(gh, gh2, rtol=1e-6, atol=1e-6 * np.abs(gh).max())
        gh_fd = np.zeros((H, W))
        fd_ok = True
        for k in hits:
            gk = {nm: (g[nm][:, k] if c > 1 else g[nm][0, k]) for nm, c in S.GRAD_FIELDS}
            args = (h, s, tw, flip, r[0:3, k], r[3:6, k], prim[k], flags)
            ref = S.surface_interaction(*args, (u[k], v[k]), h)
            for nm, _ in S.GRAD_FIELDS + S.FRAME_FIELDS:
                assert np.allclose(si[nm][..., k], ref[nm], rtol=1e-5, atol=2e-6), (flags, nm, k, si[nm][..., k], ref[nm])
            if not flags & (S.RAY_UV | S.RAY_DPDUV):   # uv = prim_uv
                assert si["uv"][0, k] == u[k] and si["uv"][1, k] == v[k]
            if not flags & S.RAY_SHADINGFRAME:
                assert np.all(si["sh_s"][:, k] == 0) and np.all(si["sh_t"][:, k] == 0)
            nz.append(float(si["n"][2, k]) * (-1 if flip else 1))
            if abs(si["n"][2, k]) < 1e-2:
                fd_ok = False
                continue
            for (i, j), val in S.fd_height_gradient(*args, gk, (u[k], v[k])).items():
                gh_fd[i, j] += val
            fo, fdd = S.fd_ray_gradient(*args, gk, (u[k], v[k]))
            assert np.allclose(go[:, k], fo, rtol=2e-4, atol=2e-4 * (1 + np.abs(fo).max())), (flags, k, go[:, k], fo)
            assert np.allclose(gd[:, k], fdd, rtol=2e-4, atol=2e-4 * (1 + np.abs(fdd).max())), (flags, k, gd[:, k], fdd)
        if mode == "detach":
            assert np.all(gh == 0)
        elif fd_ok:
            assert np.abs(gh - gh_fd).max() <= 1e-5 * np.abs(gh_fd).max(), (flags, np.abs(gh - gh_fd).max())
    # both branches of coordinate_system run: world-space normals up (identity, affine) and down (the mirror)
    nz = np.array(nz)
    assert np.all(nz < 0) if xf == "mirror_shear" else np.all(nz > 0)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("xf", ["affine", "mirror_shear"])
def test_torch_restatement_every_flag_set(oracle, xf, flip):
    """tests/smooth_ref.surface and tests/xform_ref.si_block (the GPU tests' yardsticks) on flat shading: every row
    of every flag set equals the oracle at 1e-5, and their autograd the oracle's adjoint (checked above against
    central differences), heights and rays, in the three modes"""
    import torch
    import smooth_ref as R
    import xform_ref as X
    rng = np.random.default_rng(23 + flip)
    W, H, s = 9, 7, 0.6
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
    tw = TRANSFORMS[xf]
    f = oracle.OracleField(h, max_height=s, to_world=tw, flip_normals=flip)
    n = 64
    r = common.to_world_rays(common.random_rays(n, rng, s), tw)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    hit = np.isfinite(t)
    assert hit.sum() >= n // 3
    rh = torch.from_numpy(r[:, hit].astype(np.float64))
    pr = torch.from_numpy(prim[hit].astype(np.int64))
    bf = (torch.from_numpy(u[hit].astype(np.float64)), torch.from_numpy(v[hit].astype(np.float64)))
    for mode, mb in MODE_BITS.items():
        for sub in S.FLAG_SUBSETS:
            flags = sub | mb
            si = f.compute_surface_interaction(r, t, u, v, prim, flags)
            h64 = torch.from_numpy(h.astype(np.float64)).requires_grad_(True)
            o = rh[0:3].T.clone().requires_grad_(True); d = rh[3:6].T.clone().requires_grad_(True)
            blk = X.si_block(h64, s, tw, flip, o, d, pr, bf, mode, False, flags=flags, frame=True)
            want = np.concatenate([si[nm].reshape(-1, n)[:, hit] for nm, _ in oracle.SI_FIELDS if nm != "boundary_test"])
            assert np.allclose(blk.detach().numpy(), want, rtol=1e-5, atol=2e-6), (mode, flags)
            g = rng.normal(size=(18, n)).astype(np.float32)
            (blk[:18] * torch.from_numpy(g[:, hit].astype(np.float64))).sum().backward()
            gd = {nm: g[a:b] for (nm, _), a, b in zip(S.GRAD_FIELDS, [0, 1, 4, 7, 9, 12, 15], [1, 4, 7, 9, 12, 15, 18])}
            gh, go, gdd = f.adjoint(r, t, u, v, prim, gd, flags, ray_grads=True)
            ga = h64.grad.numpy() if h64.grad is not None else np.zeros_like(gh)
            assert np.abs(ga - gh).max() <= 2e-5 * (1 + np.abs(ga).max()), (mode, flags)
            assert np.allclose(o.grad.numpy().T, go[:, hit], rtol=1e-4, atol=1e-4 * (1 + np.abs(go).max())), (mode, flags)
            assert np.allclose(d.grad.numpy().T, gdd[:, hit], rtol=1e-4, atol=1e-4 * (1 + np.abs(gdd).max())), (mode, flags)

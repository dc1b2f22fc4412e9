"""Bounce lighting on the GPU (hf_bounce_rays, hf_bounce_lighting, _adjoint, _tangent) on the scene of
tests/test_gpu_sky_lighting.py: sine_heights(96), max_height 0.5, a 64 x 64 x 4 orthographic wavefront (16 384
samples), K = 4, seed 5, two directional lights.
  (a) the materialised bounce and shadow rays against the float64 restatement (tests/bounce_ref.py);
  (b) hit_prim against the two-call sequence hf_bounce_rays + hf_ray_intersect_preliminary, bit for bit;
  (c) lit_bits against hf_bounce_rays(to_light) + hf_ray_test, bit for bit;
  (d) both against the oracle on the materialised rays, exactly;
  (e) image, grad_sh_n, grad_weight and tangent against the restatement fed with the GPU's record;
  (f) grad_heights against the composition of existing pieces, and the chain through autograd;
  (g) repeatability and edge cases;  (h) nothing written beside the rows;  (i) graph capture;  (j) the inverse loop."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import bounce_ref as B
from lighting_scenes import _close, _records, _rows7
from row_helpers import GUARD, _np, base_scene, guarded, intact, rows, sub

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
K, SEED, MAXH = 4, 5, 0.5
LIGHTS = np.array([[0.3, 0.2, 0.9, 1.0], [-0.5, 0.4, 0.6, 0.7]])
LIGHTS[:, :3] /= np.linalg.norm(LIGHTS[:, :3], axis=1, keepdims=True)
LIGHTS = LIGHTS.astype(np.float32)
NL = len(LIGHTS)
# a mask is decided by the sign of a float32 quantity that is within 2e-6 of the restatement's: a lane whose margin is
# below this is decided by rounding and is left out of mask comparisons
MARGIN = 4e-6
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def scene(hf, oracle):
    sc = base_scene(hf, oracle, (64, 64, 4), (0.6, 0.35, 2.0))                 # (max_height 0.5 = MAXH)
    shape, ray, si, n = sc.shape, sc.ray, sc.si, sc.n
    sc.lights = torch.from_numpy(LIGHTS)
    sc.w, sc.z = B.directions(sc.np["sh_n"], np.arange(n), 32, SEED)     # [32, 3, n], [32, n]: every num_rays is a prefix
    sc.eligible, _ = B.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
    sc.traced = B.traced(sc.np["sh_n"], sc.np["d"], sc.np["t"], sc.z)
    # the two-call sequences, once for all tests: bounce rays, their closest hits and interactions, shadow rays, any hits
    sc.brays, sc.si2, sc.nq = {}, {}, {}

    def second(k):
        if k not in sc.brays:
            sc.brays[k] = hf.bounce_rays(shape, si, ray, k, seed=SEED)
            sc.si2[k] = shape.ray_intersect(sc.brays[k], hf.RayFlags.All)
            sc.nq[k] = _np(sc.si2[k].n).astype(np.float64)
        return sc.brays[k], sc.si2[k]
    sc.second = second
    sc.normals = lambda num: np.stack([second(k) and sc.nq[k] for k in range(num)])  # [num, 3, n] float64: si.n of the two-call sequence
    for k in range(K):
        second(k)
    sc.srays = [[hf.bounce_rays(shape, si, ray, k, seed=SEED, to_light=LIGHTS[l, :3]) for l in range(NL)] for k in range(K)]
    sc.shit = [[shape.ray_test(sc.srays[k][l]) for l in range(NL)] for k in range(K)]
    _, prim, lit = hf.bounce_lighting(shape, si, ray, sc.lights, spp=4, num_rays=K, seed=SEED, return_records=True)
    sc.prim, sc.lit = _np(prim).view(np.uint32), _np(lit)
    return sc


def test_materialised_rays_against_the_restatement(hf, scene):
    sc = scene
    print("eligible share", sc.eligible.mean())
    assert 0.1 < float(sc.eligible.mean()) <= 1.0
    for k in range(K):
        r = sc.brays[k]
        d, o, maxt = _np(r.d), _np(r.o), _np(r.maxt)
        assert np.abs(d - sc.w[k]).max() <= 2e-6, (k, np.abs(d - sc.w[k]).max())
        assert np.all((maxt == np.inf) | (maxt == -1.0))
        sure = (sc.z[k] > MARGIN) | ~sc.eligible                         # (a sample that is not eligible traces nothing: no rounding decides)
        assert sure.mean() > 0.999
        tr = maxt == np.inf
        assert np.array_equal(tr[sure], sc.traced[k][sure]), k
        ref_o = B.spawn_origin(sc.np["p"], sc.np["n"], sc.w[k])
        assert np.abs(o - ref_o)[:, tr].max() <= 1e-6, (k, np.abs(o - ref_o)[:, tr].max())
        assert tr.any() and (~tr).any()
        # the shadow rays from the two-call sequence's second vertex
        p2, n2 = _np(sc.si2[k].p).astype(np.float64), sc.nq[k]
        valid = _np(sc.si2[k].is_valid())
        cw = (n2 * d.astype(np.float64)).sum(0)
        front = valid & (-cw > 0)
        want, margin = B.shadow_traced(front[None], n2[None], LIGHTS)
        for l in range(NL):
            s = sc.srays[k][l]
            sd, so, smaxt = _np(s.d), _np(s.o), _np(s.maxt)
            assert np.abs(sd - LIGHTS[l, :3, None]).max() == 0
            assert np.all((smaxt == np.inf) | (smaxt == -1.0))
            sure = ~valid | ((np.abs(cw) > MARGIN) & (margin[0, l] > MARGIN))
            assert sure.mean() > 0.999
            st = smaxt == np.inf
            assert np.array_equal(st[sure], want[0, l][sure]), (k, l)
            ref_o = B.spawn_origin(p2, n2, np.broadcast_to(LIGHTS[l, :3, None].astype(np.float64), p2.shape))
            assert st.any() and np.abs(so - ref_o)[:, st].max() <= 1e-6, (k, l, np.abs(so - ref_o)[:, st].max())
    # a permuted ray_index: the samples follow the id
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(4)).to(device="cuda", dtype=torch.int32)
    r = hf.bounce_rays(sc.shape, sc.si, sc.ray, 2, seed=SEED, ray_index=ids)
    w, _ = B.directions(sc.np["sh_n"], _np(ids), 3, SEED)
    assert np.abs(_np(r.d) - w[2]).max() <= 2e-6
    assert np.abs(_np(r.d) - sc.w[2]).max() > 0.5                          # (and not the position)
    same = hf.bounce_rays(sc.shape, sc.si, sc.ray, 2, seed=SEED, ray_index=torch.arange(sc.n, dtype=torch.int32, device="cuda"))
    assert torch.equal(same.d, sc.brays[2].d) and torch.equal(same.o, sc.brays[2].o) and torch.equal(same.maxt, sc.brays[2].maxt)
    assert not torch.equal(hf.bounce_rays(sc.shape, sc.si, sc.ray, 2, seed=SEED + 1).d, sc.brays[2].d)


def test_hit_prim_equals_the_two_call_sequence(hf, scene):
    sc = scene
    for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
        old = sc.shape.ray_coherence()
        sc.shape.set_ray_coherence(mode)
        try:
            for k in range(K):
                pi = sc.shape.ray_intersect_preliminary(sc.brays[k])
                valid = _np(pi.is_valid())
                two = np.where(valid, _np(pi.prim_index).view(np.uint32), np.uint32(MISS))
                assert np.array_equal(sc.prim[k], two), (mode, k, int((sc.prim[k] != two).sum()))
        finally:
            sc.shape.set_ray_coherence(old)


def test_lit_bits_equal_the_two_call_sequence(hf, scene):
    sc = scene
    _, lit = B.unpack(sc.prim, sc.lit, 8)
    assert not lit[:, NL:].any()                                           # no bit at or above n_lights
    for k in range(K):
        for l in range(NL):
            two = _np((sc.srays[k][l].maxt >= 0) & ~sc.shit[k][l])
            assert np.array_equal(lit[k, l], two), (k, l, int((lit[k, l] != two).sum()))


def test_record_equals_the_oracles_exactly(hf, scene):
    sc = scene
    hit, lit = B.unpack(sc.prim, sc.lit, NL)
    n_hit = n_traced = 0
    n_lit, n_shadow = np.zeros(NL), np.zeros(NL)
    for k in range(K):
        tr = _np(sc.brays[k].maxt >= 0)
        t, _, _, prim = sc.field.ray_intersect_preliminary(_rows7(sc.brays[k])[:, tr])
        assert np.array_equal(hit[k][tr], np.isfinite(t)), (k, int((hit[k][tr] != np.isfinite(t)).sum()))
        assert np.array_equal(sc.prim[k][tr][np.isfinite(t)], prim[np.isfinite(t)]), k
        assert not hit[k][~tr].any()
        n_hit += int(hit[k].sum()); n_traced += int(tr.sum())
        d = _np(sc.brays[k].d).astype(np.float64)
        assert np.all((sc.nq[k] * d).sum(0)[hit[k]] < 0)                    # every hit is seen from the front
        for l in range(NL):
            st = _np(sc.srays[k][l].maxt >= 0)
            occluded = sc.field.ray_test(_rows7(sc.srays[k][l])[:, st]).astype(bool)
            assert np.array_equal(lit[k, l][st], ~occluded), (k, l, int((lit[k, l][st] != ~occluded).sum()))
            assert not lit[k, l][~st].any()
            n_lit[l] += int(lit[k, l].sum()); n_shadow[l] += int(st.sum())
    print("traced", n_traced, "hit share", n_hit / n_traced, "shadow rays", n_shadow, "lit share", n_lit / n_shadow,
          "z < 0.08 share", float((sc.z[:K][sc.traced[:K]] < 0.08).mean()))
    assert 0.05 < n_hit / n_traced < 0.95
    assert np.all((0.05 < n_lit / n_shadow) & (n_lit / n_shadow < 0.95))


@pytest.mark.parametrize("num_rays", [1, 4, 32])
@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("spp", [1, 4, 3])
def test_image_adjoint_and_tangent_against_the_restatement(hf, scene, spp, with_weight, num_rays):
    """Values are at most 1 by the sizes of the inputs, not by a run: a sample's value under one light is at most
    weight_max albedo (albedo/pi) E <= 1.5 * 0.7 * 0.7 / pi = 0.23."""
    sc = scene
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    rng = np.random.default_rng(100 * spp + num_rays)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32) if with_weight else None
    wt = torch.from_numpy(wgt).cuda().requires_grad_(True) if with_weight else None
    img, prim, lit = hf.bounce_lighting(sc.shape, si, ray, sc.lights, albedo=albedo, spp=spp, num_rays=num_rays, seed=SEED,
                                        weight=wt, return_records=True)
    assert img.shape == (NL, m // spp) and prim.shape == (num_rays, m) and lit.shape == (num_rays, m)
    if num_rays == K:
        assert np.array_equal(_np(prim).view(np.uint32), sc.prim[:, :m]) and np.array_equal(_np(lit), sc.lit[:, :m])
    hit, lt = B.unpack(_np(prim), _np(lit), NL)
    nq = sc.normals(num_rays)[:, :, :m]
    arrs = [sc.np[k][..., :m] for k in ("sh_n", "d", "t")]
    w, z = sc.w[:num_rays, :, :m], sc.z[:num_rays, :m]
    ref, _, absum = B.forward(*arrs, wgt, hit, lt, nq, LIGHTS, albedo, spp)
    print("image")
    assert ref.max() > 0.01 and ref.max() <= 1.0 and _close(_np(img), ref, absum, num_rays)
    gi = rng.normal(size=(NL, m // spp)).astype(np.float32)
    (img * torch.from_numpy(gi).cuda()).sum().backward()
    adj = B.adjoint(*arrs, wgt, hit, lt, nq, LIGHTS, albedo, spp, w, z, gi)
    el, _ = B.eligible(*arrs)
    got_n = _np(si.sh_frame.n.grad)
    print("grad_sh_n")
    assert np.abs(adj["grad_sh_n"]).max() > 0 and _close(got_n, adj["grad_sh_n"], adj["abs_sh_n"], num_rays)
    assert not got_n[:, ~el].any()                                      # exact zeros
    if with_weight:
        got_w = _np(wt.grad)
        print("grad_weight")
        assert _close(got_w, adj["grad_weight"], adj["abs_weight"], num_rays)
        assert not got_w[~el].any()
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32) if with_weight else None
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), torch.from_numpy(dn).cuda())
        wd = fwAD.make_dual(wt.detach(), torch.from_numpy(dw).cuda()) if with_weight else None
        out = hf.bounce_lighting(sc.shape, si, ray, sc.lights, albedo=albedo, spp=spp, num_rays=num_rays, seed=SEED, weight=wd)
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref, tabs = B.tangent(*arrs, wgt, hit, lt, nq, LIGHTS, albedo, spp, w, z, dn, dw)
    print("tangent")
    assert np.abs(tref).max() > 0 and _close(tan, tref, tabs, num_rays)


def _nq_route(shape_flat, prim, lit, gnq):
    """the composition of existing pieces: per direction, hf_sample_position_adjoint at the centroid of the hit
    triangle with grad_n = gN_k, into one accumulator"""
    acc = shape_flat._zero_heights()
    n = prim.shape[1]
    b = torch.full((2, n), 1.0 / 3.0, device="cuda")
    for k in range(prim.shape[0]):
        active = lit[k] != 0
        ps = types.SimpleNamespace(prim_index=torch.where(active, prim[k], torch.zeros_like(prim[k])).contiguous(), b=b)
        shape_flat.sample_position_adjoint(ps, grad_n=torch.from_numpy(gnq[k].astype(np.float32)).cuda(), active=active,
                                           grad_heightfield=acc)
    return _np(acc).astype(np.float64)


@pytest.mark.parametrize("face_normals", [True, False])
def test_grad_heights_against_the_composition(hf, scene, face_normals):
    """1e-5 relative L2: the bound of the sky row's chain test, where the order of float atomics is the only difference"""
    sc = scene
    albedo, spp = 0.8, 4
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=MAXH, face_normals=face_normals)
    flat = shape if face_normals else hf.Heightfield(heightfield=sc.h.clone(), max_height=MAXH)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, prim, lit = hf.bounce_lighting(shape, si, sc.ray, sc.lights, albedo=albedo, spp=spp, num_rays=K, seed=SEED,
                                        return_records=True)
    gi = np.random.default_rng(11).normal(size=tuple(img.shape)).astype(np.float32)
    (img * torch.from_numpy(gi).cuda()).sum().backward()
    got = _np(shape.heightfield.grad).astype(np.float64)
    # the restatement at this handle's own sh_n and record; n_q: the face normals of the recorded triangles
    sh_n, t = _np(si.sh_frame.n), _np(si.t)
    hit, lt = _records(prim, lit, NL)
    hnp = _np(sc.h).astype(np.float64)
    nq = np.stack([B.face_normal(hnp, np.where(hit[k], _np(prim[k]).view(np.uint32), 0), MAXH) for k in range(K)])
    w, z = B.directions(sh_n, np.arange(sc.n), K, SEED)
    adj = B.adjoint(sh_n, sc.np["d"], t, None, hit, lt, nq, LIGHTS, albedo, spp, w, z, gi)
    route_nq = _nq_route(flat, prim, lit, adj["grad_nq"])
    assert np.linalg.norm(route_nq) > 0
    # the C entry alone, heights only
    lib = hf._capi.lib()
    L = (hf._capi.hf_dir_light_t * NL)()
    for l in range(NL):
        L[l].to_light[0], L[l].to_light[1], L[l].to_light[2], L[l].irradiance = LIGHTS[l].tolist()
    sn, dd, tt = si.sh_frame.n.detach().contiguous(), sc.ray.d.contiguous(), si.t.detach().contiguous()
    gh = shape._zero_heights()
    git = torch.from_numpy(gi).cuda()
    hf._capi.check(lib.hf_bounce_lighting_adjoint(shape._h, sc.n, spp, rows(sn), rows(dd), tt.data_ptr(), None, K, SEED, None, NL, L,
                                                  albedo, prim.data_ptr(), lit.data_ptr(), sc.n, git.data_ptr(), None, None,
                                                  gh.data_ptr(), torch.cuda.current_stream().cuda_stream))
    err = np.linalg.norm(_np(gh) - route_nq) / np.linalg.norm(route_nq)
    print("face_normals", face_normals, "n_q route: relative L2 error", err, "norm", np.linalg.norm(route_nq))
    assert err <= 1e-5, err
    # through autograd: the sh_n route (shape.adjoint fed with the restatement's grad_sh_n) + the n_q route
    ybar = torch.zeros((18, sc.n), device="cuda"); ybar[9:12] = torch.from_numpy(adj["grad_sh_n"].astype(np.float32)).cuda()
    pi = shape.ray_intersect_preliminary(sc.ray)
    route_sh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All))).astype(np.float64)
    want = route_sh + route_nq
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("face_normals", face_normals, "chain: relative L2 error", err, "norms", np.linalg.norm(route_sh), np.linalg.norm(route_nq))
    assert np.linalg.norm(route_sh) > 0 and err <= 1e-5, err


def test_tangent_of_the_heights_is_the_transpose(hf, scene):
    """forward mode through shape.heightfield: <tangent(dh), gi> = <dh, adjoint(gi)> (n_q route; float32 sums)"""
    sc = scene
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=MAXH)
    si, ray = sub(hf, sc, 0, sc.n)
    gi = torch.from_numpy(np.random.default_rng(5).normal(size=(NL, sc.n // 4)).astype(np.float32)).cuda()
    dh = torch.from_numpy(np.random.default_rng(6).normal(size=(96, 96)).astype(np.float32)).cuda()
    shape.heightfield.requires_grad_(True)
    img = hf.bounce_lighting(shape, si, ray, sc.lights, spp=4, num_rays=K, seed=SEED)
    (img * gi).sum().backward()
    rhs = float((shape.heightfield.grad.double() * dh.double()).sum())
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(shape.heightfield.detach(), dh)
        tan = fwAD.unpack_dual(hf.bounce_lighting(shape, si, ray, sc.lights, spp=4, num_rays=K, seed=SEED)).tangent
    lhs = float((tan.double() * gi.double()).sum())
    print("heights: <tangent, gi>", lhs, "<dh, adjoint>", rhs)
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


def test_repeatable_and_edge_cases(hf, scene):
    sc = scene
    m = sc.n
    gi = torch.from_numpy(np.random.default_rng(1).normal(size=(NL, m // 4)).astype(np.float32)).cuda()
    dn = torch.from_numpy(np.random.default_rng(2).normal(size=(3, m)).astype(np.float32)).cuda()
    wt0 = torch.from_numpy(np.random.default_rng(3).uniform(0.5, 1.5, m).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        si, ray = sub(hf, sc, 0, m, requires_grad=True)
        wt = wt0.clone().requires_grad_(True)
        img, prim, lit = hf.bounce_lighting(sc.shape, si, ray, sc.lights, spp=4, num_rays=K, seed=SEED, weight=wt, return_records=True)
        (img * gi).sum().backward()
        with fwAD.dual_level():
            si2, _ = sub(hf, sc, 0, m)
            si2.sh_frame.n = fwAD.make_dual(si2.sh_frame.n, dn)
            tan = fwAD.unpack_dual(hf.bounce_lighting(sc.shape, si2, ray, sc.lights, spp=4, num_rays=K, seed=SEED, weight=wt0)).tangent
        runs.append((prim.clone(), lit.clone(), img.detach().clone(), si.sh_frame.n.grad.clone(), wt.grad.clone(), tan.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # n = 0 is legal
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, prim0, lit0 = hf.bounce_lighting(sc.shape, si0, ray0, sc.lights, spp=4, num_rays=K, return_records=True)
    assert img0.shape == (NL, 0) and prim0.shape == (K, 0) and lit0.shape == (K, 0)
    img0.sum().backward()
    assert len(hf.bounce_rays(sc.shape, si0, ray0, 0)) == 0
    lib = hf._capi.lib()
    one = torch.zeros(4, device="cuda")
    p3 = (hf._capi._fp * 3)(*([one.data_ptr()] * 3))
    L = (hf._capi.hf_dir_light_t * 1)()
    L[0].to_light[2] = 1.0; L[0].irradiance = 1.0
    assert lib.hf_bounce_lighting(sc.shape._h, 0, 1, p3, p3, p3, p3, one.data_ptr(), None, K, 0, None, 1, L, 1.0, one.data_ptr(),
                                  None, None, 0, None) == 0
    # a constant height field: no bounce ray hits anything
    flat = hf.Heightfield(heightfield=torch.full((96, 96), 0.5, device="cuda"), max_height=MAXH)
    sif = flat.ray_intersect(sc.ray, hf.RayFlags.All)
    assert bool(sif.is_valid().any())
    imgf, primf, litf = hf.bounce_lighting(flat, sif, sc.ray, sc.lights, spp=4, num_rays=K, seed=SEED, return_records=True)
    assert not bool(imgf.any()) and bool((primf == -1).all()) and not bool(litf.any())
    # a wavefront with no eligible sample: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, primm, litm = hf.bounce_lighting(sc.shape, sim, up, sc.lights, spp=4, num_rays=K, return_records=True)
    assert not bool(imgm.any()) and bool((primm == -1).all()) and not bool(litm.any())
    # ... and hits seen from behind
    imgb, primb, litb = hf.bounce_lighting(sc.shape, sc.si, up, sc.lights, spp=4, num_rays=K, return_records=True)
    assert not bool(imgb.any()) and bool((primb == -1).all()) and not bool(litb.any())
    with pytest.raises(hf.HfError):
        hf.bounce_lighting(sc.shape, sc.si, sc.ray, sc.lights, spp=3)       # n not a multiple of spp
    with pytest.raises(hf.HfError):
        hf.bounce_lighting(sc.shape, sc.si, sc.ray, sc.lights, num_rays=33)
    with pytest.raises(hf.HfError):
        hf.bounce_lighting(sc.shape, sc.si, sc.ray, torch.from_numpy(np.repeat(LIGHTS[:1], 9, 0)))   # nine lights
    tw = torch.eye(4)[:3].clone().requires_grad_(True)
    moving = hf.Heightfield(heightfield=sc.h.clone(), max_height=MAXH, to_world=tw, differentiable_to_world=True)
    with pytest.raises(hf.HfError):
        hf.bounce_lighting(moving, sc.si, sc.ray, sc.lights)                 # to_world is not differentiated by this row


def test_nothing_is_written_beside_the_rows(hf, scene):
    """n = 64 * 3 + 5, spp = 1, sample_stride = n + 7: three whole batches and a part of one; guard values around
    every output row and in the gaps of both record arrays"""
    sc = scene
    lib = hf._capi.lib()
    n, G, PAD = 64 * 3 + 5, 96, 7
    stride = n + PAD
    start = int(torch.nonzero(sc.si.is_valid())[0]) // 64 * 64          # a stretch of the wavefront with hits in it
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    assert bool(torch.isfinite(t).any())
    L = (hf._capi.hf_dir_light_t * NL)()
    for l in range(NL):
        L[l].to_light[0], L[l].to_light[1], L[l].to_light[2], L[l].irradiance = LIGHTS[l].tolist()
    image = torch.full((G + NL * n + G,), GUARD, device="cuda")          # the per-light rows are contiguous (npix = n)
    prim = torch.full((G + K * stride,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lit = torch.full((G + K * stride,), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.arange(start, start + n, dtype=torch.int32, device="cuda")

    def forward():
        hf._capi.check(lib.hf_bounce_lighting(sc.shape._h, n, 1, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, K, SEED,
                                              ids.data_ptr(), NL, L, 1.0, image.data_ptr() + 4 * G, prim.data_ptr() + 4 * G,
                                              lit.data_ptr() + G, stride, stream))
    forward()
    assert bool((image[:G] == GUARD).all()) and bool((image[G + NL * n:] == GUARD).all()) and bool((image[G:G + NL * n] != GUARD).all())
    pr, lb = prim[G:].view(K, stride), lit[G:].view(K, stride)
    assert bool((prim[:G] == 0x5A5A5A5A).all()) and bool((pr[:, n:] == 0x5A5A5A5A).all()) and bool((pr[:, :n] != 0x5A5A5A5A).all())
    assert bool((lit[:G] == 0x5A).all()) and bool((lb[:, n:] == 0x5A).all()) and bool((lb[:, :n] != 0x5A).all())
    # the slice, with its ids, is the slice of the whole
    assert np.array_equal(_np(pr[:, :n]).view(np.uint32), sc.prim[:, start:start + n]) and np.array_equal(_np(lb[:, :n]), sc.lit[:, start:start + n])
    gi = torch.ones(NL * n, device="cuda")
    gn, gp = guarded(n, G, 3)
    gw, gwp = guarded(n, G)
    gh = torch.zeros((96, 96), device="cuda")
    head = (sc.shape._h, n, 1, rows(sn), rows(d), t.data_ptr(), None, K, SEED, ids.data_ptr(), NL, L, 1.0, prim.data_ptr() + 4 * G,
            lit.data_ptr() + G, stride)
    hf._capi.check(lib.hf_bounce_lighting_adjoint(*head, gi.data_ptr(), gp, gwp[0], gh.data_ptr(), stream))
    assert intact(gn, n, G) and intact(gw, n, G) and bool(gh.any())
    dimg = torch.full((G + NL * n + G,), GUARD, device="cuda")
    hf._capi.check(lib.hf_bounce_lighting_tangent(*head, rows(sn), None, None, dimg.data_ptr() + 4 * G, stream))
    assert bool((dimg[:G] == GUARD).all()) and bool((dimg[G + NL * n:] == GUARD).all()) and bool((dimg[G:G + NL * n] != GUARD).all())
    for tl in (None, (C.c_float * 3)(*LIGHTS[0, :3].tolist())):
        ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
        hf._capi.check(lib.hf_bounce_rays(sc.shape._h, n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), 0, SEED, ids.data_ptr(),
                                          tl, rop, rdp, rmp[0], stream))
        assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    torch.cuda.synchronize()


def test_forward_and_adjoint_captured_and_replayed_equal_eager(hf, scene):
    """one forward + adjoint through the C ABI captured on a side stream (a linear capture) and replayed"""
    sc = scene
    lib = hf._capi.lib()
    n, spp = sc.n, 4
    dev = torch.device("cuda", 0)
    L = (hf._capi.hf_dir_light_t * NL)()
    for l in range(NL):
        L[l].to_light[0], L[l].to_light[1], L[l].to_light[2], L[l].irradiance = LIGHTS[l].tolist()
    p, nr, sn, d, t = (x.detach().contiguous() for x in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    gi = torch.from_numpy(np.random.default_rng(8).normal(size=NL * (n // spp)).astype(np.float32)).cuda()
    out = dict(image=torch.empty(NL * (n // spp), device=dev), prim=torch.empty((K, n), dtype=torch.int32, device=dev),
               lit=torch.empty((K, n), dtype=torch.uint8, device=dev), gn=torch.empty((3, n), device=dev))

    def step(stream):
        hf._capi.check(lib.hf_bounce_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, K, SEED,
                                              None, NL, L, 1.0, out["image"].data_ptr(), out["prim"].data_ptr(),
                                              out["lit"].data_ptr(), n, stream))
        hf._capi.check(lib.hf_bounce_lighting_adjoint(sc.shape._h, n, spp, rows(sn), rows(d), t.data_ptr(), None, K, SEED, None, NL, L,
                                                      1.0, out["prim"].data_ptr(), out["lit"].data_ptr(), n, gi.data_ptr(),
                                                      rows(out["gn"]), None, None, stream))

    def clear():
        for v in out.values():
            v.zero_()
        torch.cuda.synchronize()
    clear()
    step(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    assert np.array_equal(_np(eager["prim"]).view(np.uint32), sc.prim) and bool(eager["gn"].any())
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        step(s.cuda_stream)                         # warm-up on a side stream, as torch asks before a capture
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream(dev).cuda_stream)
    clear()                                         # what the capture did to the buffers is undone; the replay does the work
    g.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(v, eager[k]), k


def test_inverse_loop_with_a_bounce_term_descends(hf):
    import inverse_heights
    hist, err, wall = inverse_heights.run(grid=64, film=64, spp=4, steps=15, lr=0.02, verbose=False, bounce=2)
    assert hist[-1] < hist[0] and math.isfinite(hist[-1])

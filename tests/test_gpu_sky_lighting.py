"""Sky lighting on the GPU (hf_sky_rays, hf_sky_lighting, _adjoint, _tangent) on the scene of
test_shadowed_lighting_matches_oracle_visibility: sine_heights(96), max_height 0.5, a 64 x 64 x 4 orthographic
wavefront, K = 8 (131 072 shadow rays).
  (a) the materialised rays against the float64 restatement (tests/sky_ref.py);
  (b) the fused kernel's visibility word against the two-call sequence hf_sky_rays + hf_ray_test, bit for bit;
  (c) the same word against the oracle's ray_test on those rays, exactly;
  (d) image, adjoint and tangent against the restatement fed with the GPU's bits;
  (e) the chain image -> backward -> dL/dheight against the oracle's chain;
  (f) repeatability, empty and all-miss wavefronts, nothing written beside the rows;
  (g) the inverse loop with a sky term descends."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import sky_ref as S
from row_helpers import base_scene, guarded, intact, rows, sub

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
K, SEED = 8, 5
# a direction is traced when the float32 <sh_n, w_k> is positive, and the kernel's float32 direction is within 2e-6 of
# the restatement's: a lane whose |<sh_n, w_k>| is below this is decided by rounding and is left out of mask comparisons
MARGIN = 4e-6


@pytest.fixture(scope="module")
def scene(hf, oracle):
    sc = base_scene(hf, oracle, (64, 64, 4), (0.6, 0.35, 2.0))
    shape, ray, si, n = sc.shape, sc.ray, sc.si, sc.n
    sc.w = S.directions(np.arange(n), 32, SEED)                          # [32, 3, n]: every num_rays is a prefix
    sc.eligible, _ = S.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
    sc.traced, sc.margin = S.traced(sc.np["sh_n"], sc.np["d"], sc.np["t"], sc.w)
    # the two-call sequence: materialised rays and their any-hit answers, once for all tests
    sc.sky_rays = [hf.sky_rays(si, ray, k, seed=SEED) for k in range(K)]
    sc.occluded = [shape.ray_test(r) for r in sc.sky_rays]
    _, vis = hf.sky_lighting(shape, si, ray, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    sc.words = vis.cpu().numpy().view(np.uint32)
    return sc


def test_materialised_rays_against_the_restatement(hf, scene):
    sc = scene
    assert 0.1 < float(np.isfinite(sc.np["t"]).mean()) <= 1.0
    for k in range(K):
        r = sc.sky_rays[k]
        d, o, maxt = r.d.cpu().numpy(), r.o.cpu().numpy(), r.maxt.cpu().numpy()
        assert np.abs(d - sc.w[k]).max() <= 2e-6, (k, np.abs(d - sc.w[k]).max())
        assert np.all((maxt == np.inf) | (maxt == -1.0))
        sure = (sc.margin[k] > MARGIN) | ~sc.eligible                   # (a sample that is not eligible traces nothing: no rounding decides)
        assert sure.mean() > 0.999
        assert np.array_equal((maxt == np.inf)[sure], sc.traced[k][sure]), k
        tr = (maxt == np.inf)
        ref_o = S.spawn_origin(sc.np["p"], sc.np["n"], sc.w[k])
        assert np.abs(o - ref_o)[:, tr].max() <= 1e-6, (k, np.abs(o - ref_o)[:, tr].max())
        assert tr.any() and (~tr).any()
    # a permuted ray_id: the samples follow the id
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(4)).to(device="cuda", dtype=torch.int32)
    r = hf.sky_rays(sc.si, sc.ray, 2, seed=SEED, ray_index=ids)
    w = S.directions(ids.cpu().numpy(), 3, SEED)[2]
    assert np.abs(r.d.cpu().numpy() - w).max() <= 2e-6
    assert np.abs(r.d.cpu().numpy() - sc.w[2]).max() > 0.5          # (and not the position)
    same = hf.sky_rays(sc.si, sc.ray, 2, seed=SEED, ray_index=torch.arange(sc.n, dtype=torch.int32, device="cuda"))
    assert torch.equal(same.d, sc.sky_rays[2].d) and torch.equal(same.o, sc.sky_rays[2].o) and torch.equal(same.maxt, sc.sky_rays[2].maxt)
    assert not torch.equal(hf.sky_rays(sc.si, sc.ray, 2, seed=SEED + 1).d, sc.sky_rays[2].d)


def test_fused_equals_the_two_call_sequence_bitwise(hf, scene):
    sc = scene
    bits = S.unpack(sc.words, 32)
    assert not bits[K:].any()                                          # no bit beyond num_rays
    for k in range(K):
        two = (sc.sky_rays[k].maxt >= 0) & ~sc.occluded[k]
        assert np.array_equal(bits[k], two.cpu().numpy()), (k, int((bits[k] != two.cpu().numpy()).sum()))
    # a permuted ray_id against the same sequence
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(6)).to(device="cuda", dtype=torch.int32)
    _, vis = hf.sky_lighting(sc.shape, sc.si, sc.ray, spp=4, num_rays=2, seed=SEED, ray_index=ids, return_visibility=True)
    b = S.unpack(vis.cpu().numpy(), 2)
    for k in range(2):
        r = hf.sky_rays(sc.si, sc.ray, k, seed=SEED, ray_index=ids)
        assert np.array_equal(b[k], ((r.maxt >= 0) & ~sc.shape.ray_test(r)).cpu().numpy()), k


def test_visibility_equals_the_oracles_exactly(hf, scene):
    sc = scene
    bits = S.unpack(sc.words, K)
    seen = traced = 0
    for k in range(K):
        r = sc.sky_rays[k]
        tr = (r.maxt >= 0).cpu().numpy()
        rows = torch.cat([r.o, r.d, r.maxt[None]]).cpu().numpy()
        occluded = sc.field.ray_test(rows[:, tr]).astype(bool)
        assert np.array_equal(bits[k][tr], ~occluded), (k, int((bits[k][tr] != ~occluded).sum()))
        assert not bits[k][~tr].any()
        seen += int(bits[k].sum()); traced += int(tr.sum())
    share = seen / traced
    print("visible share of the traced directions", share, "traced", traced)
    assert 0.05 < share < 0.95, share                                   # both outcomes occur


@pytest.mark.parametrize("num_rays", [1, 8, 32])
@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("spp", [1, 4, 3])
def test_image_adjoint_and_tangent_against_the_restatement(hf, scene, spp, with_weight, num_rays):
    """rtol 1e-5, atol 1e-7 (tests/test_direct_lighting.py).  1e-7 is an ulp of 1, and a pixel of the tangent image is a
    float32 sum of spp SIGNED float32 sample tangents: where they cancel, half an ulp of each sample (6e-8 |v|) is what is
    left, so the bound can hold only for |v| <= 1, as the lighting tests' values are.  The inputs are sized by that
    rule, not by a run: a sample's value is at most 4 albedo L weight_max (every cosine 1), set to 1 by the radiance, and
    its tangent at most 4 albedo L (weight_max |dsh_n| + |dweight|) <= sqrt(3) 0.25 + 0.5 / 1.5 = 0.77."""
    sc = scene
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    L = 1.0 / (4.0 * albedo * wmax)
    rng = np.random.default_rng(100 * spp + num_rays)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32) if with_weight else None
    wt = torch.from_numpy(wgt).cuda().requires_grad_(True) if with_weight else None
    img, vis = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=num_rays, seed=SEED,
                               weight=wt, return_visibility=True)
    assert img.shape == (m // spp,) and vis.shape == (m,)
    bits = S.unpack(vis.cpu().numpy(), num_rays)
    if num_rays == K:
        assert np.array_equal(vis.cpu().numpy().view(np.uint32), sc.words[:m])
    arrs = [sc.np[k][..., :m] for k in ("sh_n", "d", "t")]
    w = sc.w[:num_rays, :, :m]
    ref, _ = S.forward(*arrs, wgt, bits, w, L, albedo, spp)
    got = img.detach().cpu().numpy()
    print("image: max", ref.max(), "err", np.abs(got - ref).max())
    assert ref.max() > 0.05 and np.allclose(got, ref, rtol=1e-5, atol=1e-7), np.abs(got - ref).max()
    gi = rng.normal(size=m // spp).astype(np.float32)
    (img * torch.from_numpy(gi).cuda()).sum().backward()
    gn, gw = S.adjoint(*arrs, wgt, bits, w, L, albedo, spp, gi)
    got_n = si.sh_frame.n.grad.cpu().numpy()
    print("grad_sh_n: max", np.abs(gn).max(), "err", np.abs(got_n - gn).max())
    assert np.abs(gn).max() > 0 and np.allclose(got_n, gn, rtol=1e-5, atol=1e-7), np.abs(got_n - gn).max()
    el, _ = S.eligible(*arrs)
    assert not got_n[:, ~el].any()                                      # exact zeros
    if with_weight:
        got_w = wt.grad.cpu().numpy()
        print("grad_weight: err", np.abs(got_w - gw).max())
        assert np.allclose(got_w, gw, rtol=1e-5, atol=1e-7), np.abs(got_w - gw).max()
        assert not got_w[~el].any()
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32) if with_weight else None
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), torch.from_numpy(dn).cuda())
        wd = fwAD.make_dual(wt.detach(), torch.from_numpy(dw).cuda()) if with_weight else None
        out = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=num_rays, seed=SEED, weight=wd)
        tan = fwAD.unpack_dual(out).tangent.cpu().numpy()
    tref = S.tangent(*arrs, wgt, bits, w, L, albedo, spp, dn, dw)
    print("tangent: max", np.abs(tref).max(), "err", np.abs(tan - tref).max())
    assert np.abs(tref).max() > 0 and np.allclose(tan, tref, rtol=1e-5, atol=1e-7), np.abs(tan - tref).max()


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, scene, face_normals):
    """image -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n (fed with the GPU's bits) carried
    to the heights by the oracle's adjoint.  The oracle shades flat; with face_normals=False the restatement's grad_sh_n
    (at the shape's own smooth sh_n) goes through hf_adjoint, which tests/test_gpu_smooth_shading.py holds against float64."""
    sc = scene
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.sky_lighting(shape, si, sc.ray, radiance=1.3, albedo=0.8, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    gi = np.random.default_rng(11).normal(size=tuple(img.shape)).astype(np.float32)
    (img * torch.from_numpy(gi).cuda()).sum().backward()
    got = shape.heightfield.grad.cpu().numpy()
    bits = S.unpack(vis.cpu().numpy(), K)
    r = sc.rays.cpu().numpy()
    if face_normals:
        assert np.array_equal(vis.cpu().numpy().view(np.uint32), sc.words)
        t, u, v, prim = sc.field.ray_intersect_preliminary(r)
        rec = sc.field.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)
        gn, _ = S.adjoint(rec["sh_n"], r[3:6], rec["t"], None, bits, sc.w[:K], 1.3, 0.8, 4, gi)
        gh = sc.field.adjoint(r, t, u, v, prim, {"sh_n": gn.astype(np.float32)}, oracle.RAY_ALL)
    else:
        gn, _ = S.adjoint(si.sh_frame.n.detach().cpu().numpy(), r[3:6], si.t.detach().cpu().numpy(), None, bits, sc.w[:K],
                          1.3, 0.8, 4, gi)
        ybar = torch.zeros((18, sc.n), device="cuda"); ybar[9:12] = torch.from_numpy(gn.astype(np.float32)).cuda()
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)).cpu().numpy()
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= 1e-5, err


def test_repeatable_and_edge_cases(hf, scene):
    sc = scene
    m = sc.n
    gi = torch.from_numpy(np.random.default_rng(1).normal(size=m // 4).astype(np.float32)).cuda()
    dn = torch.from_numpy(np.random.default_rng(2).normal(size=(3, m)).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        si, ray = sub(hf, sc, 0, m, requires_grad=True)
        img, vis = hf.sky_lighting(sc.shape, si, ray, spp=4, num_rays=K, seed=SEED, return_visibility=True)
        (img * gi).sum().backward()
        with fwAD.dual_level():
            si2, _ = sub(hf, sc, 0, m)
            si2.sh_frame.n = fwAD.make_dual(si2.sh_frame.n, dn)
            tan = fwAD.unpack_dual(hf.sky_lighting(sc.shape, si2, ray, spp=4, num_rays=K, seed=SEED)).tangent
        runs.append((vis.clone(), si.sh_frame.n.grad.clone(), tan.clone(), img.detach().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # n = 0 is legal
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, vis0 = hf.sky_lighting(sc.shape, si0, ray0, spp=4, num_rays=K, return_visibility=True)
    assert img0.shape == (0,) and vis0.shape == (0,)
    img0.sum().backward()
    assert len(hf.sky_rays(si0, ray0, 0)) == 0
    lib = hf._capi.lib()
    one = torch.zeros(4, device="cuda")
    p3 = (hf._capi._fp * 3)(*([one.data_ptr()] * 3))
    assert lib.hf_sky_lighting(sc.shape._h, 0, 1, p3, p3, p3, p3, one.data_ptr(), None, K, 0, None, 1.0, 1.0, one.data_ptr(),
                               None, None) == 0
    # a wavefront with no eligible sample: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, vism = hf.sky_lighting(sc.shape, sim, up, spp=4, num_rays=K, return_visibility=True)
    assert not bool(imgm.any()) and not bool(vism.any())
    # ... and hits seen from behind
    back = hf.Ray3f(sc.ray.o, -sc.ray.d)
    imgb, visb = hf.sky_lighting(sc.shape, sc.si, back, spp=4, num_rays=K, return_visibility=True)
    assert not bool(imgb.any()) and not bool(visb.any())
    with pytest.raises(hf.HfError):
        hf.sky_lighting(sc.shape, sc.si, sc.ray, spp=3)                  # n not a multiple of spp
    with pytest.raises(hf.HfError):
        hf.sky_lighting(sc.shape, sc.si, sc.ray, num_rays=33)


def test_nothing_is_written_beside_the_rows(hf, scene):
    """n = 64 * 3 + 5, spp = 1: three whole batches and a part of one; guard values around every output row"""
    sc = scene
    lib = hf._capi.lib()
    n, G = 64 * 3 + 5, 96
    start = int(torch.nonzero(sc.si.is_valid())[0]) // 64 * 64          # a stretch of the wavefront with hits in it
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    assert bool(torch.isfinite(t).any())
    image, ip = guarded(n, G)
    vis = torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hf._capi.check(lib.hf_sky_lighting(sc.shape._h, n, 1, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, K, SEED, None,
                                       1.0, 1.0, ip[0], vis.data_ptr() + 4 * G, stream))
    assert intact(image, n, G)
    assert bool((vis[:G] == 0x5A5A5A5A).all()) and bool((vis[G + n:] == 0x5A5A5A5A).all())
    ids = torch.arange(start, start + n, dtype=torch.int32, device="cuda")
    _, whole = hf.sky_lighting(sc.shape, *sub(hf, sc, 0, sc.n), spp=1, num_rays=K, seed=SEED, return_visibility=True)
    hf._capi.check(lib.hf_sky_lighting(sc.shape._h, n, 1, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, K, SEED,
                                       ids.data_ptr(), 1.0, 1.0, ip[0], vis.data_ptr() + 4 * G, stream))
    assert torch.equal(vis[G:G + n], whole[start:start + n])             # the slice, with its ids, is the slice of the whole
    words = vis[G:G + n].contiguous()
    gi = torch.ones(n, device="cuda")
    gn, gp = guarded(n, G, 3)
    gw, gwp = guarded(n, G)
    hf._capi.check(lib.hf_sky_lighting_adjoint(n, 1, rows(sn), rows(d), t.data_ptr(), None, K, SEED, ids.data_ptr(), 1.0, 1.0,
                                               words.data_ptr(), gi.data_ptr(), gp, gwp[0], stream))
    assert intact(gn, n, G) and intact(gw, n, G)
    dimg, dp = guarded(n, G)
    hf._capi.check(lib.hf_sky_lighting_tangent(n, 1, rows(sn), rows(d), t.data_ptr(), None, K, SEED, ids.data_ptr(), 1.0, 1.0,
                                               words.data_ptr(), rows(sn), None, dp[0], stream))
    assert intact(dimg, n, G)
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    hf._capi.check(lib.hf_sky_rays(n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), 0, SEED, ids.data_ptr(), rop, rdp,
                                   rmp[0], stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    torch.cuda.synchronize()


def test_inverse_loop_with_a_sky_term_descends(hf):
    import inverse_heights
    hist, err, wall = inverse_heights.run(grid=64, film=64, spp=4, steps=15, lr=0.02, verbose=False, sky=1.0)
    assert hist[-1] < hist[0] and math.isfinite(hist[-1])

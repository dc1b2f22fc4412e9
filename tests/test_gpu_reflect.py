"""Specular reflection of the environment map on the GPU (hf_reflect_rays, hf_reflect_lighting, _adjoint, _tangent;
reflection_lighting, reflection_rays) on the scene of the sibling rows' tests: sine_heights(96), max_height 0.5, a
64 x 64 x 4 orthographic wavefront (16 384 samples) from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0), both face_normals
modes, eta 0 and 1.5, the maps map_sun(17, 9) and map_gradient(9, 5), the identity and one other rotation, weights in
[0.5, 1.5].
  (a) the materialised rays against the float64 restatement (tests/reflect_ref.py): masks on the sure lanes, origin,
      direction, maxt;
  (b) the fused kernel's visibility byte against the two-call sequence hf_reflect_rays + hf_ray_test, bit for bit, and
      against the oracle's ray_test on those rays, exactly;
  (c) eta = 0, no weight: value = Envmap.eval(rays.d) bit for bit on visible lanes, exactly 0 elsewhere; eta = 1.5 with a
      weight: value and image against the restatement fed with the GPU's visibility;
  (d) adjoint and tangent against the restatement, and transposition on the device;
  (e) the chain reflection_lighting -> loss -> backward -> dL/dheight against the restatement's chain and the oracle's adjoint;
  (f) repeatability, n = 0, an all-miss wavefront, n = spp * odd, guard bands, optional outputs, a captured graph;
  (g) forward_ad and backward agree through reflection_lighting;
  (h) examples/inverse_reflection.py descends; a flat field seen straight down shows F * env(up).

Tolerances (scripts/reflect_f32_error.py computes them on the CPU, profiles/reflect/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records,
weights in [0.5, 1.5] and standard normal upstream gradients and tangents, by at most the figures of F32 below (value
and image absolute, every derivative as the L2 norm of the difference over the L2 norm of the float64 result).  The GPU
is allowed four times that: another operation order and fused multiply-adds.  Left out of the derivative comparison:
lanes whose lookup is within 1e-4 of a cell border in fx or fy (the direction derivative jumps there) and lanes at the
poles; at most 2e-3 of the samples (2.5e-4 on the oracle's records)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import envmap_ref as E
import reflect_ref as R
from row_helpers import (GUARD, UNSURE_CAP, _cu, _fold, _np, _rel, base_scene, envmap, guarded, intact, leaf_si, rows,
                         transposition_gap)

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
ETAS = (0.0, 1.5)
SPP = 4
ROT2 = E.DEFAULT_ROT @ np.array([[np.cos(0.7), 0.0, np.sin(0.7)], [0.0, 1.0, 0.0], [-np.sin(0.7), 0.0, np.cos(0.7)]])
ROTS = {"identity": np.eye(3), "rotated": ROT2}
MAPS = {"sun": (17, 9), "gradient": (9, 5)}
F32 = {"value": 5.6e-5, "image": 3.1e-5, "grad_sh_n": 2.3e-4, "grad_weight": 6.5e-7, "grad_data": 9.8e-7, "dimage": 6.2e-5,
       "dvalue": 6.8e-5}
TOL = {k: 4 * v for k, v in F32.items()}
# a mask is decided by the sign of a float32 quantity (c, <g, wi>, <g, wr>): a lane on which one of them is below this in
# magnitude is decided by rounding and is left out of mask comparisons
MARGIN = 1e-5
BORDER, LEFT_OUT_CAP = 1e-4, 2e-3


def _envmap(hf, name, rname, requires_grad=False):
    return envmap(hf, MAPS, ROTS, name, rname, requires_grad)


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """the wavefront from origin `oi` on the shape in the given shading mode, its records as numpy, the reflected rays,
    the two-call answer and the restatement's rays: once for all tests"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), ORIGINS[oi], face_normals)
        sc.p = sc.np["p"]
        sc.a = tuple(sc.np[k] for k in ("n", "sh_n", "d", "t"))                      # the restatement's first four arguments
        sc.rr = hf.reflection_rays(sc.si, sc.ray)
        sc.occluded = sc.shape.ray_test(sc.rr)
        env, _, _ = _envmap(hf, "gradient", "identity")
        _, sc.vis = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, spp=SPP, return_visibility=True)
        sc.visn = _np(sc.vis).astype(bool)
        sc.traced, sc.o, sc.wr, sc.maxt, sc.v = R.rays(sc.p, *sc.a)
        sc.sure = (sc.v.margin > MARGIN) | ~sc.hit
        _SCENES[key] = sc
    return _SCENES[key]


@pytest.mark.parametrize("face_normals", [True, False])
def test_materialised_rays_against_the_restatement(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        assert 0.1 < float(sc.hit.mean()) < 1.0
        o, d, maxt = _np(sc.rr.o), _np(sc.rr.d), _np(sc.rr.maxt)
        tr = maxt >= 0
        unsure = float((~sc.sure).mean())
        print(ORIGINS[oi], "face" if face_normals else "smooth", "traced", int(tr.sum()), "inconsistent",
              int((sc.v.eligible & ~sc.v.consistent).sum()), "unsure", int((~sc.sure).sum()))
        assert unsure <= UNSURE_CAP, unsure
        assert np.array_equal(tr[sc.sure], sc.traced[sc.sure])
        assert np.all(maxt[tr] == np.inf) and np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
        both = tr & sc.traced
        assert both.sum() > 1000
        assert np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max() <= 1e-5
        assert np.abs(d - sc.wr)[:, both].max() <= 1e-6, np.abs(d - sc.wr)[:, both].max()      # a few float32 roundings of a unit vector
        assert np.abs(o - sc.o)[:, both].max() <= 1e-6, np.abs(o - sc.o)[:, both].max()
    # the `active` row: an inactive lane is not traced, the others are unchanged
    sc = _scene(hf, oracle, 0, True)
    act = torch.arange(sc.n, device="cuda") % 3 != 0
    ra = hf.reflection_rays(sc.si, sc.ray, active=act)
    assert bool((ra.maxt[~act] == -1.0).all()) and torch.equal(ra.maxt[act], sc.rr.maxt[act]) and torch.equal(ra.d[:, act], sc.rr.d[:, act])
    env, _, _ = _envmap(hf, "sun", "rotated")
    img, val, vis = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, spp=SPP, active=act, return_value=True, return_visibility=True)
    assert not bool(vis[~act].any()) and torch.equal(vis[act], sc.vis[act]) and not bool(val[~act].any())


@pytest.mark.parametrize("face_normals", [True, False])
def test_fused_equals_the_two_call_sequence_and_the_oracle(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        tr = sc.rr.maxt >= 0
        two = tr & ~sc.occluded
        assert torch.equal(sc.vis.bool(), two), int((sc.vis.bool() != two).sum())                     # bitwise
        rows = _np(torch.cat([sc.rr.o, sc.rr.d, sc.rr.maxt[None]]))
        trn = _np(tr)
        occluded = sc.field.ray_test(rows[:, trn]).astype(bool)
        assert np.array_equal(sc.visn[trn], ~occluded), int((sc.visn[trn] == occluded).sum())
        assert not sc.visn[~trn].any()
        lit, occ = int(sc.visn.sum()), int(occluded.sum())
        print(ORIGINS[oi], "face" if face_normals else "smooth", "traced", int(trn.sum()), "occluded", occ, "visible", lit)
        assert lit >= 0.01 * sc.n and occ >= 0.01 * sc.n                                              # both outcomes occur


@pytest.mark.parametrize("face_normals", [True, False])
def test_mirror_value_is_the_emitters_eval_bit_for_bit(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        for name in MAPS:
            for rname in ROTS:
                env, full, rot = _envmap(hf, name, rname)
                img, val, vis = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, eta=0.0, spp=SPP, return_value=True,
                                                       return_visibility=True)
                assert torch.equal(vis, sc.vis)
                lit = vis.bool()
                want = env.eval(sc.rr.d)
                assert torch.equal(val[lit], want[lit]) and not bool(val[~lit].any())
                assert float(val[lit].max()) > 0
                # the film: the tree's sum of the four samples of a pixel, once rounded per addition
                assert float((img - val.reshape(-1, SPP).double().mean(1)).abs().max()) <= 2.5e-7 * float(val.max())   # (at most four roundings of 2^-24)


def _inputs(n, shape):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    gi, gv = rng.normal(size=n // SPP).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dn, dw = rng.normal(size=(3, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dd = rng.normal(size=shape).astype(np.float32)
    return w, gi, gv, dn, dw, dd


@pytest.mark.parametrize("face_normals", [True, False])
@pytest.mark.parametrize("eta", ETAS)
def test_values_adjoint_and_tangent_against_the_restatement(hf, oracle, eta, face_normals):
    worst = {k: 0.0 for k in TOL}
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        for name in MAPS:
            for rname in ROTS:
                env, full, rot = _envmap(hf, name, rname, requires_grad=True)
                w, gi, gv, dn, dw, dd = _inputs(sc.n, full.shape)
                smooth = R.smooth_lanes(sc.v.wr, full.shape[1], full.shape[0], rot, BORDER)
                keep = sc.sure & (sc.visn == (sc.traced & sc.visn)) & smooth        # (a lane the GPU traced and the restatement did not is not sure)
                left_out = float((sc.visn & ~keep).mean())
                assert left_out <= LEFT_OUT_CAP, left_out
                dn = dn * keep
                args = (*sc.a, None, w, eta, full, rot, sc.visn, SPP)
                si = leaf_si(hf, sc)
                wt = _cu(w).requires_grad_(True)
                img, val, vis = hf.reflection_lighting(sc.shape, si, sc.ray, env, eta=eta, spp=SPP, weight=wt, return_value=True,
                                                       return_visibility=True)
                assert torch.equal(vis, sc.vis)
                ri, rv = R.forward(*args)
                assert not _np(val)[~sc.visn].any()
                err = {"value": np.abs(_np(val) - rv)[keep | ~sc.visn].max(), "image": np.abs(_np(img) - ri).max()}
                assert sc.visn[keep].sum() > 1000 and rv.max() > 0.01
                ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
                gm, gw, gd = R.adjoint(*args, gi, gv)
                got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_weight": _np(wt.grad), "grad_data": _np(env.data.grad)}
                assert not got["grad_sh_n"][:, ~sc.visn].any() and not got["grad_weight"][~sc.visn].any()   # exact zeros where vis = 0
                err["grad_sh_n"] = _rel(got["grad_sh_n"][:, keep], gm[:, keep])
                err["grad_weight"] = _rel(got["grad_weight"][keep], gw[keep])
                err["grad_data"] = _rel(got["grad_data"], _fold(gd))
                with fwAD.dual_level():
                    sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(dn.astype(np.float32))))
                    envd = hf.Envmap(fwAD.make_dual(env.data.detach(), _cu(dd[:, :-1])), to_world=rot)
                    # (the seam column's tangent is column 0's, as Envmap.full() copies it)
                    ti, tv = hf.reflection_lighting(sc.shape, sd, sc.ray, envd, eta=eta, spp=SPP, weight=fwAD.make_dual(_cu(w), _cu(dw)),
                                                    return_value=True)
                    timg, tval = fwAD.unpack_dual(ti).tangent, fwAD.unpack_dual(tv).tangent
                ddf = np.concatenate([dd[:, :-1], dd[:, :1]], 1)
                dimg, dval = R.tangent(*args, dn, dw, ddf)
                assert not _np(tval)[~sc.visn].any()
                err["dimage"], err["dvalue"] = _rel(_np(timg), dimg), _rel(_np(tval)[keep], dval[keep])
                # transposition on the device: <J u, v> = <u, J^T v>, both sides float32 results added up in float64; each
                # side is within its tolerance of the exact bilinear form, so they agree to the sum of the two
                gap = transposition_gap(((_np(timg), gi), (_np(tval), gv)),
                                        ((got["grad_sh_n"], dn), (got["grad_weight"], dw), (got["grad_data"], dd[:, :-1])))
                size = np.linalg.norm(dimg) * np.linalg.norm(gi) + np.linalg.norm(dval) * np.linalg.norm(gv)
                print(ORIGINS[oi], name, rname, {k: "%.3g" % v for k, v in err.items()}, "left out", left_out, "transposition",
                      gap / size)
                assert gap <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size, gap
                for k in err:
                    worst[k] = max(worst[k], err[k])
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """reflection_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's chain: the
    restatement's grad_sh_n (fed with the GPU's records and visibility) carried to the heights by the oracle's adjoint
    (flat shading) or by hf_adjoint, which tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).
    Bound: four times the float32 error of grad_sh_n + the 1e-5 of the sky row's chain to the heights, as the caustic
    row's chain test has it."""
    sc0 = _scene(hf, oracle, 0, face_normals)
    env, full, rot = _envmap(hf, "gradient", "rotated")
    shape = hf.Heightfield(heightfield=sc0.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc0.ray, hf.RayFlags.All)
    img, vis = hf.reflection_lighting(shape, si, sc0.ray, env, eta=1.5, spp=SPP, return_visibility=True)
    assert torch.equal(vis, sc0.vis) and float(img.detach().sum()) > 0
    gi = np.random.default_rng(11).normal(size=sc0.n // SPP).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(x) for x in (si.n, si.sh_frame.n, sc0.ray.d, si.t))
    gm, _, _ = R.adjoint(*a, None, None, 1.5, full, rot, sc0.visn, SPP, gi, None)
    r = _np(sc0.rays)
    if face_normals:
        t, u, v, prim = sc0.field.ray_intersect_preliminary(r)
        gh = sc0.field.adjoint(r, t, u, v, prim, {"sh_n": gm.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc0.n), device="cuda")
        ybar[9:12] = _cu(gm.astype(np.float32))
        pi = shape.ray_intersect_preliminary(sc0.ray)
        gh = _np(shape.adjoint(sc0.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= TOL["grad_sh_n"] + 1e-5, err


def test_repeatable_and_edge_cases(hf, oracle):
    sc = _scene(hf, oracle, 0, False)
    env, full, rot = _envmap(hf, "sun", "rotated")
    w, gi, gv, dn, dw, dd = (_cu(x) for x in _inputs(sc.n, full.shape))
    runs = []
    for _ in range(2):
        si = leaf_si(hf, sc)
        wt = w.clone().requires_grad_(True)
        img, val, vis = hf.reflection_lighting(sc.shape, si, sc.ray, env, eta=1.5, spp=SPP, weight=wt, return_value=True,
                                               return_visibility=True)
        ((img * gi).sum() + (val * gv).sum()).backward()
        runs.append((img.detach(), val.detach(), vis, si.sh_frame.n.grad, wt.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # n = 0 is legal
    e = hf.SurfaceInteraction3f()
    e.p, e.n, e.t = (x.detach()[..., :0].contiguous() for x in (sc.si.p, sc.si.n, sc.si.t))
    e.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach()[:, :0].contiguous().requires_grad_(True))
    ray0 = hf.Ray3f(sc.ray.o[:, :0].contiguous(), sc.ray.d[:, :0].contiguous())
    img0, val0, vis0 = hf.reflection_lighting(sc.shape, e, ray0, env, return_value=True, return_visibility=True)
    assert img0.shape == (0,) and val0.shape == (0,) and vis0.shape == (0,)
    (img0.sum() + val0.sum()).backward()
    assert len(hf.reflection_rays(e, ray0)) == 0
    # an all-miss wavefront: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, valm, vism = hf.reflection_lighting(sc.shape, sim, up, env, spp=SPP, return_value=True, return_visibility=True)
    assert not bool(vism.any()) and not bool(valm.any()) and not bool(imgm.any())
    assert bool((hf.reflection_rays(sim, up).maxt == -1.0).all())
    with pytest.raises(hf.HfError):
        hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, eta=-1.0)
    with pytest.raises(hf.HfError):
        hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, spp=3)            # 16 384 is no multiple of 3


@pytest.mark.parametrize("spp", [1, 3, 4])
def test_odd_sizes_guard_bands_and_optional_outputs(hf, oracle, spp):
    """n = spp * 151 (for spp = 4: two whole workgroups, one whole batch and a part of one); guard values around every
    output row; the slice equals the slice of the whole wavefront; every optional output NULL in turn"""
    sc = _scene(hf, oracle, 0, True)
    lib = hf._capi.lib()
    env, full, rot = _envmap(hf, "sun", "rotated")
    dat = _cu(full.astype(np.float32))
    H, W = full.shape
    rotc = env._rot
    eta = 1.5
    _, whole_val, _ = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, eta=eta, spp=1, return_value=True, return_visibility=True)
    n, G = spp * 151, 96
    npix = n // spp
    start = int(torch.nonzero(sc.vis)[0]) // 64 * 64
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    stream = torch.cuda.current_stream().cuda_stream
    mid = (None, None, eta, W, H, dat.data_ptr(), C.byref(rotc))
    fwd = lambda image, value, vis: hf._capi.check(lib.hf_reflect_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d),
                                                                           t.data_ptr(), *mid, image, value, vis, stream))
    img, ip = guarded(npix, G); val, vp = guarded(n, G)
    vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    fwd(ip[0], vp[0], vis.data_ptr() + G)
    assert intact(img, npix, G) and intact(val, n, G)
    assert bool((vis[:G] == 0x5A).all()) and bool((vis[G + n:] == 0x5A).all())
    assert torch.equal(vis[G:G + n], sc.vis[start:start + n]) and torch.equal(val[0, G:G + n], whole_val[start:start + n])
    assert 0 < int(vis[G:G + n].sum()) < n
    want = val[0, G:G + n].reshape(npix, spp).double().mean(1)
    assert float((img[0, G:G + npix] - want).abs().max()) <= 2.5e-7 * float(want.abs().max())
    # (the film: one product and at most three additions per pixel, each rounded to 2^-24 of the largest value: 2.5e-7)
    # every optional output NULL in turn: the others are unchanged
    for skip in range(3):
        img2, ip2 = guarded(npix, G); val2, vp2 = guarded(n, G)
        vis2 = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        fwd(None if skip == 0 else ip2[0], None if skip == 1 else vp2[0], None if skip == 2 else vis2.data_ptr() + G)
        if skip != 0:
            assert intact(img2, npix, G) and float((img2 - img).abs().max()) <= 2.5e-7 * float(want.abs().max())
        else:
            assert bool((img2 == GUARD).all())
        assert torch.equal(val2, val) if skip != 1 else bool((val2 == GUARD).all())
        assert torch.equal(vis2, vis) if skip != 2 else bool((vis2 == 0x5A).all())
    bytes_ = vis[G:G + n].contiguous()
    ones, onesp = torch.ones((3, n), device="cuda"), torch.ones(npix, device="cuda")
    head = (n, spp, rows(sn), rows(d), t.data_ptr(), *mid, bytes_.data_ptr())
    gn, gnp = guarded(n, G, 3); gw, gwp = guarded(n, G)
    gd = torch.full((H * W + 2 * G,), 0.0, device="cuda"); gd[:G] = GUARD; gd[G + H * W:] = GUARD
    hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, onesp.data_ptr(), ones.data_ptr(), gnp, gwp[0], gd.data_ptr() + 4 * G, stream))
    assert intact(gn, n, G) and intact(gw, n, G) and bool((gd[:G] == GUARD).all()) and bool((gd[G + H * W:] == GUARD).all())
    assert float(gd[G:G + H * W].abs().sum()) > 0
    # each adjoint output NULL in turn, and each upstream NULL
    gn2, gnp2 = guarded(n, G, 3); gw2, gwp2 = guarded(n, G)
    hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, onesp.data_ptr(), ones.data_ptr(), None, gwp2[0], None, stream))
    hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, onesp.data_ptr(), ones.data_ptr(), gnp2, None, None, stream))
    assert torch.equal(gn2, gn) and torch.equal(gw2, gw)
    ga, gap = guarded(n, G, 3); gb, gbp = guarded(n, G, 3)
    hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, onesp.data_ptr(), None, gap, None, None, stream))
    hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, None, ones.data_ptr(), gbp, None, None, stream))
    scale = float(gn[:, G:G + n].abs().max())
    assert float((ga + gb - gn)[:, G:G + n].abs().max()) <= 1e-6 * scale
    dimg, dip = guarded(npix, G); dval, dvp = guarded(n, G)
    ddat = torch.ones((H, W), device="cuda")
    tail = (rows(ones), ones.data_ptr(), ddat.data_ptr())
    hf._capi.check(lib.hf_reflect_lighting_tangent(*head, *tail, dip[0], dvp[0], stream))
    assert intact(dimg, npix, G) and intact(dval, n, G)
    wantd = dval[0, G:G + n].reshape(npix, spp).double().mean(1)
    assert float((dimg[0, G:G + npix] - wantd).abs().max()) <= 2.5e-7 * float(dval[0, G:G + n].abs().max())
    dimg2, dip2 = guarded(npix, G); dval2, dvp2 = guarded(n, G)
    hf._capi.check(lib.hf_reflect_lighting_tangent(*head, *tail, dip2[0], None, stream))
    hf._capi.check(lib.hf_reflect_lighting_tangent(*head, *tail, None, dvp2[0], stream))
    assert torch.equal(dimg2, dimg) and torch.equal(dval2, dval)
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    hf._capi.check(lib.hf_reflect_rays(n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, rop, rdp, rmp[0], stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    assert torch.equal(rm[0, G:G + n], sc.rr.maxt[start:start + n])
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    lib = hf._capi.lib()
    env, full, rot = _envmap(hf, "gradient", "rotated")
    dat = _cu(full.astype(np.float32))
    H, W = full.shape
    p, nr, sn, d, t = (x.detach().contiguous() for x in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    img = torch.zeros(sc.n // SPP, device="cuda"); value = torch.zeros(sc.n, device="cuda")
    vis = torch.zeros(sc.n, dtype=torch.uint8, device="cuda")
    gn = torch.zeros((3, sc.n), device="cuda"); timg = torch.zeros(sc.n // SPP, device="cuda")
    gi, ones = torch.ones(sc.n // SPP, device="cuda"), torch.ones((3, sc.n), device="cuda")
    mid = (None, None, 1.5, W, H, dat.data_ptr(), C.byref(env._rot))

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        hf._capi.check(lib.hf_reflect_lighting(sc.shape._h, sc.n, SPP, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), *mid,
                                               img.data_ptr(), value.data_ptr(), vis.data_ptr(), s))
        head = (sc.n, SPP, rows(sn), rows(d), t.data_ptr(), *mid, vis.data_ptr())
        hf._capi.check(lib.hf_reflect_lighting_adjoint(*head, gi.data_ptr(), None, rows(gn), None, None, s))
        hf._capi.check(lib.hf_reflect_lighting_tangent(*head, rows(ones), None, None, timg.data_ptr(), None, s))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    outs = (img, value, vis, gn, timg)
    first = [x.clone() for x in outs]
    assert torch.equal(vis, sc.vis) and float(img.sum()) > 0 and float(gn.abs().sum()) > 0 and float(timg.abs().sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for x in outs:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def test_forward_and_reverse_mode_agree(hf, oracle):
    """<J u, v> = <u, J^T v> for J = reflection_lighting with respect to (sh_n, weight, data), jvp on one side and
    backward on the other, through the public function; the bound is that of the kernels' own transposition check"""
    sc = _scene(hf, oracle, 0, False)
    env, full, rot = _envmap(hf, "sun", "identity", requires_grad=True)
    w, gi, gv, dn, dw, dd = (_cu(x) for x in _inputs(sc.n, full.shape))
    si = leaf_si(hf, sc)
    wt = w.clone().requires_grad_(True)
    img, val = hf.reflection_lighting(sc.shape, si, sc.ray, env, eta=1.5, spp=SPP, weight=wt, return_value=True)
    ((img * gi).sum() + (val * gv).sum()).backward()
    rhs = sum(float((g.double() * t.double()).sum()) for g, t in ((si.sh_frame.n.grad, dn), (wt.grad, dw), (env.data.grad, dd[:, :-1])))
    with fwAD.dual_level():
        sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), dn))
        envd = hf.Envmap(fwAD.make_dual(env.data.detach(), dd[:, :-1].contiguous()), to_world=rot)
        ti, tv = hf.reflection_lighting(sc.shape, sd, sc.ray, envd, eta=1.5, spp=SPP, weight=fwAD.make_dual(w, dw), return_value=True)
        timg, tval = fwAD.unpack_dual(ti).tangent, fwAD.unpack_dual(tv).tangent
    lhs = float((timg.double() * gi.double()).sum() + (tval.double() * gv.double()).sum())
    size = float(timg.double().norm() * gi.double().norm() + tval.double().norm() * gv.double().norm())
    print("lhs", lhs, "rhs", rhs, "relative to |J u| |v|", abs(lhs - rhs) / size)
    assert abs(lhs) > 0 and abs(lhs - rhs) <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size


@pytest.mark.parametrize("eta,F", [(0.0, 1.0), (1.5, 0.04)])
def test_flat_field_seen_straight_down_shows_the_zenith(hf, eta, F):
    """a flat field, an orthographic view straight down: every sample reflects straight up, sees the map's +Y (world +Z
    under the default rotation: row 0, which is constant) and the image is F * env(up)"""
    shape = hf.Heightfield(heightfield=torch.full((16, 16), 0.5, device="cuda"), max_height=0.5)
    xs = (torch.arange(24, device="cuda", dtype=torch.float32) + 0.5) / 24 * 1.6 - 0.8
    py, px = torch.meshgrid(xs, xs, indexing="ij")
    o = torch.stack([px.reshape(-1), py.reshape(-1), torch.full((px.numel(),), 1.0, device="cuda")]).contiguous()
    d = torch.zeros_like(o); d[2] = -1.0
    ray = hf.Ray3f(o, d)
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid().all())
    full = E.map_sun()
    env = hf.Envmap(_cu(full[:, :-1].astype(np.float32)))
    img, val, vis = hf.reflection_lighting(shape, si, ray, env, eta=eta, spp=4, return_value=True, return_visibility=True)
    assert bool(vis.all()) and img.shape == (144,)
    rr = hf.reflection_rays(si, ray)
    assert float((rr.d - torch.tensor([[0.0], [0.0], [1.0]], device="cuda")).abs().max()) <= 1e-6
    want = F * float(full[0, 0])
    # the lookup's acos is ill-conditioned at the pole: a mirror direction whose z is a few float32 roundings below 1
    # (within 2^-21: the normalised normal, c, 2 c and the fused multiply-add) is theta = sqrt(2 * 2^-21) = 9.8e-4 off the
    # zenith, which moves the lookup by theta (H - 1) / pi rows towards row 1
    theta = math.sqrt(2.0 * 2.0 ** -21)
    tol = F * theta * (full.shape[0] - 1) / math.pi * abs(float(full[1, 0]) - float(full[0, 0])) + 1e-6
    print("largest difference", float((val - want).abs().max()), "bound", tol)
    assert float((val - want).abs().max()) <= tol and float((img - want).abs().max()) <= tol


def test_inverse_reflection_example_descends(hf):
    import inverse_reflection
    hist = inverse_reflection.main(["--size", "32", "--steps", "30", "--quiet"])
    print("loss", hist[0], "->", hist[-1])
    assert math.isfinite(hist[-1]) and hist[-1] < hist[0]

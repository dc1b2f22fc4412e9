"""Glossy reflection of the environment map on the GPU (hf_glossy_rays, hf_glossy_lighting, _adjoint, _tangent;
glossy_lighting, glossy_rays) on the scenes of tests/glossy_ref.py: sine_heights(96), max_height 0.5, a 25 x 23 x 4
orthographic wavefront (2300 samples: nine workgroups, the last one partial) from (1.2, 0.3, 1.2) and from
(0.6, 0.35, 2.0), both face_normals modes, eta 0 and 1.5, and the seven (num_rays, alpha, map, rotation) combinations
COMBOS: num_rays 1, 3 and 32 (bit 31 of the word), alpha 0.05 and 0.3 as constant rows and one random row in
[0.05, 0.6], the maps map_sun(17, 9) and map_gradient(9, 5), the identity and one other rotation; weights in [0.5, 1.5].
  (a) the materialised rays and microfacet normals against the float64 restatement (tests/glossy_ref.py);
  (b) every bit of the fused kernel's visibility word against the two-call sequence hf_glossy_rays + hf_ray_test, bit
      for bit, and against the oracle's ray_test on those rays, exactly;
  (c) value, image, adjoint and tangent against the restatement fed with the GPU's bits, and transposition on the device;
  (d) forward_ad and backward agree through glossy_lighting;
  (e) the chain glossy_lighting -> loss -> backward -> dL/dheight against the restatement's chain and the oracle's adjoint;
  (f) repeatability, n = 0, an all-miss wavefront, n = spp * 151, guard bands, optional pointers, a captured graph;
  (g) known answers: a flat field under a constant map shows mean_k G1(c_o); alpha = 1e-4 shows hf_reflect_lighting's image;
  (h) examples/inverse_roughness.py descends in the loss and in |alpha - alpha_true|.

Tolerances (scripts/glossy_f32_error.py computes them on the CPU, profiles/glossy/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records,
weights in [0.5, 1.5] and standard normal upstream gradients and tangents (0.1 standard normal for alpha), by at most
the figures of F32 below (value and image absolute, every derivative and the ray directions as the L2 norm of the
difference over the L2 norm of the float64 result).  The GPU is allowed four times that: another operation order and
fused multiply-adds.  Left out of every comparison: samples with a direction within 1e-5 of a mask decision (c_i,
<g, wi>, <wi, h>, c_o, <g, wo>; the denominator of the draw's norm within 1e-4); at most 1e-3 of the samples.  No
sample is left out for a lookup near a cell border: the direction is held, no derivative of this row jumps there."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import glossy_ref as G
import reflect_ref as R
from row_helpers import (GUARD, UNSURE_CAP, _cu, _fold, _np, _rel, base_scene, envmap, guarded, intact, leaf_si, rows,
                         transposition_gap)

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SPP, SEED = G.SPP, G.SEED
ETAS = (0.0, 1.5)
# the maxima of profiles/glossy/f32_error.json, rounded up to two digits
F32 = {"value": 8.7e-4, "image": 2.2e-4, "grad_sh_n": 3.1e-5, "grad_weight": 1.5e-5, "grad_alpha": 9.2e-5, "grad_data": 1.3e-5,
       "dimage": 3.1e-5, "dvalue": 3.0e-5, "ray_d": 4.2e-6, "ray_h": 2.1e-6}
TOL = {k: 4 * v for k, v in F32.items()}
MARGIN = 1e-5


def _envmap(hf, name, rname, requires_grad=False):
    return envmap(hf, G.MAP_SIZES, G.ROTS, name, rname, requires_grad)


_SCENES, _DRAWS = {}, {}


def _scene(hf, oracle, oi, face_normals):
    """the wavefront from origin `oi` on the shape in the given shading mode and its records as numpy: once for all tests"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, G.FILM, G.ORIGINS[oi], face_normals)
        sc.key = key
        sc.p = sc.np["p"]
        sc.a = tuple(sc.np[k] for k in ("n", "sh_n", "d", "t"))                      # the restatement's first four arguments
        _SCENES[key] = sc
    return _SCENES[key]


def _draws(hf, sc, akind):
    """for one roughness row: the 32 materialised rays, their any-hit answers, the fused word at num_rays = 32 (every
    smaller num_rays is a prefix of it) and the restatement's rays and margins: once for all tests"""
    key = sc.key + (akind,)
    if key not in _DRAWS:
        dw = types.SimpleNamespace(alpha=G.alpha_row(akind, sc.n))
        dw.alpha_t = _cu(dw.alpha)
        dw.rr, dw.hh = zip(*[hf.glossy_rays(sc.si, sc.ray, dw.alpha_t, k, seed=SEED, return_normal=True) for k in range(32)])
        dw.occluded = [sc.shape.ray_test(r) for r in dw.rr]
        env, _, _ = _envmap(hf, "gradient", "identity")
        _, dw.words = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, dw.alpha_t, spp=SPP, num_rays=32, seed=SEED, return_visibility=True)
        dw.bits = G.unpack(_np(dw.words), 32)
        ref = [G.rays(sc.p, *sc.a, dw.alpha, k, SEED) for k in range(32)]
        dw.traced, dw.o, dw.wo, dw.maxt, dw.h, dw.margin, _ = (np.stack(x) for x in zip(*[r[:6] + (0,) for r in ref]))
        _DRAWS[key] = dw
    return _DRAWS[key]


def _sure(sc, dw, K):
    """samples none of whose first K directions is within MARGIN of a mask decision"""
    return (dw.margin[:K].min(0) > MARGIN) | ~sc.hit


@pytest.mark.parametrize("face_normals", [True, False])
def test_materialised_rays_against_the_restatement(hf, oracle, face_normals):
    worst = {"ray_d": 0.0, "ray_h": 0.0}
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        assert 0.1 < float(sc.hit.mean()) < 1.0
        for akind in (0.05, 0.3, "row"):
            dw = _draws(hf, sc, akind)
            assert float((~_sure(sc, dw, 32)).mean()) <= UNSURE_CAP
            num = {"ray_d": [0.0, 0.0], "ray_h": [0.0, 0.0]}
            for k in range(32):
                o, d, maxt, h = _np(dw.rr[k].o), _np(dw.rr[k].d), _np(dw.rr[k].maxt), _np(dw.hh[k])
                tr = maxt >= 0
                sure = (dw.margin[k] > MARGIN) | ~sc.hit
                for i in np.nonzero((tr != dw.traced[k]) & sure)[0]:
                    print("mask differs: origin", oi, "alpha", akind, "k", k, "lane", i, "margin %.3g" % dw.margin[k][i], "c_i %.9g" % -(sc.a[1][:, i] * sc.a[2][:, i]).sum())
                assert np.array_equal(tr[sure], dw.traced[k][sure])
                assert np.all(maxt[tr] == np.inf) and np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
                assert not h[:, ~sc.hit].any()
                both = tr & dw.traced[k] & sure
                assert np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max() <= 1e-5
                assert np.abs(o - dw.o[k])[:, both].max() <= 1e-6           # p moved along g: the direction enters by its side only
                for key, got, ref in (("ray_d", d, dw.wo[k]), ("ray_h", h, dw.h[k])):
                    num[key][0] += ((got - ref)[:, both] ** 2).sum(); num[key][1] += (ref[:, both] ** 2).sum()
            for key in num:
                assert num[key][1] > 1000
                worst[key] = max(worst[key], math.sqrt(num[key][0] / num[key][1]))
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])
    # the `active` row and ray_index: an inactive lane is not traced, the others are unchanged; ids move the stream
    sc = _scene(hf, oracle, 0, True)
    dw = _draws(hf, sc, 0.3)
    act = torch.arange(sc.n, device="cuda") % 3 != 0
    ra = hf.glossy_rays(sc.si, sc.ray, 0.3, 2, seed=SEED, active=act)
    assert bool((ra.maxt[~act] == -1.0).all()) and torch.equal(ra.maxt[act], dw.rr[2].maxt[act]) and torch.equal(ra.d[:, act], dw.rr[2].d[:, act])
    ids = torch.arange(sc.n, device="cuda", dtype=torch.int32).flip(0).contiguous()
    rb = hf.glossy_rays(sc.si, sc.ray, 0.3, 2, seed=SEED, ray_index=ids)
    assert not torch.equal(rb.d, dw.rr[2].d)
    rc = hf.glossy_rays(sc.si, sc.ray, 0.3, 2, seed=SEED, ray_index=torch.arange(sc.n, device="cuda", dtype=torch.int32))
    assert torch.equal(rc.d, dw.rr[2].d)


@pytest.mark.parametrize("face_normals", [True, False])
def test_fused_equals_the_two_call_sequence_and_the_oracle(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        for akind in (0.05, 0.3, "row"):
            dw = _draws(hf, sc, akind)
            lit = occ = 0
            for k in range(32):
                tr = dw.rr[k].maxt >= 0
                two = tr & ~dw.occluded[k]
                fused = ((dw.words >> k) & 1).bool()
                assert torch.equal(fused, two), (k, int((fused != two).sum()))                          # bitwise
                rows = _np(torch.cat([dw.rr[k].o, dw.rr[k].d, dw.rr[k].maxt[None]]))
                trn = _np(tr)
                occluded = sc.field.ray_test(rows[:, trn]).astype(bool)
                assert np.array_equal(dw.bits[k][trn], ~occluded) and not dw.bits[k][~trn].any()
                lit += int(dw.bits[k].sum()); occ += int(occluded.sum())
            print(G.ORIGINS[oi], "face" if face_normals else "smooth", "alpha", akind, "visible", lit, "occluded", occ)
            assert lit >= 0.01 * 32 * sc.n and occ >= 0.01 * 32 * sc.n                                  # both outcomes occur
            # a smaller num_rays is a prefix of the word
            env, _, _ = _envmap(hf, "sun", "rotated")
            _, w3 = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, dw.alpha_t, spp=SPP, num_rays=3, seed=SEED, return_visibility=True)
            assert torch.equal(w3, dw.words & 7)


@pytest.mark.parametrize("face_normals", [True, False])
@pytest.mark.parametrize("eta", ETAS)
def test_values_adjoint_and_tangent_against_the_restatement(hf, oracle, eta, face_normals):
    worst = {k: 0.0 for k in TOL if not k.startswith("ray")}
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        for K, akind, name, rname in G.COMBOS:
            dw = _draws(hf, sc, akind)
            env, full, rot = _envmap(hf, name, rname, requires_grad=True)
            w, gi, gv, dn, dwt, da, dd = G.test_inputs(sc.n, full.shape)
            bits = dw.bits[:K]
            keep = _sure(sc, dw, K) & ~(bits & ~dw.traced[:K]).any(0)      # (a direction the GPU traced and the restatement did not is not sure)
            assert float((~keep).mean()) <= UNSURE_CAP
            kp = keep.reshape(-1, SPP).all(1)
            dn, dwt, da, gv, gi = dn * keep, dwt * keep, da * keep, gv * keep, gi * kp
            args = (*sc.a, None, w, dw.alpha, eta, K, SEED, None, full, rot, bits, SPP)
            si = leaf_si(hf, sc)
            wt, at = _cu(w).requires_grad_(True), dw.alpha_t.clone().requires_grad_(True)
            img, val, words = hf.glossy_lighting(sc.shape, si, sc.ray, env, at, eta=eta, spp=SPP, num_rays=K, seed=SEED, weight=wt,
                                                 return_value=True, return_visibility=True)
            assert torch.equal(words, dw.words & ((1 << K) - 1 if K < 32 else -1))
            ri, rv = G.forward(*args)
            lit = bits.any(0)
            assert not _np(val)[~lit].any()
            err = {"value": np.abs(_np(val) - rv)[keep].max(), "image": np.abs(_np(img) - ri)[kp].max()}
            assert lit[keep].sum() > 200 and rv.max() > 0.01
            ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
            gm, gw, ga, gd = G.adjoint(*args, gi, gv)
            got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_weight": _np(wt.grad), "grad_alpha": _np(at.grad),
                   "grad_data": _np(env.data.grad)}
            for k_ in ("grad_sh_n", "grad_weight", "grad_alpha"):
                assert not got[k_][..., ~lit].any()                           # exact zeros where no bit is set
            err["grad_sh_n"] = _rel(got["grad_sh_n"][:, keep], gm[:, keep])
            err["grad_weight"] = _rel(got["grad_weight"][keep], gw[keep])
            err["grad_alpha"] = _rel(got["grad_alpha"][keep], ga[keep])
            err["grad_data"] = _rel(got["grad_data"], _fold(gd))
            with fwAD.dual_level():
                sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(dn.astype(np.float32))))
                envd = hf.Envmap(fwAD.make_dual(env.data.detach(), _cu(dd[:, :-1])), to_world=rot)
                ti, tv = hf.glossy_lighting(sc.shape, sd, sc.ray, envd, fwAD.make_dual(dw.alpha_t, _cu(da.astype(np.float32))), eta=eta,
                                            spp=SPP, num_rays=K, seed=SEED, weight=fwAD.make_dual(_cu(w), _cu(dwt.astype(np.float32))),
                                            return_value=True)
                timg, tval = fwAD.unpack_dual(ti).tangent, fwAD.unpack_dual(tv).tangent
            ddf = np.concatenate([dd[:, :-1], dd[:, :1]], 1)
            dimg, dval = G.tangent(*args, dn, dwt, da, ddf)
            assert not _np(tval)[~lit].any()
            err["dimage"], err["dvalue"] = _rel(_np(timg)[kp], dimg[kp]), _rel(_np(tval)[keep], dval[keep])
            # transposition on the device: <J u, v> = <u, J^T v>, both sides float32 results added up in float64; each side
            # is within its tolerance of the exact bilinear form, so they agree to the sum of the two
            gap = transposition_gap(((_np(timg), gi), (_np(tval), gv)),
                                    ((got["grad_sh_n"], dn), (got["grad_weight"], dwt), (got["grad_alpha"], da),
                                     (got["grad_data"], dd[:, :-1])))
            size = np.linalg.norm(dimg) * np.linalg.norm(gi) + np.linalg.norm(dval) * np.linalg.norm(gv)
            print(G.ORIGINS[oi], K, akind, name, rname, {k: "%.3g" % v for k, v in err.items()}, "left out", float((~keep).mean()),
                  "transposition", gap / size)
            assert gap <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size, gap
            for k in err:
                worst[k] = max(worst[k], err[k])
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


def test_forward_and_reverse_mode_agree(hf, oracle):
    """<J u, v> = <u, J^T v> for J = glossy_lighting with respect to (sh_n, weight, alpha, data), jvp on one side and
    backward on the other, through the public function, with a scalar alpha (its gradient is torch's sum over the row);
    the bound is that of the kernels' own transposition check"""
    sc = _scene(hf, oracle, 1, False)
    env, full, rot = _envmap(hf, "sun", "identity", requires_grad=True)
    w, gi, gv, dn, dw, da, dd = (_cu(x) for x in G.test_inputs(sc.n, full.shape))
    si = leaf_si(hf, sc)
    wt = w.clone().requires_grad_(True)
    al = torch.tensor(0.3, device="cuda", requires_grad=True)
    img, val = hf.glossy_lighting(sc.shape, si, sc.ray, env, al, eta=1.5, spp=SPP, num_rays=3, seed=SEED, weight=wt, return_value=True)
    ((img * gi).sum() + (val * gv).sum()).backward()
    assert al.grad.shape == ()
    rhs = sum(float((g.double() * t.double()).sum()) for g, t in ((si.sh_frame.n.grad, dn), (wt.grad, dw), (env.data.grad, dd[:, :-1]))) + \
        0.7 * float(al.grad)
    with fwAD.dual_level():
        sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), dn))
        envd = hf.Envmap(fwAD.make_dual(env.data.detach(), dd[:, :-1].contiguous()), to_world=rot)
        ald = fwAD.make_dual(torch.tensor(0.3, device="cuda"), torch.tensor(0.7, device="cuda"))
        ti, tv = hf.glossy_lighting(sc.shape, sd, sc.ray, envd, ald, eta=1.5, spp=SPP, num_rays=3, seed=SEED, weight=fwAD.make_dual(w, dw),
                                    return_value=True)
        timg, tval = fwAD.unpack_dual(ti).tangent, fwAD.unpack_dual(tv).tangent
    lhs = float((timg.double() * gi.double()).sum() + (tval.double() * gv.double()).sum())
    size = float(timg.double().norm() * gi.double().norm() + tval.double().norm() * gv.double().norm())
    print("lhs", lhs, "rhs", rhs, "relative to |J u| |v|", abs(lhs - rhs) / size)
    assert abs(lhs) > 0 and abs(lhs - rhs) <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """glossy_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's chain: the restatement's
    grad_sh_n (fed with the GPU's records and bits) carried to the heights by the oracle's adjoint (flat shading) or by
    hf_adjoint, which tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: four times the
    float32 error of grad_sh_n + the 1e-5 of the sky row's chain to the heights, as the reflect row's chain test has it."""
    sc0 = _scene(hf, oracle, 1, face_normals)
    dw = _draws(hf, sc0, 0.3)
    K = 3
    env, full, rot = _envmap(hf, "gradient", "rotated")
    shape = hf.Heightfield(heightfield=sc0.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc0.ray, hf.RayFlags.All)
    img, words = hf.glossy_lighting(shape, si, sc0.ray, env, 0.3, eta=1.5, spp=SPP, num_rays=K, seed=SEED, return_visibility=True)
    assert torch.equal(words, dw.words & 7) and float(img.detach().sum()) > 0
    keep = _sure(sc0, dw, K).reshape(-1, SPP).all(1)
    gi = np.random.default_rng(11).normal(size=sc0.n // SPP).astype(np.float32) * keep
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(x) for x in (si.n, si.sh_frame.n, sc0.ray.d, si.t))
    gm, _, _, _ = G.adjoint(*a, None, None, 0.3, 1.5, K, SEED, None, full, rot, dw.bits[:K], SPP, gi, None)
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
    dw = _draws(hf, sc, "row")
    env, full, rot = _envmap(hf, "sun", "rotated")
    w, gi, gv, dn, dwt, da, dd = (_cu(x) for x in G.test_inputs(sc.n, full.shape))
    runs = []
    for _ in range(2):
        si = leaf_si(hf, sc)
        wt, at = w.clone().requires_grad_(True), dw.alpha_t.clone().requires_grad_(True)
        img, val, vis = hf.glossy_lighting(sc.shape, si, sc.ray, env, at, eta=1.5, spp=SPP, num_rays=32, seed=SEED, weight=wt,
                                           return_value=True, return_visibility=True)
        ((img * gi).sum() + (val * gv).sum()).backward()
        runs.append((img.detach(), val.detach(), vis, si.sh_frame.n.grad, wt.grad, at.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # n = 0 is legal
    e = hf.SurfaceInteraction3f()
    e.p, e.n, e.t = (x.detach()[..., :0].contiguous() for x in (sc.si.p, sc.si.n, sc.si.t))
    e.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach()[:, :0].contiguous().requires_grad_(True))
    ray0 = hf.Ray3f(sc.ray.o[:, :0].contiguous(), sc.ray.d[:, :0].contiguous())
    img0, val0, vis0 = hf.glossy_lighting(sc.shape, e, ray0, env, 0.3, return_value=True, return_visibility=True)
    assert img0.shape == (0,) and val0.shape == (0,) and vis0.shape == (0,)
    (img0.sum() + val0.sum()).backward()
    assert len(hf.glossy_rays(e, ray0, 0.3, 0)) == 0
    # an all-miss wavefront: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, valm, vism = hf.glossy_lighting(sc.shape, sim, up, env, 0.3, spp=SPP, return_value=True, return_visibility=True)
    assert not bool(vism.any()) and not bool(valm.any()) and not bool(imgm.any())
    assert bool((hf.glossy_rays(sim, up, 0.3, 5).maxt == -1.0).all())
    # an inactive lane and a non-finite roughness: no bit, no value; the others unchanged
    act = torch.arange(sc.n, device="cuda") % 3 != 0
    bad = torch.where(act, dw.alpha_t, torch.full_like(dw.alpha_t, float("nan")))
    for kw, al in (({"active": act}, dw.alpha_t), ({}, bad)):
        _, v2, b2 = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, al, eta=1.5, spp=SPP, num_rays=32, seed=SEED, weight=w,
                                       return_value=True, return_visibility=True, **kw)
        assert not bool(b2[~act].any()) and not bool(v2[~act].any())
        assert torch.equal(b2[act], runs[0][2][act]) and torch.equal(v2[act], runs[0][1][act])
    for bad_kw in ({"eta": -1.0}, {"spp": 3}, {"num_rays": 0}, {"num_rays": 33}):           # (2300 is no multiple of 3)
        with pytest.raises(hf.HfError):
            hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, 0.3, **bad_kw)
    with pytest.raises(ValueError):
        hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, torch.full((7,), 0.3, device="cuda"))


@pytest.mark.parametrize("spp", [1, 3, 4])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, spp):
    """n = spp * 151; guard values around every output row; the slice equals the slice of the whole wavefront (ray_id
    carries the ids); every optional pointer NULL in turn"""
    sc = _scene(hf, oracle, 1, True)
    dw = _draws(hf, sc, "row")
    lib = hf._capi.lib()
    env, full, rot = _envmap(hf, "sun", "rotated")
    dat = _cu(full.astype(np.float32))
    H, W = full.shape
    eta, K = 1.5, 32
    _, whole_val, _ = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, dw.alpha_t, eta=eta, spp=1, num_rays=K, seed=SEED,
                                         return_value=True, return_visibility=True)
    n, GB = spp * 151, 96
    npix = n // spp
    start = 640
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t, al = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t), cut(dw.alpha_t)
    ids = torch.arange(start, start + n, device="cuda", dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    mid = (None, None, al.data_ptr(), eta, K, SEED, ids.data_ptr(), W, H, dat.data_ptr(), C.byref(env._rot))
    fwd = lambda image, value, vis: hf._capi.check(lib.hf_glossy_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d),
                                                                          t.data_ptr(), *mid, image, value, vis, stream))
    img, ip = guarded(npix, GB); val, vp = guarded(n, GB); vis, vsp = guarded(n, GB, 1, torch.int32)
    fwd(ip[0], vp[0], vsp[0])
    assert intact(img, npix, GB) and intact(val, n, GB) and intact(vis, n, GB)
    assert torch.equal(vis[0, GB:GB + n], dw.words[start:start + n]) and torch.equal(val[0, GB:GB + n], whole_val[start:start + n])
    assert int((vis[0, GB:GB + n] != 0).sum()) > 0
    want = val[0, GB:GB + n].reshape(npix, spp).double().mean(1)
    assert float((img[0, GB:GB + npix] - want).abs().max()) <= 2.5e-7 * float(want.abs().max())
    # (the film: one product and at most three additions per pixel, each rounded to 2^-24 of the largest value: 2.5e-7)
    for skip in range(3):       # every optional output NULL in turn: the others are unchanged
        img2, ip2 = guarded(npix, GB); val2, vp2 = guarded(n, GB); vis2, vsp2 = guarded(n, GB, 1, torch.int32)
        fwd(None if skip == 0 else ip2[0], None if skip == 1 else vp2[0], None if skip == 2 else vsp2[0])
        if skip != 0:
            assert intact(img2, npix, GB) and float((img2 - img).abs().max()) <= 2.5e-7 * float(want.abs().max())
        else:
            assert bool((img2 == GUARD).all())
        assert torch.equal(val2, val) if skip != 1 else bool((val2 == GUARD).all())
        assert torch.equal(vis2, vis) if skip != 2 else bool((vis2 == int(GUARD)).all())
    words = vis[0, GB:GB + n].contiguous()
    ones, onesp = torch.ones((3, n), device="cuda"), torch.ones(npix, device="cuda")
    head = (n, spp, rows(sn), rows(d), t.data_ptr(), *mid, words.data_ptr())
    adj = lambda *tail: hf._capi.check(lib.hf_glossy_lighting_adjoint(*head, *tail, stream))
    gn, gnp = guarded(n, GB, 3); gw, gwp = guarded(n, GB); ga, gap = guarded(n, GB)
    gd = torch.full((H * W + 2 * GB,), 0.0, device="cuda"); gd[:GB] = GUARD; gd[GB + H * W:] = GUARD
    adj(onesp.data_ptr(), ones.data_ptr(), gnp, gwp[0], gap[0], gd.data_ptr() + 4 * GB)
    assert intact(gn, n, GB) and intact(gw, n, GB) and intact(ga, n, GB) and bool((gd[:GB] == GUARD).all()) and bool((gd[GB + H * W:] == GUARD).all())
    assert float(gd[GB:GB + H * W].abs().sum()) > 0 and float(ga[0, GB:GB + n].abs().sum()) > 0
    # each adjoint output NULL in turn, and each upstream NULL
    gn2, gnp2 = guarded(n, GB, 3); gw2, gwp2 = guarded(n, GB); ga2, gap2 = guarded(n, GB)
    adj(onesp.data_ptr(), ones.data_ptr(), None, gwp2[0], None, None)
    adj(onesp.data_ptr(), ones.data_ptr(), gnp2, None, gap2[0], None)
    assert torch.equal(gn2, gn) and torch.equal(gw2, gw) and torch.equal(ga2, ga)
    g1, g1p = guarded(n, GB, 3); g2, g2p = guarded(n, GB, 3)
    adj(onesp.data_ptr(), None, g1p, None, None, None)
    adj(None, ones.data_ptr(), g2p, None, None, None)
    scale = float(gn[:, GB:GB + n].abs().max())
    assert float((g1 + g2 - gn)[:, GB:GB + n].abs().max()) <= 1e-6 * scale
    dimg, dip = guarded(npix, GB); dval, dvp = guarded(n, GB)
    ddat = torch.ones((H, W), device="cuda")
    tail = (rows(ones), ones.data_ptr(), ones.data_ptr(), ddat.data_ptr())
    tan = lambda *out: hf._capi.check(lib.hf_glossy_lighting_tangent(*head, *tail, *out, stream))
    tan(dip[0], dvp[0])
    assert intact(dimg, npix, GB) and intact(dval, n, GB)
    wantd = dval[0, GB:GB + n].reshape(npix, spp).double().mean(1)
    assert float((dimg[0, GB:GB + npix] - wantd).abs().max()) <= 2.5e-7 * float(dval[0, GB:GB + n].abs().max())
    dimg2, dip2 = guarded(npix, GB); dval2, dvp2 = guarded(n, GB)
    tan(dip2[0], None)
    tan(None, dvp2[0])
    assert torch.equal(dimg2, dimg) and torch.equal(dval2, dval)
    # every tangent input NULL in turn: the sum of the four single-input tangents is the whole
    # (each part is a few float32 roundings of its own size off: 1e-6 of the largest part)
    parts, size = torch.zeros(n, device="cuda", dtype=torch.float64), float(dval[0, GB:GB + n].abs().max())
    for j in range(4):
        dv, dvq = guarded(n, GB)
        one = [None] * 4; one[j] = tail[j]
        hf._capi.check(lib.hf_glossy_lighting_tangent(*head, *one, None, dvq[0], stream))
        parts += dv[0, GB:GB + n].double()
        size = max(size, float(dv[0, GB:GB + n].abs().max()))
    assert float((parts - dval[0, GB:GB + n].double()).abs().max()) <= 1e-6 * size
    ro, rop = guarded(n, GB, 3); rd, rdp = guarded(n, GB, 3); rm, rmp = guarded(n, GB); rh, rhp = guarded(n, GB, 3)
    ray_args = (n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, al.data_ptr(), 31, SEED, ids.data_ptr())
    hf._capi.check(lib.hf_glossy_rays(*ray_args, rop, rdp, rmp[0], rhp, stream))
    assert intact(ro, n, GB) and intact(rd, n, GB) and intact(rm, n, GB) and intact(rh, n, GB)
    assert torch.equal(rm[0, GB:GB + n], dw.rr[31].maxt[start:start + n]) and torch.equal(rh[:, GB:GB + n], dw.hh[31][:, start:start + n])
    rd2, rdp2 = guarded(n, GB, 3)
    hf._capi.check(lib.hf_glossy_rays(*ray_args, rop, rdp2, rmp[0], None, stream))        # out_h is optional
    assert torch.equal(rd2, rd)
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    dw = _draws(hf, sc, 0.3)
    lib = hf._capi.lib()
    env, full, rot = _envmap(hf, "gradient", "rotated")
    dat = _cu(full.astype(np.float32))
    H, W = full.shape
    K = 3
    p, nr, sn, d, t = (x.detach().contiguous() for x in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    img = torch.zeros(sc.n // SPP, device="cuda"); value = torch.zeros(sc.n, device="cuda")
    vis = torch.zeros(sc.n, dtype=torch.int32, device="cuda")
    gn = torch.zeros((3, sc.n), device="cuda"); ga = torch.zeros(sc.n, device="cuda"); timg = torch.zeros(sc.n // SPP, device="cuda")
    gi, ones = torch.ones(sc.n // SPP, device="cuda"), torch.ones((3, sc.n), device="cuda")
    mid = (None, None, dw.alpha_t.data_ptr(), 1.5, K, SEED, None, W, H, dat.data_ptr(), C.byref(env._rot))

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        hf._capi.check(lib.hf_glossy_lighting(sc.shape._h, sc.n, SPP, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), *mid,
                                              img.data_ptr(), value.data_ptr(), vis.data_ptr(), s))
        head = (sc.n, SPP, rows(sn), rows(d), t.data_ptr(), *mid, vis.data_ptr())
        hf._capi.check(lib.hf_glossy_lighting_adjoint(*head, gi.data_ptr(), None, rows(gn), None, ga.data_ptr(), None, s))
        hf._capi.check(lib.hf_glossy_lighting_tangent(*head, rows(ones), None, ones.data_ptr(), None, timg.data_ptr(), None, s))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    outs = (img, value, vis, gn, ga, timg)
    first = [x.clone() for x in outs]
    assert torch.equal(vis, dw.words & 7) and float(img.sum()) > 0 and float(gn.abs().sum()) > 0 and float(timg.abs().sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for x in outs:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def _flat(hf, tilt=0.5):
    """a flat field (nothing occludes) seen under the angle `tilt` from the vertical by a 24 x 24 x 4 parallel wavefront
    (2304 samples: one sample near a mask decision is within the cap)"""
    shape = hf.Heightfield(heightfield=torch.full((16, 16), 0.5, device="cuda"), max_height=0.5)
    xs = (torch.arange(48, device="cuda", dtype=torch.float32) + 0.5) / 48 * 0.8
    py, px = torch.meshgrid(xs - 0.43, xs - 0.37, indexing="ij")           # (off the grid's edges and diagonals)
    o = torch.stack([px.reshape(-1) + math.tan(tilt), py.reshape(-1), torch.full((px.numel(),), 1.25, device="cuda")]).contiguous()
    d = torch.zeros_like(o); d[0] = -math.sin(tilt); d[2] = -math.cos(tilt)
    ray = hf.Ray3f(o, d)
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid().all())
    return shape, si, ray


@pytest.mark.parametrize("alpha", [0.3, 0.6])
def test_flat_field_under_a_constant_map_shows_the_mean_smith_term(hf, alpha):
    shape, si, ray = _flat(hf)
    n, K = len(ray), 8
    env = hf.Envmap(torch.ones((5, 8), device="cuda"))
    img, val, words = hf.glossy_lighting(shape, si, ray, env, alpha, eta=0.0, spp=4, num_rays=K, seed=SEED, return_value=True,
                                         return_visibility=True)
    a = tuple(_np(x) for x in (si.n, si.sh_frame.n, ray.d, si.t))
    bits = G.unpack(_np(words), K)
    want, sure = np.zeros(n), np.ones(n, bool)
    el, _ = G.eligible(*a, None, alpha)
    for k in range(K):
        dr = G.draw(a[1], a[2], alpha, np.arange(n), k, SEED)
        tr, m = G.traced(a[0], dr, el)
        sure &= m > MARGIN
        assert np.array_equal(bits[k][m > MARGIN], tr[m > MARGIN])          # nothing occludes: a traced direction is visible
        want += np.where(bits[k], G.smith(np.float64(alpha), dr.co)[0], 0.0) / K
    assert float((~sure).mean()) <= UNSURE_CAP and bits.mean() > 0.5
    got = _np(val)
    print("alpha", alpha, "largest difference", np.abs(got - want)[sure].max(), "mean value", got.mean())
    assert np.all(got <= 1.0) and np.all(got >= 0.0)
    assert np.abs(got - want)[sure].max() <= TOL["value"]
    assert float((img - val.reshape(-1, 4).mean(1)).abs().max()) <= 2.5e-7


def test_mirror_limit_shows_the_reflection_rows_image(hf, oracle):
    """alpha = 1e-4, the gradient map, num_rays = 4: the image of hf_reflect_lighting on the same wavefront.  Bound: four
    times the difference the float64 restatements of the two rows show on this scene (each fed its row's visibility from
    the GPU) plus the image tolerance"""
    for face_normals in (True, False):
        sc = _scene(hf, oracle, 1, face_normals)
        env, full, rot = _envmap(hf, "gradient", "identity")
        for eta in ETAS:
            gimg, words = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, 1e-4, eta=eta, spp=SPP, num_rays=4, seed=SEED,
                                             return_visibility=True)
            rimg, vis = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, eta=eta, spp=SPP, return_visibility=True)
            ref_g, _ = G.forward(*sc.a, None, None, 1e-4, eta, 4, SEED, None, full, rot, G.unpack(_np(words), 4), SPP)
            ref_r, _ = R.forward(*sc.a, None, None, eta, full, rot, _np(vis).astype(bool), SPP)
            bound = 4 * float(np.abs(ref_g - ref_r).max()) + TOL["image"]
            diff = float((gimg - rimg).abs().max())
            print("face_normals", face_normals, "eta", eta, "difference", diff, "restatements differ by", float(np.abs(ref_g - ref_r).max()),
                  "bound", bound)
            assert float(rimg.max()) > 0.01 and diff <= bound


def test_inverse_roughness_example_descends(hf):
    import inverse_roughness
    hist, alphas, alpha_true = inverse_roughness.main(["--size", "32", "--steps", "30", "--quiet"])
    print("loss", hist[0], "->", hist[-1], "alpha", alphas[0], "->", alphas[-1], "true", alpha_true)
    assert math.isfinite(hist[-1]) and hist[-1] < hist[0]
    assert abs(alphas[-1] - alpha_true) < abs(alphas[0] - alpha_true)

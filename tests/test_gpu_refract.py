"""The refraction view on the GPU (hf_bitmap_eval, _adjoint, hf_refract_lighting, _adjoint, _tangent; Bitmap,
refraction_lighting, dielectric_lighting) on the scene of the caustic row's tests: sine_heights(96), max_height 0.5, a
64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0), both face_normals modes, eta 1.33 and
1 / 1.33, the receiver plane_z(z, (-1, 1), (-1, 1), 16, 8) at z = -0.5 (below the terrain's bound) and z = 0.2 (cutting
through it) carrying a 16 x 8 texture (a smooth sum of sines, a random one), both wraps, sigma_t 0 and 0.7.
  (a) vis and pos bit for bit hf_caustic_lighting's, vis bit for bit hf_caustic_rays + hf_ray_test, and for sigma_t = 0
      the value on lit lanes bit for bit ((caustic value) eta_ti^2) * Bitmap.eval(pos) formed in float32 torch;
  (b) value, image, every gradient and both tangents against the float64 restatement (tests/refract_ref.py) fed the GPU's
      visibility; transposition on the device; forward_ad against backward through the public function;
  (c) the chain refraction_lighting -> loss -> backward -> dL/dheight against the restatement's gradients carried by the
      oracle's adjoint;
  (d) repeatability, n = 0, an all-miss wavefront, n = spp * 151 with guard bands, every optional output and gradient
      NULL in turn, a captured graph;
  (e) a flat field seen straight down and at 40 degrees, and dielectric_lighting as the sum of its two rows;
  (f) examples/inverse_refraction.py descends.

Tolerances (scripts/refract_f32_error.py computes them on the CPU, profiles/refract/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records, over
sigma_t, both textures and both wraps, by at most the figures of F32 below (value and image absolute, every derivative as
the L2 norm of the difference over the L2 norm of the float64 result; the maxima come from eta = 1 / 1.33, whose lanes near
the critical angle carry a factor 1 / cos_theta_t).  The GPU is allowed four times that: another operation order and fused
multiply-adds.  Lit lanes whose float64 landing position lies within BORDER = 5e-3 texel of a cell border of the lookup
are left out of the per-sample comparisons (the float32 position error is at most 1.06e-3 texel there, so four times it
stays below BORDER): at most 3e-2 of the lit lanes (the restatement alone leaves out at most 2.27 %)."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import caustic_ref as CR
import refract_ref as R
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, _rel, base_scene, guarded, intact, rows, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
ETAS = (1.33, 1 / 1.33)
PLANES = (-0.5, 0.2)
SIGMAS = (0.0, 0.7)
WRAPS = ("clamp", "repeat")
TW, TH, SPP = 16, 8, 4
F32 = {"value": 7.38e-4, "image": 1.85e-4, "grad_sh_n": 9.85e-4, "grad_p": 3.84e-5, "grad_weight": 3.74e-6, "grad_tex": 9.46e-6,
       "dvalue": 1.31e-3, "dimage": 1.33e-3}
TOL = {k: 4 * v for k, v in F32.items()}
MARGIN = 1e-5          # the caustic row's: a lane on which a mask's deciding quantity is below this is decided by rounding
BORDER = 5e-3          # texels
LEFT_OUT_CAP = 3e-2    # of the lit lanes
TEX = R.textures(TW, TH)


def _rcv(hf, z):
    return hf.Receiver.plane_z(z, (-1.0, 1.0), (-1.0, 1.0), TW, TH), R.plane_z(z, (-1.0, 1.0), (-1.0, 1.0), TW, TH)


def _bitmap(hf, name, wrap, requires_grad=False):
    data = _cu(TEX[name])
    return hf.Bitmap(data.requires_grad_(True) if requires_grad else data, wrap=wrap)


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """the wavefront from origin `oi` on the shape in the given shading mode, its records as numpy, once for all tests"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), ORIGINS[oi], face_normals)
        sc.a = tuple(sc.np[k] for k in ("p", "n", "sh_n", "d", "t"))                 # the restatement's first five arguments
        sc.runs = {}
        _SCENES[key] = sc
    return _SCENES[key]


def _run(hf, sc, eta, z):
    """the caustic row's answers for one (eta, receiver) on a scene and the lanes the comparisons keep, once"""
    key = (eta, z)
    if key not in sc.runs:
        rcv, rref = _rcv(hf, z)
        r = types.SimpleNamespace(rcv=rcv, rref=rref)
        r.rays = hf.caustic_rays(sc.si, sc.ray, rcv, eta)
        r.occluded = sc.shape.ray_test(r.rays)
        r.pos, r.value, r.vis = hf.caustic_lighting(sc.shape, sc.si, sc.ray, rcv, eta=eta, power=1.0, return_visibility=True)
        r.v = CR.vertex(*sc.a, None, eta, rref)
        vis = _np(r.vis).astype(bool)
        r.visn = vis
        sure = ((r.v.margin > MARGIN) | ~sc.hit) & (vis == (r.v.traced & vis))
        assert (~sure).mean() <= UNSURE_CAP
        _, _, pos64 = R.forward(*sc.a, None, None, eta, 0.0, rref, TEX["smooth"], R.CLAMP, vis)
        r.keep = sure & vis & ~R.near_border(pos64, BORDER)
        r.left_out = float((vis & ~r.keep).sum() / vis.sum())
        r.pix = R.whole_pixels(r.keep | (sure & ~vis), SPP)
        inside = vis & (pos64[0] >= 0) & (pos64[0] <= TW) & (pos64[1] >= 0) & (pos64[1] <= TH)
        r.inside = float(inside.sum() / vis.sum())
        sc.runs[key] = r
    return sc.runs[key]


@pytest.mark.parametrize("face_normals", [True, False])
def test_masks_positions_and_values_are_the_caustic_rows_bit_for_bit(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        ci = -(sc.si.sh_frame.n.detach() * sc.ray.d).sum(0)
        w = _cu(R.inputs(sc.n, SPP, (TH, TW)).w)
        for eta in ETAS:
            eta32 = torch.tensor(eta, dtype=torch.float32, device="cuda")
            e_ti = torch.where(ci >= 0, 1.0 / eta32, eta32)
            for z in PLANES:
                r = _run(hf, sc, eta, z)
                lit = r.vis.bool()
                two = (r.rays.maxt >= 0) & ~r.occluded
                assert torch.equal(lit, two)
                assert r.left_out <= LEFT_OUT_CAP and 0.4 < r.inside < 0.995, (r.left_out, r.inside)
                _, cw, _ = hf.caustic_lighting(sc.shape, sc.si, sc.ray, r.rcv, eta=eta, power=1.0, weight=w, return_visibility=True)
                for name in TEX:
                    for wrap in WRAPS:
                        bm = _bitmap(hf, name, wrap)
                        L = bm.eval(r.pos)
                        for sigma_t in SIGMAS:
                            for weight, cv in ((None, r.value), (w, cw)):
                                img, val, vis, pos = hf.refraction_lighting(sc.shape, sc.si, sc.ray, r.rcv, bm, eta=eta, sigma_t=sigma_t,
                                                                            spp=SPP, weight=weight, return_value=True,
                                                                            return_visibility=True, return_position=True)
                                assert torch.equal(vis, r.vis) and torch.equal(pos, r.pos)
                                assert bool((val[~lit] == 0).all())
                                if sigma_t == 0.0:
                                    want = (cv * (e_ti * e_ti)) * L
                                    assert torch.equal(val[lit], want[lit]), int((val[lit] != want[lit]).sum())
                                else:
                                    assert bool((val[lit].abs() <= (cv * (e_ti * e_ti) * L)[lit].abs()).all())
                                want_img = val.reshape(-1, SPP).double().mean(1)
                                assert float((img - want_img).abs().max()) <= 2.5e-7 * float(want_img.abs().max())


def test_bitmap_eval_against_the_restatement_and_its_derivatives(hf):
    """hf_bitmap_eval / _adjoint alone: positions inside, outside, on texel centres, not finite and beyond 2^23, both
    wraps; the value within eight roundings of 2^-25 of the float64 lookup of the same float32 position (two complements,
    three products and three fused multiply-adds of values of at most 1) + the rounding of q = pos - 0.5, 2^-24 |q| with
    |q| <= Q = 40.5 here, times a texel difference of at most 1; the slopes likewise (a second difference of at most 2
    for the rounding of q); the texel gradient within
    the worst case of a float32 sum of n terms, n 2^-24; backward and forward_ad through Bitmap.eval"""
    rng = np.random.default_rng(4)
    n, Q = 4096 + 37, 40.5
    pos = rng.uniform(-20, 40, (2, n)).astype(np.float32)
    pos[:, :8] = np.array([[0.5, 15.5, 0.0, 16.0, np.inf, -np.inf, np.nan, 2.0 ** 23 + 1], [0.5, 7.5, 8.0, 0.0, 3.0, 3.0, 3.0, 3.0]], np.float32)
    pos[:, 8:12] = pos[::-1, 4:8]
    act = rng.uniform(size=n) < 0.9
    gout = rng.normal(size=n).astype(np.float32)
    dtex, dpos = rng.normal(size=(TH, TW)).astype(np.float32), rng.normal(size=(2, n)).astype(np.float32)
    for name, tex in TEX.items():
        for wrap, wr in zip(WRAPS, (R.CLAMP, R.REPEAT)):
            e = R.lookup(tex, pos, wr)
            bm = _bitmap(hf, name, wrap, requires_grad=True)
            p = _cu(pos).requires_grad_(True)
            out = bm.eval(p, active=_cu(act))
            got = _np(out)
            assert not got[~act].any() and np.abs(got - e.L)[act].max() <= (4 + Q) * 2.0 ** -24
            (out * _cu(gout)).sum().backward()
            gp = _np(p.grad)
            assert not gp[:, ~act].any()
            ref = np.stack([e.Lx, e.Ly]) * gout
            assert np.abs(gp - ref)[:, act].max() <= (8 + 2 * Q) * 2.0 ** -24 * np.abs(gout).max()
            gt = np.zeros(tex.size)
            for j in range(4):
                np.add.at(gt, e.idx[j][act], (gout * e.b[j])[act])
            assert _rel(_np(bm.data.grad).ravel(), gt) <= n * 2.0 ** -24
            with fwAD.dual_level():
                bd = hf.Bitmap(fwAD.make_dual(bm.data.detach(), _cu(dtex)), wrap=wrap)
                tan = fwAD.unpack_dual(bd.eval(fwAD.make_dual(_cu(pos), _cu(dpos)), active=_cu(act))).tangent
            # (an inf or nan tangent direction times a zero slope is of no interest: finite positions only)
            fin = act & np.isfinite(pos).all(0)
            dref = e.Lx * dpos[0] + e.Ly * dpos[1] + sum(e.b[j] * dtex.ravel()[e.idx[j]] for j in range(4))
            assert np.abs(_np(tan) - dref)[fin].max() <= 1e-5 * np.abs(dref[fin]).max()
            if wrap == "repeat":
                assert not got[4:12].any() and not gp[:, 4:12].any()


def _leaf_si(hf, sc):
    si = hf.SurfaceInteraction3f()
    si.p, si.n, si.t = sc.si.p.detach().clone().requires_grad_(True), sc.si.n.detach(), sc.si.t.detach()
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True))
    return si


def _dual_si(hf, sc, dn, dp):
    sd = hf.SurfaceInteraction3f()
    sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), dp), sc.si.n.detach(), sc.si.t.detach()
    sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), dn))
    return sd


@pytest.mark.parametrize("face_normals", [True, False])
@pytest.mark.parametrize("eta", ETAS)
def test_values_adjoint_and_tangent_against_the_restatement(hf, oracle, eta, face_normals):
    worst = {k: 0.0 for k in TOL}
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        x = R.inputs(sc.n, SPP, (TH, TW))
        for z in PLANES:
            r = _run(hf, sc, eta, z)
            keep, pix, vis = r.keep, r.pix, r.visn
            assert r.left_out <= LEFT_OUT_CAP, r.left_out
            assert keep.sum() > 1000 and pix.sum() > 1000
            for sigma_t in SIGMAS:
                for name, tex in TEX.items():
                    for wrap, wr in zip(WRAPS, (R.CLAMP, R.REPEAT)):
                        args = (*sc.a, None, x.w, eta, sigma_t, r.rref, tex, wr, vis)
                        si = _leaf_si(hf, sc)
                        wt = _cu(x.w).requires_grad_(True)
                        bm = _bitmap(hf, name, wrap, requires_grad=True)
                        img, val, vis2 = hf.refraction_lighting(sc.shape, si, sc.ray, r.rcv, bm, eta=eta, sigma_t=sigma_t, spp=SPP,
                                                                weight=wt, return_value=True, return_visibility=True)
                        assert torch.equal(vis2, r.vis)
                        rv, ri, _ = R.forward(*args, SPP)
                        err = {"value": np.abs(_np(val) - rv)[keep].max(), "image": np.abs(_np(img) - ri)[pix].max()}
                        assert rv[keep].max() > 0.2
                        ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
                        gm, gp, gw, gt = R.adjoint(*args, x.gi, x.gv, SPP)
                        got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad), "grad_weight": _np(wt.grad)}
                        for k, ref in (("grad_sh_n", gm), ("grad_p", gp), ("grad_weight", gw)):
                            assert not got[k][..., ~vis].any()                              # exact zeros where vis = 0
                            err[k] = _rel(got[k][..., keep], ref[..., keep])
                        got["grad_tex"] = _np(bm.data.grad)
                        err["grad_tex"] = _rel(got["grad_tex"], gt)
                        with fwAD.dual_level():
                            bd = hf.Bitmap(fwAD.make_dual(_cu(tex), _cu(x.dtex)), wrap=wrap)
                            ti, tv = hf.refraction_lighting(sc.shape, _dual_si(hf, sc, _cu(x.dn), _cu(x.dp)), sc.ray, r.rcv, bd, eta=eta,
                                                            sigma_t=sigma_t, spp=SPP, weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)),
                                                            return_value=True)
                            timg, tval = _np(fwAD.unpack_dual(ti).tangent), _np(fwAD.unpack_dual(tv).tangent)
                        dval, dimg = R.tangent(*args, x.dn, x.dp, x.dw, x.dtex, SPP)
                        assert not tval[~vis].any()
                        err["dvalue"], err["dimage"] = _rel(tval[keep], dval[keep]), _rel(timg[pix], dimg[pix])
                        # transposition on the device, forward_ad against backward through the public function:
                        # <J u, v> = <u, J^T v>, both sides float32 results added up in float64; each side is within its
                        # tolerance of the exact bilinear form, so they agree to the sum of the two
                        gap = transposition_gap(((timg, x.gi), (tval, x.gv)),
                                                ((got["grad_sh_n"], x.dn), (got["grad_p"], x.dp), (got["grad_weight"], x.dw),
                                                 (got["grad_tex"], x.dtex)))
                        size = np.linalg.norm(dimg) * np.linalg.norm(x.gi) + np.linalg.norm(dval) * np.linalg.norm(x.gv)
                        assert gap <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size, (gap, size)
                        for k in err:
                            worst[k] = max(worst[k], err[k])
            print(ORIGINS[oi], "z %.1f" % z, "left out %.4f" % r.left_out, "inside %.3f" % r.inside)
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """refraction_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n and grad_p
    (fed with the GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by
    hf_adjoint, which tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  The upstream gradient is
    zero on the lanes near a cell border (and on their pixels): the two sides may read another cell there.  Bound: four
    times the float32 error of grad_sh_n (the larger of the two gradients' errors) + the 1e-5 of the sky row's chain."""
    sc0 = _scene(hf, oracle, 0, face_normals)
    eta, z, sigma_t = ETAS[0], PLANES[0], SIGMAS[1]
    r0 = _run(hf, sc0, eta, z)
    x = R.inputs(sc0.n, SPP, (TH, TW))
    gv = np.where(r0.keep, x.gv, 0).astype(np.float32)
    gi = np.where(r0.pix, x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc0.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc0.ray, hf.RayFlags.All)
    bm = _bitmap(hf, "smooth", "clamp")
    img, val, vis = hf.refraction_lighting(shape, si, sc0.ray, r0.rcv, bm, eta=eta, sigma_t=sigma_t, spp=SPP, return_value=True,
                                           return_visibility=True)
    assert torch.equal(vis, r0.vis)
    ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(v) for v in (si.p, si.n, si.sh_frame.n, sc0.ray.d, si.t))
    gm, gp, _, _ = R.adjoint(*a, None, None, eta, sigma_t, r0.rref, TEX["smooth"], R.CLAMP, r0.visn, gi, gv, SPP)
    rr = _np(sc0.rays)
    if face_normals:
        t, u, v, prim = sc0.field.ray_intersect_preliminary(rr)
        gh = sc0.field.adjoint(rr, t, u, v, prim, {"sh_n": gm.astype(np.float32), "p": gp.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc0.n), device="cuda")
        ybar[1:4] = _cu(gp.astype(np.float32)); ybar[9:12] = _cu(gm.astype(np.float32))
        pi = shape.ray_intersect_preliminary(sc0.ray)
        gh = _np(shape.adjoint(sc0.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= TOL["grad_sh_n"] + 1e-5, err


def test_repeatable_and_edge_cases(hf, oracle):
    sc = _scene(hf, oracle, 0, False)
    eta, z = ETAS[1], PLANES[1]
    r = _run(hf, sc, eta, z)
    x = R.inputs(sc.n, SPP, (TH, TW))
    w, gi, gv, dn, dp = (_cu(v) for v in (x.w, x.gi, x.gv, x.dn, x.dp))
    runs = []
    for _ in range(2):
        si = _leaf_si(hf, sc)
        bm = _bitmap(hf, "random", "repeat")
        img, val, vis, pos = hf.refraction_lighting(sc.shape, si, sc.ray, r.rcv, bm, eta=eta, sigma_t=0.7, spp=SPP, weight=w,
                                                    return_value=True, return_visibility=True, return_position=True)
        ((img * gi).sum() + (val * gv).sum()).backward()
        with fwAD.dual_level():
            ti, tv = hf.refraction_lighting(sc.shape, _dual_si(hf, sc, dn, dp), sc.ray, r.rcv, bm, eta=eta, sigma_t=0.7, spp=SPP,
                                            weight=w, return_value=True)
            ti, tv = fwAD.unpack_dual(ti).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        runs.append((img.detach(), val.detach(), vis, pos, si.sh_frame.n.grad, si.p.grad, ti, tv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    bm = _bitmap(hf, "smooth", "clamp")
    # n = 0 is legal
    e = hf.SurfaceInteraction3f()
    e.p, e.n, e.t = (v.detach()[..., :0].contiguous() for v in (sc.si.p, sc.si.n, sc.si.t))
    e.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach()[:, :0].contiguous().requires_grad_(True))
    ray0 = hf.Ray3f(sc.ray.o[:, :0].contiguous(), sc.ray.d[:, :0].contiguous())
    img0, val0, vis0, pos0 = hf.refraction_lighting(sc.shape, e, ray0, r.rcv, bm, spp=SPP, return_value=True, return_visibility=True,
                                                    return_position=True)
    assert img0.shape == (0,) and val0.shape == (0,) and vis0.shape == (0,) and pos0.shape == (2, 0)
    (img0.sum() + val0.sum()).backward()
    assert bm.eval(pos0).shape == (0,)
    # an all-miss wavefront: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, valm, vism, posm = hf.refraction_lighting(sc.shape, sim, up, r.rcv, bm, spp=SPP, return_value=True, return_visibility=True,
                                                    return_position=True)
    assert not bool(vism.any()) and not bool(valm.any()) and not bool(imgm.any()) and bool((posm == -16.0).all())
    for bad in ({"eta": 0.0}, {"sigma_t": -1.0}, {"spp": 3}):
        with pytest.raises(hf.HfError):
            hf.refraction_lighting(sc.shape, sc.si, sc.ray, r.rcv, bm, **bad)
    with pytest.raises(hf.HfError):
        hf.refraction_lighting(sc.shape, sc.si, sc.ray, hf.Receiver((0, 0, -1), (1, 0, 0), (1, 1, 0)), bm)
    with pytest.raises(ValueError):
        hf.Bitmap(bm.data, wrap="mirror")


@pytest.mark.parametrize("spp", [1, 3, 4])
def test_odd_sizes_guard_bands_and_optional_outputs(hf, oracle, spp):
    """n = spp * 151 (for spp = 4: two whole workgroups, one whole batch and a part of one); guard values around every
    output row; the slice equals the slice of the whole wavefront; every optional output, gradient and tangent NULL in turn"""
    sc = _scene(hf, oracle, 0, True)
    lib = hf._capi.lib()
    eta, z, sigma_t = ETAS[0], PLANES[0], 0.7
    r = _run(hf, sc, eta, z)
    rcv = r.rcv._struct()
    tex = _cu(TEX["random"])
    _, whole_val = hf.refraction_lighting(sc.shape, sc.si, sc.ray, r.rcv, hf.Bitmap(tex, "repeat"), eta=eta, sigma_t=sigma_t, spp=1,
                                          return_value=True)
    n, G = spp * 151, 96
    npix = n // spp
    start = int(torch.nonzero(r.vis)[0]) // 64 * 64
    cut = lambda v: v.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    stream = torch.cuda.current_stream().cuda_stream
    mid = (rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, None, eta, sigma_t, rcv, TW, TH, tex.data_ptr(), 1)
    fwd = lambda image, value, vis, pos: hf._capi.check(lib.hf_refract_lighting(sc.shape._h, n, spp, *mid, image, value, vis, pos, stream))
    img, ip = guarded(npix, G); val, vp = guarded(n, G); pos, pp = guarded(n, G, 2)
    vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    fwd(ip[0], vp[0], vis.data_ptr() + G, pp)
    assert intact(img, npix, G) and intact(val, n, G) and intact(pos, n, G)
    assert bool((vis[:G] == 0x5A).all()) and bool((vis[G + n:] == 0x5A).all())
    assert torch.equal(vis[G:G + n], r.vis[start:start + n]) and torch.equal(val[0, G:G + n], whole_val[start:start + n])
    assert torch.equal(pos[:, G:G + n], r.pos[:, start:start + n]) and 0 < int(vis[G:G + n].sum()) < n
    want = val[0, G:G + n].reshape(npix, spp).double().mean(1)
    # (the film: one product and at most three additions per pixel, each rounded to 2^-24 of the largest value: 2.5e-7)
    assert float((img[0, G:G + npix] - want).abs().max()) <= 2.5e-7 * float(want.abs().max())
    # every optional output NULL in turn: the others are unchanged
    for skip in range(4):
        img2, ip2 = guarded(npix, G); val2, vp2 = guarded(n, G); pos2, pp2 = guarded(n, G, 2)
        vis2 = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        fwd(None if skip == 0 else ip2[0], None if skip == 1 else vp2[0], None if skip == 2 else vis2.data_ptr() + G,
            None if skip == 3 else pp2)
        if skip != 0:
            assert intact(img2, npix, G) and float((img2 - img).abs().max()) <= 2.5e-7 * float(want.abs().max())
        else:
            assert bool((img2 == GUARD).all())
        assert torch.equal(val2, val) if skip != 1 else bool((val2 == GUARD).all())
        assert torch.equal(vis2, vis) if skip != 2 else bool((vis2 == 0x5A).all())
        assert torch.equal(pos2, pos) if skip != 3 else bool((pos2 == GUARD).all())
    bytes_ = vis[G:G + n].contiguous()
    ones, onesp = torch.ones((3, n), device="cuda"), torch.ones(npix, device="cuda")
    head = (n, spp, *mid, bytes_.data_ptr())
    adj = lambda *o: hf._capi.check(lib.hf_refract_lighting_adjoint(*head, *o, stream))
    gn, gnp = guarded(n, G, 3); gp, gpp = guarded(n, G, 3); gw, gwp = guarded(n, G)
    gd = torch.full((TH * TW + 2 * G,), 0.0, device="cuda"); gd[:G] = GUARD; gd[G + TH * TW:] = GUARD
    adj(onesp.data_ptr(), ones.data_ptr(), gnp, gpp, gwp[0], gd.data_ptr() + 4 * G)
    assert intact(gn, n, G) and intact(gp, n, G) and intact(gw, n, G)
    assert bool((gd[:G] == GUARD).all()) and bool((gd[G + TH * TW:] == GUARD).all()) and float(gd[G:G + TH * TW].abs().sum()) > 0
    # each adjoint output NULL in turn, and each upstream NULL
    gn2, gnp2 = guarded(n, G, 3); gp2, gpp2 = guarded(n, G, 3); gw2, gwp2 = guarded(n, G)
    adj(onesp.data_ptr(), ones.data_ptr(), None, gpp2, gwp2[0], None)
    adj(onesp.data_ptr(), ones.data_ptr(), gnp2, None, None, None)
    assert torch.equal(gn2, gn) and torch.equal(gp2, gp) and torch.equal(gw2, gw)
    ga, gap = guarded(n, G, 3); gb, gbp = guarded(n, G, 3)
    adj(onesp.data_ptr(), None, gap, None, None, None)
    adj(None, ones.data_ptr(), gbp, None, None, None)
    scale = float(gn[:, G:G + n].abs().max())
    assert float((ga + gb - gn)[:, G:G + n].abs().max()) <= 1e-6 * scale
    tan = lambda *o: hf._capi.check(lib.hf_refract_lighting_tangent(*head, *o, stream))
    dtex = torch.ones((TH, TW), device="cuda")
    dimg, dip = guarded(npix, G); dval, dvp = guarded(n, G)
    tan(rows(ones), rows(ones), ones.data_ptr(), dtex.data_ptr(), dip[0], dvp[0])
    assert intact(dimg, npix, G) and intact(dval, n, G)
    wantd = dval[0, G:G + n].reshape(npix, spp).double().mean(1)
    assert float((dimg[0, G:G + npix] - wantd).abs().max()) <= 1e-6 * float(wantd.abs().max())
    # each tangent NULL in turn: the four partial tangents add up to the whole; each output NULL in turn
    parts = []
    for k in range(4):
        dv2, dvp2 = guarded(n, G)
        tan(rows(ones) if k == 0 else None, rows(ones) if k == 1 else None, ones.data_ptr() if k == 2 else None,
            dtex.data_ptr() if k == 3 else None, None, dvp2[0])
        assert intact(dv2, n, G)
        parts.append(dv2)
    assert float((sum(parts) - dval)[:, G:G + n].abs().max()) <= 1e-5 * float(dval[:, G:G + n].abs().max())
    di3, dip3 = guarded(npix, G)
    tan(rows(ones), rows(ones), ones.data_ptr(), dtex.data_ptr(), dip3[0], None)
    assert torch.equal(di3, dimg)
    # the bitmap entries beside their rows
    out, op = guarded(n, G); og, ogp = guarded(n, G, 2)
    q = pos[:, G:G + n].contiguous()
    hf._capi.check(lib.hf_bitmap_eval(n, rows(q), None, TW, TH, tex.data_ptr(), 1, op[0], ogp, stream))
    assert intact(out, n, G) and intact(og, n, G)
    out2, op2 = guarded(n, G)
    hf._capi.check(lib.hf_bitmap_eval(n, rows(q), None, TW, TH, tex.data_ptr(), 1, op2[0], None, stream))
    assert torch.equal(out2, out)
    gq, gqp = guarded(n, G, 2)
    hf._capi.check(lib.hf_bitmap_eval_adjoint(n, rows(q), None, TW, TH, tex.data_ptr(), 1, ones.data_ptr(), gqp, None, stream))
    assert intact(gq, n, G) and torch.equal(gq, og)
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    eta, z = ETAS[0], PLANES[1]
    r = _run(hf, sc, eta, z)
    lib = hf._capi.lib()
    rcv = r.rcv._struct()
    tex = _cu(TEX["smooth"])
    p, nr, sn, d, t = (v.detach().contiguous() for v in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    img = torch.zeros(sc.n // SPP, device="cuda"); val = torch.zeros(sc.n, device="cuda")
    vis = torch.zeros(sc.n, dtype=torch.uint8, device="cuda"); pos = torch.zeros((2, sc.n), device="cuda")
    gn = torch.zeros((3, sc.n), device="cuda"); gp = torch.zeros((3, sc.n), device="cuda")
    dimg = torch.zeros(sc.n // SPP, device="cuda")
    gi, ones = torch.ones(sc.n // SPP, device="cuda"), torch.ones((3, sc.n), device="cuda")
    mid = (rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, None, eta, 0.7, rcv, TW, TH, tex.data_ptr(), 0)

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        hf._capi.check(lib.hf_refract_lighting(sc.shape._h, sc.n, SPP, *mid, img.data_ptr(), val.data_ptr(), vis.data_ptr(), rows(pos), s))
        hf._capi.check(lib.hf_refract_lighting_adjoint(sc.n, SPP, *mid, vis.data_ptr(), gi.data_ptr(), None, rows(gn), rows(gp), None,
                                                       None, s))
        hf._capi.check(lib.hf_refract_lighting_tangent(sc.n, SPP, *mid, vis.data_ptr(), rows(ones), rows(ones), None, None,
                                                       dimg.data_ptr(), None, s))
    outs = (img, val, vis, pos, gn, gp, dimg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert torch.equal(vis, r.vis) and torch.equal(pos, r.pos) and float(img.abs().sum()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for v in outs:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def _flat(hf, d, k=24):
    """a flat field z = 0.5 seen along d from a k x k grid of camera rays over [-0.3, 0.3]^2"""
    shape = hf.Heightfield(heightfield=torch.full((16, 16), 1.0, device="cuda"), max_height=0.5)
    xs = (torch.arange(k, device="cuda", dtype=torch.float32) + 0.5) / k * 0.6 - 0.3
    py, px = torch.meshgrid(xs, xs, indexing="ij")
    hit = torch.stack([px.reshape(-1), py.reshape(-1), torch.full((k * k,), 0.5, device="cuda")])
    dd = torch.tensor(d, device="cuda", dtype=torch.float32)[:, None].expand(3, k * k).contiguous()
    ray = hf.Ray3f((hit - dd).contiguous(), dd)
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid().all()) and float((si.p - hit).abs().max()) <= 1e-6
    return shape, si, ray, hit


@pytest.mark.parametrize("sigma_t", SIGMAS)
@pytest.mark.parametrize("eta", [1.33, 1.5])
def test_flat_field_seen_straight_down_over_a_constant_texture(hf, eta, sigma_t):
    """(1 - F0) / eta^2 exp(-sigma_t depth) c: the Fresnel transmittance at normal incidence, the radiance-mode factor and
    Beer's law over the depth 1 of the plane z = -0.5 below the field z = 0.5.  Float32 throughout: 1e-6 relative"""
    shape, si, ray, _ = _flat(hf, (0.0, 0.0, -1.0))
    c = 0.8
    rcv = hf.Receiver.plane_z(-0.5, (-1.0, 1.0), (-1.0, 1.0), TW, TH)
    for wrap in WRAPS:
        bm = hf.Bitmap(torch.full((TH, TW), c, device="cuda"), wrap=wrap)
        img, vis = hf.refraction_lighting(shape, si, ray, rcv, bm, eta=eta, sigma_t=sigma_t, return_visibility=True)
        assert bool(vis.all())
        want = (1 - ((eta - 1) / (eta + 1)) ** 2) / eta ** 2 * math.exp(-sigma_t * 1.0) * c
        assert float((img - want).abs().max()) <= 1e-6 * want, (float(img.min()), float(img.max()), want)


def test_flat_field_seen_at_40_degrees_shows_the_ramp_at_the_snell_displaced_point(hf):
    """clamp, landing inside: the texture is the ramp L = 1 + 0.25 (x_texel - 0.5); a ray that enters at x lands at
    x + depth tan(theta_t), sin theta_t = sin theta / eta; the value is (1 - F(theta)) / eta^2 times the ramp there.  The
    position is exact to 1e-5 texel in float32 (8 texels per unit), the value to 1e-5 relative"""
    eta, a = 1.33, math.radians(40)
    shape, si, ray, hit = _flat(hf, (math.sin(a), 0.0, -math.cos(a)))
    rcv = hf.Receiver.plane_z(-0.5, (-1.0, 1.0), (-1.0, 1.0), TW, TH)
    ramp = (1 + 0.25 * torch.arange(TW, device="cuda", dtype=torch.float32))[None].expand(TH, TW).contiguous()
    img, pos = hf.refraction_lighting(shape, si, ray, rcv, hf.Bitmap(ramp, "clamp"), eta=eta, return_position=True)
    tt = math.asin(math.sin(a) / eta)
    x = (hit[0].double() + 1.0 * math.tan(tt) + 1.0) * (TW / 2)
    y = (hit[1].double() + 1.0) * (TH / 2)
    assert float(x.min()) > 0.5 and float(x.max()) < TW - 0.5
    assert float((pos[0] - x).abs().max()) <= 1e-5 * TW and float((pos[1] - y).abs().max()) <= 1e-5 * TH
    rs = (math.sin(a - tt) / math.sin(a + tt)) ** 2
    rp = (math.tan(a - tt) / math.tan(a + tt)) ** 2
    want = (1 - 0.5 * (rs + rp)) / eta ** 2 * (1 + 0.25 * (x - 0.5))
    assert float((img - want).abs().max()) <= 1e-5 * float(want.max())


def test_dielectric_lighting_is_the_sum_of_its_two_rows(hf, oracle):
    import envmap_ref as E
    sc = _scene(hf, oracle, 1, False)
    r = _run(hf, sc, ETAS[0], PLANES[0])
    env = hf.Envmap(_cu(E.MAPS["sun"](17, 9)[:, :-1].astype(np.float32)))
    bm = _bitmap(hf, "smooth", "repeat")
    w = _cu(R.inputs(sc.n, SPP, (TH, TW)).w)
    both = hf.dielectric_lighting(sc.shape, sc.si, sc.ray, env, r.rcv, bm, eta=1.33, sigma_t=0.7, spp=SPP, weight=w)
    refl = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, eta=1.33, spp=SPP, weight=w)
    refr = hf.refraction_lighting(sc.shape, sc.si, sc.ray, r.rcv, bm, eta=1.33, sigma_t=0.7, spp=SPP, weight=w)
    assert torch.equal(both, refl + refr) and float(refl.abs().sum()) > 0 and float(refr.abs().sum()) > 0


def test_inverse_refraction_example_descends(hf):
    import inverse_refraction
    hist = inverse_refraction.main(["--size", "32", "--steps", "30", "--quiet"])
    print("loss", hist[0], "->", hist[-1])
    assert math.isfinite(hist[-1]) and hist[-1] < hist[0]

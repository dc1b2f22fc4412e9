"""Refractive caustics on the GPU (hf_caustic_rays, hf_caustic_lighting, _adjoint, _tangent; caustic_lighting,
caustic_rays, caustic_film) on the scene of the sky row's tests: sine_heights(96), max_height 0.5, a 64 x 64 x 4
orthographic wavefront (16 384 light samples) from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0), both face_normals modes,
eta 1.33 and 1 / 1.33, a receiver below the terrain's bound (z = -0.5) and one that cuts through it (z = 0.2).
  (a) the materialised rays against the float64 restatement (tests/caustic_ref.py): masks on the sure lanes, origin,
      direction, maxt;
  (b) the fused kernel's visibility byte against the two-call sequence hf_caustic_rays + hf_ray_test, bit for bit;
  (c) the same byte against the oracle's ray_test on those rays, exactly;
  (d) pos and value against the restatement fed with the GPU's visibility;
  (e) adjoint and tangent against the restatement, and transposition on the device;
  (f) the chain caustic_film -> loss -> backward -> dL/dheight against the restatement's chain and the oracle's adjoint;
  (g) repeatability, n = 0, an all-miss wavefront, an odd n, guard bands, a captured graph;
  (h) forward_ad and backward agree through caustic_lighting and caustic_film;
  (i) examples/inverse_caustic.py descends; and the flux of a flat field at normal incidence.

Tolerances (scripts/caustic_f32_error.py computes them on the CPU).  The restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed
with the oracle's records, weights in [0.5, 1.5], power 1 and standard normal upstream gradients and tangents, by at most
the figures of F32 below (pos in pixels, value absolute, every derivative as the L2 norm of the difference over the L2
norm of the float64 result; the maxima over the 16 scenes come from eta = 1 / 1.33, whose lanes near the critical angle
carry a factor 1 / cos_theta_t).  The GPU is allowed four times that: another operation order and fused multiply-adds."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import caustic_ref as R
import film_ref
from row_helpers import UNSURE_CAP, _np, _rel, base_scene, guarded, intact, rows, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
ETAS = (1.33, 1 / 1.33)
PLANES = (-0.5, 0.2)
FILM = 64
F32 = {"pos": 4.25e-3, "value": 7.4e-5, "grad_sh_n": 6.6e-4, "grad_p": 5.4e-7, "grad_weight": 1.7e-6, "dpos": 2.8e-4,
       "dvalue": 2.9e-4}
TOL = {k: 4 * v for k, v in F32.items()}
# a mask is decided by the sign of a float32 quantity (c_i, <g, wi> c_i, cos_theta_t_sqr, <g, wo> <g, wi>, s, <wo, N>): a
# lane on which one of them is below this in magnitude is decided by rounding and is left out of mask comparisons
MARGIN = 1e-5


def _rcv(hf, z):
    return hf.Receiver.plane_z(z, (-1.0, 1.0), (-1.0, 1.0), FILM, FILM), R.plane_z(z, (-1.0, 1.0), (-1.0, 1.0), FILM, FILM)


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """the wavefront from origin `oi` on the shape in the given shading mode, its records as numpy, once for all tests"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, 4), ORIGINS[oi], face_normals)
        sc.a = tuple(sc.np[k] for k in ("p", "n", "sh_n", "d", "t"))                 # the restatement's first five arguments
        sc.runs = {}
        _SCENES[key] = sc
    return _SCENES[key]


def _run(hf, sc, eta, z):
    """rays, the two-call answer and the fused outputs of one (eta, receiver) on a scene, once"""
    key = (eta, z)
    if key not in sc.runs:
        rcv, rref = _rcv(hf, z)
        r = types.SimpleNamespace(rcv=rcv, rref=rref)
        r.rays = hf.caustic_rays(sc.si, sc.ray, rcv, eta)
        r.occluded = sc.shape.ray_test(r.rays)
        r.pos, r.value, r.vis = hf.caustic_lighting(sc.shape, sc.si, sc.ray, rcv, eta=eta, power=1.0, return_visibility=True)
        r.traced, r.o, r.wo, r.maxt, r.v = R.rays(*sc.a, None, eta, rref)
        r.sure = (r.v.margin > MARGIN) | ~sc.hit
        sc.runs[key] = r
    return sc.runs[key]


@pytest.mark.parametrize("face_normals", [True, False])
def test_materialised_rays_against_the_restatement(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        assert 0.1 < float(sc.hit.mean()) < 1.0
        for eta in ETAS:
            for z in PLANES:
                r = _run(hf, sc, eta, z)
                o, d, maxt = _np(r.rays.o), _np(r.rays.d), _np(r.rays.maxt)
                tr = maxt >= 0
                unsure = float((~r.sure).mean())
                print(ORIGINS[oi], "face" if face_normals else "smooth", "eta %.3f z %.1f" % (eta, z), "traced", int(tr.sum()),
                      "TIR", int((r.v.eligible & r.v.tir).sum()), "unsure", int((~r.sure).sum()))
                assert unsure <= UNSURE_CAP, unsure
                assert np.array_equal(tr[r.sure], r.traced[r.sure])
                assert np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
                both = tr & r.traced
                assert both.sum() > 1000
                # direction: unit, within a few float32 roundings of the restatement's (amplified by 1 / cos_theta_t near
                # the critical angle: the measured float32 error of dpos bounds it); origin: 1e-6 as for the sky rays
                assert np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max() <= 1e-5
                assert np.abs(d - r.wo)[:, both].max() <= TOL["dpos"], np.abs(d - r.wo)[:, both].max()
                assert np.abs(o - r.o)[:, both].max() <= 1e-6, np.abs(o - r.o)[:, both].max()
                # maxt in world units: the landing point moves by d maxt, TOL["pos"] pixels at FILM / 2 pixels per unit
                assert np.abs(maxt - r.maxt)[both].max() <= TOL["pos"] / (FILM / 2), np.abs(maxt - r.maxt)[both].max()


def test_both_outcomes_of_the_masks_occur(hf, oracle):
    """on the first origin: total internal reflection, occlusion and deposition each decide at least 1 % of the hits both
    ways, and the receiver that cuts through the bound changes at least 100 answers.  (Every hit of this wavefront is
    eligible with face normals, and at most 82 lanes are inconsistent with smooth ones: tests/test_caustic_ref.py holds
    those two masks; the `active` row below gives eligibility both outcomes here.)"""
    sc = _scene(hf, oracle, 0, True)
    hits = int(sc.hit.sum())
    for eta in ETAS:
        below, cut = _run(hf, sc, eta, PLANES[0]), _run(hf, sc, eta, PLANES[1])
        tir = int((below.v.eligible & below.v.tir).sum())
        tr = _np(below.rays.maxt) >= 0
        occ = int(_np(below.occluded)[tr].sum())
        lit = int(_np(below.vis).sum())
        print("eta %.3f" % eta, "hits", hits, "TIR", tir, "traced", int(tr.sum()), "occluded", occ, "deposited", lit)
        for count in (tir, hits - tir, occ, int(tr.sum()) - occ, lit, hits - lit):
            assert count >= 0.01 * hits, (eta, count, hits)
        # the same rays with maxt = +inf: what a walk that ignored the receiver would answer
        trc = cut.rays.maxt >= 0
        unbounded = hf.Ray3f(cut.rays.o, cut.rays.d, torch.where(trc, torch.full_like(cut.rays.maxt, math.inf), cut.rays.maxt))
        differ = int((sc.shape.ray_test(unbounded) != cut.occluded).sum())
        print("   z = 0.2: answers that maxt = s changes", differ)
        assert differ >= 100, differ
    act = torch.arange(sc.n, device="cuda") % 3 != 0
    pos, value, vis = hf.caustic_lighting(sc.shape, sc.si, sc.ray, below.rcv, eta=ETAS[1], active=act, return_visibility=True)
    assert not bool(vis[~act].any()) and torch.equal(vis[act], below.vis[act]) and torch.equal(pos[:, act], below.pos[:, act])
    assert bool((value[~act] == 0).all()) and bool((pos[:, ~act] == -16.0).all())
    assert int((~act & torch.from_numpy(sc.hit).cuda()).sum()) >= 0.01 * hits


@pytest.mark.parametrize("face_normals", [True, False])
def test_fused_equals_the_two_call_sequence_and_the_oracle(hf, oracle, face_normals):
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        for eta in ETAS:
            for z in PLANES:
                r = _run(hf, sc, eta, z)
                tr = r.rays.maxt >= 0
                two = tr & ~r.occluded
                assert torch.equal(r.vis.bool(), two), int((r.vis.bool() != two).sum())             # (b) bitwise
                rows = _np(torch.cat([r.rays.o, r.rays.d, r.rays.maxt[None]]))
                trn = _np(tr)
                occluded = sc.field.ray_test(rows[:, trn]).astype(bool)
                assert np.array_equal(_np(r.vis).astype(bool)[trn], ~occluded), int((_np(r.vis).astype(bool)[trn] == occluded).sum())  # (c)
                assert not _np(r.vis)[~trn].any()
                lit = r.vis.bool()
                assert bool((r.value[~lit] == 0).all()) and bool((r.pos[:, ~lit] == -16.0).all()) and bool((r.value[lit] > 0).all())


def _inputs(n):
    """the weights, upstream gradients and tangents the float32 error of the restatement was measured with"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    gpos, gv = rng.normal(size=(2, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dn, dp, dw = (rng.normal(size=s).astype(np.float32) for s in ((3, n), (3, n), (n,)))
    return w, gpos, gv, dn, dp, dw


def _leaf_si(hf, sc):
    si = hf.SurfaceInteraction3f()
    si.p, si.n, si.t = sc.si.p.detach().clone().requires_grad_(True), sc.si.n.detach(), sc.si.t.detach()
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True))
    return si


@pytest.mark.parametrize("face_normals", [True, False])
@pytest.mark.parametrize("eta", ETAS)
def test_values_adjoint_and_tangent_against_the_restatement(hf, oracle, eta, face_normals):
    worst = {k: 0.0 for k in TOL}
    for oi in range(2):
        sc = _scene(hf, oracle, oi, face_normals)
        w, gpos, gv, dn, dp, dw = _inputs(sc.n)
        cu = lambda x: torch.from_numpy(x).cuda()
        for z in PLANES:
            r = _run(hf, sc, eta, z)
            vis = _np(r.vis).astype(bool)
            keep = r.sure & (vis == (r.traced & vis))           # (a lane the GPU traced and the restatement did not is not sure)
            assert (~keep).mean() <= UNSURE_CAP
            args = (*sc.a, None, w, eta, 1.0, r.rref, vis)
            si = _leaf_si(hf, sc)
            wt = cu(w).requires_grad_(True)
            pos, value, vis2 = hf.caustic_lighting(sc.shape, si, sc.ray, r.rcv, eta=eta, power=1.0, weight=wt, return_visibility=True)
            assert torch.equal(vis2, r.vis) and torch.equal(pos, r.pos)
            rp, rv = R.forward(*args)
            err = {"pos": np.abs(_np(pos) - rp)[:, keep].max(), "value": np.abs(_np(value) - rv)[keep].max()}
            assert vis[keep].sum() > 1000 and rv[keep].max() > 0.5
            ((pos * cu(gpos)).sum() + (value * cu(gv)).sum()).backward()
            gm, gp, gw = R.adjoint(*args, gpos, gv)
            got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad), "grad_weight": _np(wt.grad)}
            for k, ref in (("grad_sh_n", gm), ("grad_p", gp), ("grad_weight", gw)):
                assert not got[k][..., ~vis].any()                                      # exact zeros where vis = 0
                err[k] = _rel(got[k][..., keep], ref[..., keep])
            with fwAD.dual_level():
                sd = hf.SurfaceInteraction3f()
                sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), cu(dp)), sc.si.n.detach(), sc.si.t.detach()
                sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), cu(dn)))
                tp, tv = hf.caustic_lighting(sc.shape, sd, sc.ray, r.rcv, eta=eta, power=1.0, weight=fwAD.make_dual(cu(w), cu(dw)))
                tpos, tval = fwAD.unpack_dual(tp).tangent, fwAD.unpack_dual(tv).tangent
            dpos, dval = R.tangent(*args, dn, dp, dw)
            assert not _np(tpos)[:, ~vis].any() and not _np(tval)[~vis].any()
            err["dpos"], err["dvalue"] = _rel(_np(tpos)[:, keep], dpos[:, keep]), _rel(_np(tval)[keep], dval[keep])
            # transposition on the device: <J u, v> = <u, J^T v>, both sides float32 results added up in float64; each
            # side is within its tolerance of the exact bilinear form, so they agree to the sum of the two
            gap = transposition_gap(((_np(tpos), gpos), (_np(tval), gv)),
                                    ((got["grad_sh_n"], dn), (got["grad_p"], dp), (got["grad_weight"], dw)))
            size = np.linalg.norm(dpos) * np.linalg.norm(gpos) + np.linalg.norm(dval) * np.linalg.norm(gv)
            print(ORIGINS[oi], "z %.1f" % z, {k: "%.3g" % v for k, v in err.items()}, "transposition", gap / size)
            assert gap <= (TOL["dpos"] + TOL["grad_sh_n"]) * size, gap
            for k in err:
                worst[k] = max(worst[k], err[k])
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """caustic_film -> loss -> backward() -> shape.heightfield.grad against the restatement's chain: film_ref's adjoint of
    the accumulated plane over the filter's mass, the restatement's grad_sh_n and grad_p (fed with the GPU's records and
    visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: four times the float32 error of
    grad_sh_n (the larger of the two gradients' errors) + the 1e-5 of the sky row's chain to the heights."""
    sc0 = _scene(hf, oracle, 0, face_normals)
    eta, z = ETAS[0], PLANES[0]
    rcv, rref = _rcv(hf, z)
    shape = hf.Heightfield(heightfield=sc0.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc0.ray, hf.RayFlags.All)
    pos, value, vis = hf.caustic_lighting(shape, si, sc0.ray, rcv, eta=eta, power=0.5, return_visibility=True)
    film = hf.caustic_film(pos, value, FILM, FILM)
    assert film.shape == (FILM * FILM,) and float(film.detach().sum()) > 0
    gi = np.random.default_rng(11).normal(size=FILM * FILM).astype(np.float32)
    (film * torch.from_numpy(gi).cuda()).sum().backward()
    got = _np(shape.heightfield.grad)
    visn = _np(vis).astype(bool)
    assert torch.equal(vis, _run(hf, sc0, eta, z).vis)
    a = tuple(_np(x) for x in (si.p, si.n, si.sh_frame.n, sc0.ray.d, si.t))
    rp, rv = R.forward(*a, None, None, eta, 0.5, rref, visn)
    ref_film = film_ref.forward(rv[None], None, rp, FILM, FILM, 0.5)[0][0] / R.filter_mass(0.5)
    assert np.abs(_np(film) - ref_film).max() <= 1e-4 * np.abs(ref_film).max()
    assert abs(R.filter_mass(0.5) - hf.caustic_filter_mass(0.5)) < 1e-9
    gv, _, gpos = film_ref.adjoint(rv[None], None, rp, FILM, FILM, 0.5, (gi / R.filter_mass(0.5))[None])
    gm, gp, _ = R.adjoint(*a, None, None, eta, 0.5, rref, visn, gpos, gv[0])
    r = _np(sc0.rays)
    if face_normals:
        t, u, v, prim = sc0.field.ray_intersect_preliminary(r)
        gh = sc0.field.adjoint(r, t, u, v, prim, {"sh_n": gm.astype(np.float32), "p": gp.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc0.n), device="cuda")
        ybar[1:4] = torch.from_numpy(gp.astype(np.float32)).cuda(); ybar[9:12] = torch.from_numpy(gm.astype(np.float32)).cuda()
        pi = shape.ray_intersect_preliminary(sc0.ray)
        gh = _np(shape.adjoint(sc0.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= TOL["grad_sh_n"] + 1e-5, err


def test_repeatable_and_edge_cases(hf, oracle):
    sc = _scene(hf, oracle, 0, False)
    eta, z = ETAS[1], PLANES[1]
    r = _run(hf, sc, eta, z)
    w, gpos, gv, dn, dp, dw = (torch.from_numpy(x).cuda() for x in _inputs(sc.n))
    runs = []
    for _ in range(2):
        si = _leaf_si(hf, sc)
        rays = hf.caustic_rays(si, sc.ray, r.rcv, eta)
        pos, value, vis = hf.caustic_lighting(sc.shape, si, sc.ray, r.rcv, eta=eta, weight=w, return_visibility=True)
        ((pos * gpos).sum() + (value * gv).sum()).backward()
        with fwAD.dual_level():
            sd = hf.SurfaceInteraction3f()
            sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), dp), sc.si.n.detach(), sc.si.t.detach()
            sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), dn))
            tp, tv = hf.caustic_lighting(sc.shape, sd, sc.ray, r.rcv, eta=eta, weight=w)
            tp, tv = fwAD.unpack_dual(tp).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        runs.append((rays.o, rays.d, rays.maxt, pos.detach(), value.detach(), vis, si.sh_frame.n.grad, si.p.grad, tp, tv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # n = 0 is legal
    e = hf.SurfaceInteraction3f()
    e.p, e.n, e.t = (x.detach()[..., :0].contiguous() for x in (sc.si.p, sc.si.n, sc.si.t))
    e.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach()[:, :0].contiguous().requires_grad_(True))
    ray0 = hf.Ray3f(sc.ray.o[:, :0].contiguous(), sc.ray.d[:, :0].contiguous())
    pos0, value0, vis0 = hf.caustic_lighting(sc.shape, e, ray0, r.rcv, return_visibility=True)
    assert pos0.shape == (2, 0) and value0.shape == (0,) and vis0.shape == (0,)
    (pos0.sum() + value0.sum()).backward()
    assert len(hf.caustic_rays(e, ray0, r.rcv)) == 0
    # an all-miss wavefront: rays that leave the terrain behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    posm, valuem, vism = hf.caustic_lighting(sc.shape, sim, up, r.rcv, return_visibility=True)
    assert not bool(vism.any()) and not bool(valuem.any()) and bool((posm == -16.0).all())
    assert bool((hf.caustic_rays(sim, up, r.rcv).maxt == -1.0).all())
    with pytest.raises(hf.HfError):
        hf.caustic_lighting(sc.shape, sc.si, sc.ray, r.rcv, eta=0.0)
    with pytest.raises(hf.HfError):
        hf.caustic_lighting(sc.shape, sc.si, sc.ray, hf.Receiver((0, 0, -1), (1, 0, 0), (1, 1, 0)))


def test_nothing_is_written_beside_the_rows(hf, oracle):
    """n = 256 + 64 * 3 + 5: a whole workgroup, three whole batches and a part of one; guard values around every output
    row; the slice equals the slice of the whole wavefront"""
    sc = _scene(hf, oracle, 0, True)
    lib = hf._capi.lib()
    eta, z = ETAS[0], PLANES[0]
    whole = _run(hf, sc, eta, z)
    rcv = whole.rcv._struct()
    n, G = 256 + 64 * 3 + 5, 96
    start = int(torch.nonzero(whole.vis)[0]) // 64 * 64
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    stream = torch.cuda.current_stream().cuda_stream
    head = (n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None)
    pos, pp = guarded(n, G, 2); val, vp = guarded(n, G)
    vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    hf._capi.check(lib.hf_caustic_lighting(sc.shape._h, *head, None, eta, 1.0, rcv, pp, vp[0], vis.data_ptr() + G, stream))
    assert intact(pos, n, G) and intact(val, n, G)
    assert bool((vis[:G] == 0x5A).all()) and bool((vis[G + n:] == 0x5A).all())
    assert torch.equal(vis[G:G + n], whole.vis[start:start + n]) and torch.equal(pos[:, G:G + n], whole.pos[:, start:start + n])
    assert torch.equal(val[0, G:G + n], whole.value[start:start + n]) and 0 < int(vis[G:G + n].sum()) < n
    bytes_ = vis[G:G + n].contiguous()
    ones = torch.ones((3, n), device="cuda")
    gn, gnp = guarded(n, G, 3); gp, gpp = guarded(n, G, 3); gw, gwp = guarded(n, G)
    hf._capi.check(lib.hf_caustic_adjoint(*head, None, eta, 1.0, rcv, bytes_.data_ptr(), (hf._capi._fp * 2)(*rows(ones)[:2]),
                                          ones.data_ptr(), gnp, gpp, gwp[0], stream))
    assert intact(gn, n, G) and intact(gp, n, G) and intact(gw, n, G)
    dpos, dpp = guarded(n, G, 2); dval, dvp = guarded(n, G)
    hf._capi.check(lib.hf_caustic_tangent(*head, None, eta, 1.0, rcv, bytes_.data_ptr(), rows(ones), rows(ones), ones.data_ptr(),
                                          dpp, dvp[0], stream))
    assert intact(dpos, n, G) and intact(dval, n, G)
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    hf._capi.check(lib.hf_caustic_rays(*head, eta, rcv, rop, rdp, rmp[0], stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    assert torch.equal(rm[0, G:G + n], whole.rays.maxt[start:start + n])
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    eta, z = ETAS[0], PLANES[1]
    r = _run(hf, sc, eta, z)
    lib = hf._capi.lib()
    rcv = r.rcv._struct()
    p, nr, sn, d, t = (x.detach().contiguous() for x in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    pos = torch.zeros((2, sc.n), device="cuda"); value = torch.zeros(sc.n, device="cuda")
    vis = torch.zeros(sc.n, dtype=torch.uint8, device="cuda")
    gn = torch.zeros((3, sc.n), device="cuda"); gp = torch.zeros((3, sc.n), device="cuda")
    gpos, gv = torch.ones((2, sc.n), device="cuda"), torch.ones(sc.n, device="cuda")
    head = (sc.n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None)

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        hf._capi.check(lib.hf_caustic_lighting(sc.shape._h, *head, None, eta, 1.0, rcv, rows(pos), value.data_ptr(), vis.data_ptr(), s))
        hf._capi.check(lib.hf_caustic_adjoint(*head, None, eta, 1.0, rcv, vis.data_ptr(), rows(gpos), gv.data_ptr(), rows(gn),
                                              rows(gp), None, s))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [x.clone() for x in (pos, value, vis, gn, gp)]
    assert torch.equal(vis, r.vis) and torch.equal(pos, r.pos) and torch.equal(value, r.value)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for x in (pos, value, vis, gn, gp):
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, (pos, value, vis, gn, gp)):
        assert torch.equal(a, b)


def test_forward_and_reverse_mode_agree_through_the_film(hf, oracle):
    """<J u, v> = <u, J^T v> for J = caustic_film o caustic_lighting with respect to (sh_n, p, weight), jvp on one side and
    backward on the other.  The film adds with float atomics, so neither side is repeatable to the bit; the bound is that
    of the kernels' own transposition check."""
    sc = _scene(hf, oracle, 0, False)
    eta, z = ETAS[0], PLANES[0]
    rcv, _ = _rcv(hf, z)
    w, _, _, dn, dp, dw = (torch.from_numpy(x).cuda() for x in _inputs(sc.n))
    v = torch.from_numpy(np.random.default_rng(8).normal(size=FILM * FILM).astype(np.float32)).cuda()
    si = _leaf_si(hf, sc)
    wt = w.clone().requires_grad_(True)
    film = hf.caustic_film(*hf.caustic_lighting(sc.shape, si, sc.ray, rcv, eta=eta, weight=wt), FILM, FILM)
    (film * v).sum().backward()
    rhs = sum(float((g.double() * t.double()).sum()) for g, t in ((si.sh_frame.n.grad, dn), (si.p.grad, dp), (wt.grad, dw)))
    with fwAD.dual_level():
        sd = hf.SurfaceInteraction3f()
        sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), dp), sc.si.n.detach(), sc.si.t.detach()
        sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), dn))
        out = hf.caustic_film(*hf.caustic_lighting(sc.shape, sd, sc.ray, rcv, eta=eta, weight=fwAD.make_dual(w, dw)), FILM, FILM)
        tan = fwAD.unpack_dual(out).tangent
    lhs = float((tan.double() * v.double()).sum())
    size = float(tan.double().norm() * v.double().norm())
    print("lhs", lhs, "rhs", rhs, "relative to |J u| |v|", abs(lhs - rhs) / size)
    assert abs(lhs) > 0 and abs(lhs - rhs) <= (TOL["dpos"] + TOL["grad_sh_n"]) * size


def test_flat_field_at_normal_incidence_fills_the_film_with_the_transmitted_flux(hf):
    """a flat field, light straight down on a regular grid of 2 x 2 samples per pixel over pixels 8 .. 24 of a 32 x 32 film:
    inside the lit footprint a pixel holds power (1 - F) samples-per-pixel to within 3 % -- the lattice ripple of a Gaussian
    of sigma = 0.5 px, 2 exp(-2 pi^2 sigma^2) = 1.4 %, doubled"""
    shape = hf.Heightfield(heightfield=torch.full((16, 16), 0.5, device="cuda"), max_height=0.5)
    k, eta, power = 2, 1.33, 0.25
    xs = (torch.arange(16 * k, device="cuda", dtype=torch.float32) + 0.5) / k + 8
    py, px = torch.meshgrid(xs, xs, indexing="ij")
    o = torch.stack([px.reshape(-1) / 16 - 1, py.reshape(-1) / 16 - 1, torch.full((px.numel(),), 1.0, device="cuda")])
    d = torch.zeros_like(o); d[2] = -1.0
    ray = hf.Ray3f(o.contiguous(), d)
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid().all())
    rcv = hf.Receiver.plane_z(-0.5, (-1.0, 1.0), (-1.0, 1.0), 32, 32)
    pos, value, vis = hf.caustic_lighting(shape, si, ray, rcv, eta=eta, power=power, return_visibility=True)
    assert bool(vis.all())
    assert float((pos - torch.stack([px.reshape(-1), py.reshape(-1)])).abs().max()) <= 1e-4
    F = ((eta - 1) / (eta + 1)) ** 2
    assert float((value - power * (1 - F)).abs().max()) <= 1e-6
    film = hf.caustic_film(pos, value, 32, 32).reshape(32, 32)
    want = power * (1 - F) * k * k
    inner = film[11:21, 11:21]
    print("film inside the footprint", float(inner.min()), float(inner.max()), "expected", want)
    assert float((inner / want - 1).abs().max()) < 0.03
    assert not bool(film[:5].any()) and not bool(film[:, 27:].any())


def test_inverse_caustic_example_descends(hf):
    import inverse_caustic
    hist = inverse_caustic.run(size=32, steps=30, verbose=False)
    print("loss", hist[0], "->", hist[-1])
    assert math.isfinite(hist[-1]) and hist[-1] < hist[0]

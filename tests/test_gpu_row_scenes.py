"""The ten lighting rows that came after the environment map -- directional, spot, caustic, refract, rect, projector,
reflect, glossy, specular and medium (hf_directional_*, hf_spot_*, hf_caustic_*, hf_refract_*, hf_rect_*, hf_projector_*,
hf_reflect_*, hf_glossy_*, hf_specular_*, hf_medium_*) -- on the GPU, on the scenes of tests/row_scenes.py: a general
affine to_world, a mirror with flip_normals, flip_normals seen from below; rectangular grids that are no power of two,
2300 samples (partial last wave and workgroup), the rows' rigs carried to world, the spot light `inside` ending its shadow
rays inside the field's bound, as the rect lamp `side` does; the caustic receiver `cut` crosses the relief.  The rows' own
files (tests/test_gpu_directional.py, _spot, _caustic, _refract, _rect, _projector, _reflect, _glossy, _specular, _medium) run on one identity-transformed square
field only; guard bands, odd n, NULL pointers and graphs do not depend on the transform and
stay there.  Everything here goes through the public functions.  The directional and the spot row share the first three
tests; the other rows have a section each below, with the same letters.  Per (row, scene, shading mode):
  (a) the materialised rays against the restatement on the sure lanes: masks exactly, origin, direction and maxt at the
      tolerances of the row's own file;
  (b) the fused kernel's visibility byte against the two-call sequence *_rays + shape.ray_test, bit for bit, in both
      coherence modes;
  (c) and against the oracle's ray_test, built with the same to_world and flip_normals, on those rays: exactly;
  (d) image and per-sample value against the float64 restatement fed with the GPU's records and visibility;
  (e) the adjoint (grad_sh_n, grad_p, grad_weight, the lights' own numbers) through backward() and the tangent through
      forward_ad against the restatement, and the transposition gap <J u, v> = <u, J^T v> on the device;
  (f) on `mirror_flip` (flat shading) and `affine` (smooth) the chain row -> loss -> backward() -> shape.heightfield.grad
      against the restatement's grad_sh_n and grad_p carried to the heights by the oracle's adjoint under the same
      to_world and flip_normals (flat) or by hf_adjoint (smooth);
  (g) the populations of tests/test_row_scenes.py again on the GPU's own records: a run that shadows nothing cannot pass.

Tolerances of (d) and (e): row_scenes.TOL, four times the float32 error of the restatement on these scenes
(scripts/row_scenes_f32_error.py, profiles/row_scenes/f32_error.json), in the measures of each row's own file.  Samples
on which rounding may decide a mask (a deciding quantity within the row's MARGIN; at most row_helpers.UNSURE_CAP of the
samples over the union of the lights) are left out of the comparisons; for the spot row so are the lanes within KINK of
theta = beam under the light concerned, where the slope of the falloff jumps: their upstream gradients are zero and their
tangents are not compared.

The last two sections.  `specular` traces nothing: (d), (e), (g) in specular_ref.errors()' measures with no sample left out,
its byte the directional row's launch of the same scene, and (f) through ray_intersect -> directional_lighting ->
specular_lighting.  `medium`, per (case, medium of row_scenes.MEDIA), all eight lights in one launch with 4 points per
sample: (a) to (g) with the letters above, where (c) leaves out only the lanes whose origin lies within the sky row's spawn
offset of the primary hit (at most row_helpers.UNSURE_CAP), the origins are held to TOL[medium][origin] and values,
gradients and tangents to the row's own rule (rtol 1e-5, atol 1e-7 max(1, largest |reference|)); its gradient reaches the
heights through si.t alone."""
import math
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import caustic_ref as CR
import film_ref
import glossy_ref as GL
import medium_ref as MR
import projector_ref as PJ
import rect_ref as AR
import reflect_ref as RF
import refract_ref as RR
import row_scenes as RS
import specular_ref as SP
from row_helpers import _cu, _fold, _np, _rel, envmap, leaf_si, transposition_gap

pytestmark = pytest.mark.gpu

SPP = RS.SPP
TRIPLES = [(row, name, fn) for row in RS.ROWS for name, fn in RS.CASES]
_SCENES, _RIGGED = {}, {}


def _f64(a):
    return torch.tensor(np.asarray(a, np.float64))


def _lights(hf, row, ref, params=None):
    """the public light objects of the restatement's lights (params: their tensors, leaves or duals)"""
    cls = hf.DirectionalLight if row == "directional" else hf.SpotLight
    return [cls(*(_numbers(row, L) if params is None else params[k])) for k, L in enumerate(ref)]


def _numbers(row, L):
    """the light's own numbers in the order of its reduced row"""
    return (L.to_light, L.irradiance) if row == "directional" else (L.to_world, L.intensity, L.cutoff, L.beam)


def _lighting(hf, row):
    return (hf.directional_lighting, hf.directional_rays) if row == "directional" else (hf.spot_lighting, hf.spot_rays)


def _scene(hf, oracle, name, view, face_normals):
    key = (name, view, face_normals)
    if key not in _SCENES:
        _SCENES[key] = RS.device_scene(hf, oracle, name, view, face_normals)
    return _SCENES[key]


def _rigged(hf, oracle, row, name, face_normals):
    """the scene with the row's rig on it, once: the GPU's launch of the whole rig, the restatement's masks, and (g) the
    populations of the GPU's own records and visibility, asserted before anything is compared"""
    key = (row, name, face_normals)
    if key not in _RIGGED:
        sc = _scene(hf, oracle, name, RS.VIEW_OF[row], face_normals)
        M = RS.REF[row]
        q = types.SimpleNamespace(sc=sc, M=M, row=row)
        q.names, q.ref = RS.rig(row, sc)
        q.K = len(q.ref)
        q.lights = _lights(hf, row, q.ref)
        q.x = M.inputs(sc.n, SPP, q.K)
        fused, _ = _lighting(hf, row)
        img, val, vis = fused(sc.shape, sc.si, sc.ray, q.lights, albedo=M.ALBEDO, spp=SPP, weight=_cu(q.x.w), return_value=True,
                              return_visibility=True)
        q.img, q.val, q.byte = _np(img).copy(), _np(val).copy(), _np(vis).copy()
        q.vis = M.unpack(q.byte, q.K)
        q.pop = RS.populations(row, sc, q.names, q.ref, sc.np, sc.np["d"], sc.np["t"], q.vis, sc.field)
        print(row, name, "face" if face_normals else "smooth", RS.describe(q.pop))
        RS.conditions(row, sc, q.pop)                                              # (g)
        q.traced, q.unsure = q.pop.traced, q.pop.unsure
        q.sure = ~q.pop.union
        # the (light, lane) pairs whose derivatives are compared: not at the kink of a lit lane, not decided by rounding
        steady = q.vis if row == "directional" else np.stack([M.steady(L, sc.np["p"], q.vis[k]) for k, L in enumerate(q.ref)])
        q.okl = (steady | ~q.vis) & q.sure[None]
        q.okpix = q.okl.reshape(q.K, -1, SPP).all(2)
        assert q.okl.mean() > 1 - 2 * RS.UNSURE_CAP, q.okl.mean()
        _RIGGED[key] = q
    return _RIGGED[key]


def _to_heights(hf, oracle, sc, shape, gn, gp, face_normals):
    """the restatement's grad_sh_n and grad_p [3, n] (gp None: zero) carried to the heights [H, W]: by the oracle's adjoint
    under the scene's to_world and flip_normals (flat shading), or by hf_adjoint on `shape`, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading)"""
    gp = np.zeros_like(gn) if gp is None else gp
    if face_normals:
        t, u, v, prim = sc.pi_oracle
        return sc.field.adjoint(sc.rays, t, u, v, prim, {"sh_n": gn.astype(np.float32), "p": gp.astype(np.float32)}, oracle.RAY_ALL)
    ybar = torch.zeros((18, sc.n), device="cuda")
    ybar[1:4] = _cu(gp.astype(np.float32)); ybar[9:12] = _cu(gn.astype(np.float32))
    pi = shape.ray_intersect_preliminary(sc.ray)
    return _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))


# ---- (a), (b), (c), (g) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,name,face_normals", TRIPLES)
def test_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, row, name, face_normals):
    q = _rigged(hf, oracle, row, name, face_normals)
    sc, M = q.sc, q.M
    fused, rays_of = _lighting(hf, row)
    rec = sc.np
    assert np.abs(rec["p"]).max() < 4                                                # (what the 1e-6 on origins rests on)
    assert not q.byte[~q.pop.eligible & q.sure].any()                                # not eligible: a zero byte
    worst = {"o": 0.0, "d": 0.0, "maxt": 0.0}
    ended = changed = 0
    for k, (lname, L) in enumerate(zip(q.names, q.ref)):
        ray = rays_of(sc.si, sc.ray, q.lights[k])
        o, d, maxt = _np(ray.o), _np(ray.d), _np(ray.maxt)
        tr = maxt >= 0
        # (b) the two-call sequence in both coherence modes, and the fused launch of this light alone
        old = sc.shape.ray_coherence()
        for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
            sc.shape.set_ray_coherence(mode)
            try:
                two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
                _, byte = fused(sc.shape, sc.si, sc.ray, q.lights[k], spp=SPP, return_visibility=True)
            finally:
                sc.shape.set_ray_coherence(old)
            assert np.array_equal(q.vis[k], two), (lname, mode, int((q.vis[k] != two).sum()))
            assert np.array_equal(_np(byte), (q.byte >> k) & 1), (lname, mode)
        # (c) the oracle's ray_test on those rays
        r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
        occ = np.zeros(sc.n, bool)
        occ[tr] = sc.field.ray_test(r7[:, tr]).astype(bool)
        assert np.array_equal(q.vis[k], tr & ~occ), (lname, int((q.vis[k] != (tr & ~occ)).sum()))
        if row == "spot" and RS.in_bound(sc, L.to_world[:, 3]):                       # the end of the ray decides the answer
            far = r7[:, tr].copy()
            far[6] = np.inf
            ended += int(tr.sum())
            changed += int((sc.field.ray_test(far).astype(bool) != occ[tr]).sum())
        # (a) the rays against the restatement
        sure = ~q.unsure[k]
        assert np.array_equal(tr[sure], q.traced[k][sure]), lname
        ro, rw, rmaxt, _ = M.rays(L, rec["p"], rec["n"], rec["sh_n"], rec["d"], rec["t"])
        both = tr & q.traced[k]
        assert not o[:, ~tr].any() and not d[:, ~tr].any() and (maxt[~tr] == -1).all(), lname
        assert not q.val[k][~q.vis[k]].any(), lname                                  # exactly 0 where the bit is clear
        if not both.any():
            assert lname == "below" and not q.vis[k].any()
            continue
        worst["o"] = max(worst["o"], np.abs(o - ro)[:, both].max())
        if row == "directional":
            lf = M.unit(L)[0].astype(np.float32)
            assert np.array_equal(d[:, tr], np.repeat(lf[:, None], int(tr.sum()), 1)), lname   # bitwise float32(l)
            assert np.isinf(maxt[tr]).all(), lname
        else:
            worst["d"] = max(worst["d"], np.abs(d - rw)[:, both].max())
            worst["maxt"] = max(worst["maxt"], (np.abs(maxt - rmaxt)[both] / rmaxt[both].max()).max())
            assert np.isfinite(maxt[tr]).all(), lname
    print(row, name, "worst ray error: origin %.3g / 1e-6, direction %.3g / 2e-6, maxt %.3g / 1e-5 (relative)" % (worst["o"], worst["d"], worst["maxt"]),
          "| rays that end inside the bound", ended, "of which +inf changes the oracle's answer on", changed)
    assert worst["o"] <= 1e-6 and worst["d"] <= 2e-6 and worst["maxt"] <= 1e-5, worst
    if row == "spot":
        assert ended >= 100 and changed >= 10, (ended, changed)


# ---- (d), (e) ----------------------------------------------------------------------------------------------------------
def _leaf(hf, sc, sh_n=None, p=None):
    si = hf.SurfaceInteraction3f()
    si.n, si.t = sc.si.n.detach(), sc.si.t.detach()
    si.p = sc.si.p.detach().clone().requires_grad_(True) if p is None else p
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True) if sh_n is None else sh_n)
    return si


def _flat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors])


@pytest.mark.parametrize("row,name,face_normals", TRIPLES)
def test_values_gradients_and_tangents_against_the_restatement_and_the_transposition_gap(hf, oracle, row, name, face_normals):
    q = _rigged(hf, oracle, row, name, face_normals)
    sc, M, x, K = q.sc, q.M, q.x, q.K
    fused, _ = _lighting(hf, row)
    rec = sc.np
    spot = row == "spot"
    pix = q.sure.reshape(-1, SPP).all(1)
    gi = np.where(q.okpix, x.gi, 0).astype(np.float32)
    gv = np.where(q.okl, x.gv, 0).astype(np.float32)
    geo = (rec["p"], rec["sh_n"]) if spot else (rec["sh_n"],)
    tol = RS.TOL[row]
    worst = {k: 0.0 for k in tol}
    for weighted in (True, False):
        wa = x.w if weighted else None
        # ---- the GPU: backward and forward_ad through the public function
        si = _leaf(hf, sc)
        wt = _cu(x.w).requires_grad_(True) if weighted else None
        par = [[_f64(v).requires_grad_(True) for v in _numbers(row, L)] for L in q.ref]
        img, val, vis = fused(sc.shape, si, sc.ray, _lights(hf, row, q.ref, par), albedo=M.ALBEDO, spp=SPP, weight=wt, return_value=True,
                              return_visibility=True)
        assert np.array_equal(_np(vis), q.byte)
        ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
        got = types.SimpleNamespace(image=_np(img.detach()).copy(), value=_np(val.detach()).copy(), gn=_np(si.sh_frame.n.grad),
                                    gw=_np(wt.grad) if weighted else None)
        rows_ = _np(torch.stack([_flat([t.grad for t in p]) for p in par]))
        assert rows_.shape == (K, M.PARAMS)
        if spot:
            got.gp, got.g15 = _np(si.p.grad), rows_
        else:
            got.g4 = rows_
            assert si.p.grad is None or not bool(si.p.grad.any())                   # a directional light has no position
        with fwAD.dual_level():
            sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)),
                        fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)) if spot else sc.si.p.detach())
            dual, at = [], 0
            for k, L in enumerate(q.ref):
                ts, at = [], 0
                for v in _numbers(row, L):
                    v = _f64(v)
                    ts.append(fwAD.make_dual(v, _f64(x.dl[k, at:at + max(1, v.numel())]).reshape(v.shape)))
                    at += max(1, v.numel())
                dual.append(ts)
            out = fused(sc.shape, sid, sc.ray, _lights(hf, row, q.ref, dual), albedo=M.ALBEDO, spp=SPP,
                        weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)) if weighted else None, return_value=True)
            got.dimage, got.dvalue = (_np(fwAD.unpack_dual(o).tangent).copy() for o in out)
        # ---- the restatement fed with the GPU's records and visibility
        ref = types.SimpleNamespace()
        ref.image, ref.value = M.forward(q.ref, *geo, wa, M.ALBEDO, q.vis, SPP)
        kw = dict(dn=x.dn, dw=x.dw if weighted else None, d_lights=x.dl)
        if spot:
            kw["dp"] = x.dp
        ref.dimage, ref.dvalue = M.tangent(q.ref, *geo, wa, M.ALBEDO, q.vis, SPP, **kw)
        g = M.adjoint(q.ref, *geo, wa, M.ALBEDO, q.vis, SPP, gi, gv)
        ref.gn, ref.gw = g.gn, g.gw if weighted else None
        if spot:
            ref.gp, ref.g15 = g.gp, g.g15
        else:
            ref.g4 = g.g4
        full = (got.dimage.copy(), got.dvalue.copy())
        for ns in (got, ref):                               # (samples that rounding may decide, lanes at the kink)
            ns.value, ns.image = np.where(q.sure[None], ns.value, 0.0), np.where(pix[None], ns.image, 0.0)
            ns.dvalue, ns.dimage = np.where(q.okl, ns.dvalue, 0.0), np.where(q.okpix, ns.dimage, 0.0)
        dark = ~q.vis.any(0)
        assert not got.gn[:, dark].any() and not got.dvalue[~q.vis].any() and not got.value[~q.vis].any()
        assert ref.value.max() > 0.1 and np.abs(ref.gn).max() > 0 and (np.abs(rows_).max(1) > 0).sum() >= K - 1
        err = M.errors(got, ref)
        print(row, name, "weighted" if weighted else "unweighted", {k: "%.3g" % v for k, v in err.items()})
        for k, v in err.items():
            worst[k] = max(worst[k], v)
        if weighted:
            # the transposition gap on the device: both sides float32 results added up in float64
            rhs = [(got.gn, x.dn), (got.gw, x.dw), (rows_, x.dl)] + ([(got.gp, x.dp)] if spot else [])
            gap = transposition_gap(((full[0], gi), (full[1], gv)), rhs)
            size = np.linalg.norm(full[1]) * np.linalg.norm(gv) + np.linalg.norm(full[0]) * np.linalg.norm(gi)
            bound = (tol["dvalue"] + tol["grad_p" if spot else "grad_sh_n"]) * size
            print(row, name, "transposition gap %.3g / %.3g" % (gap, bound))
            assert size > 0 and gap <= bound, (gap, bound)
    print(row, name, "worst", {k: "%.3g / %.3g" % (worst[k], tol[k]) for k in tol})
    for k in tol:
        assert worst[k] <= tol[k], (row, name, k, worst[k], tol[k])


# ---- (f) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
@pytest.mark.parametrize("row", RS.ROWS)
def test_chain_to_the_heights(hf, oracle, row, name, face_normals):
    """row -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n (and grad_p) fed with the GPU's
    records and visibility, carried to the heights by the oracle's adjoint under the scene's to_world and flip_normals (flat
    shading) or by hf_adjoint, which tests/test_gpu_smooth_shading.py holds against float64 (smooth).  Bound: the one of
    the rows' own chain tests"""
    q = _rigged(hf, oracle, row, name, face_normals)
    sc, M = q.sc, q.M
    fused, _ = _lighting(hf, row)
    gi = np.where(q.okpix, q.x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = fused(shape, si, sc.ray, q.lights, albedo=M.ALBEDO, spp=SPP, return_visibility=True)
    assert np.array_equal(_np(vis), q.byte)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    geo = (_np(si.p), _np(si.sh_frame.n)) if row == "spot" else (_np(si.sh_frame.n),)
    g = M.adjoint(q.ref, *geo, None, M.ALBEDO, q.vis, SPP, gi)
    gp = g.gp if row == "spot" else np.zeros_like(g.gn)
    gh = _to_heights(hf, oracle, sc, shape, g.gn, gp, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print(row, name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, RS.CHAIN), "norm", np.linalg.norm(gh))
    assert got.shape == (sc.H, sc.W) and np.linalg.norm(gh) > 0 and err <= RS.CHAIN, err


# ---- the caustic row: rays that end at the receiver, the oblique view ---------------------------------------------------


CTOL = RS.TOL["caustic"]
CHAIN_FILM = 96            # the film of the chain test: the carried receivers' positions reach 76 pixels
_CAUSTIC = {}


def _caustic(hf, oracle, name, face_normals):
    """{(eta, plane): run} of a scene, once: the restatement's rays and masks on the GPU's records, the GPU's rays, the
    two-call answer and the fused outputs, and (g) the conditions of tests/test_row_scenes.py on the GPU's own records and
    visibility, asserted before anything is compared"""
    key = (name, face_normals)
    if key not in _CAUSTIC:
        sc = _scene(hf, oracle, name, "oblique", face_normals)
        runs = {}
        for eta, plane in RS.caustic_runs(face_normals):
            rcv3 = RS.caustic_receiver(sc, plane)
            rcv = hf.Receiver(*(tuple(float(c) for c in v) for v in rcv3))
            pos, value, vis = hf.caustic_lighting(sc.shape, sc.si, sc.ray, rcv, eta=eta, power=1.0, return_visibility=True)
            r = RS.caustic_run(sc, sc.np, sc.np["d"], sc.np["t"], eta, plane, sc.field, vis=_np(vis).astype(bool))
            r.rcv, r.pos, r.value, r.byte = rcv, pos, value, vis
            r.rays = hf.caustic_rays(sc.si, sc.ray, rcv, eta)
            r.occluded = sc.shape.ray_test(r.rays)
            print("caustic", name, "face" if face_normals else "smooth", "eta %.3f %s" % (eta, plane), r.counts)
            runs[(eta, plane)] = r
        RS.caustic_conditions(sc, runs)                                            # (g)
        _CAUSTIC[key] = (sc, runs)
    return _CAUSTIC[key]


def _receiver_rays_checks(hf, sc, runs, name, label, pos_tol):
    """(a), (b), (c) of the rows whose rays end at a receiver (caustic, refract): runs as _caustic() builds them; pos_tol:
    the row's tolerance of a landing position, in the units of its receiver's film"""
    for (eta, plane), r in runs.items():
        o, d, maxt = _np(r.rays.o), _np(r.rays.d), _np(r.rays.maxt)
        tr = maxt >= 0
        # (b) the two-call sequence, bit for bit
        two = (r.rays.maxt >= 0) & ~r.occluded
        assert torch.equal(r.byte.bool(), two), (eta, plane, int((r.byte.bool() != two).sum()))
        # (c) the oracle's ray_test on those rays, exactly; and what a walk that ignored the ray's end would answer
        r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
        occ = sc.field.ray_test(r7[:, tr]).astype(bool)
        assert np.array_equal(r.vis[tr], ~occ) and not r.vis[~tr].any(), (eta, plane, int((r.vis[tr] == occ).sum()))
        r7[6] = np.inf
        changed = int((sc.field.ray_test(r7[:, tr]).astype(bool) != occ).sum())
        unbounded = hf.Ray3f(r.rays.o, r.rays.d, torch.where(r.rays.maxt >= 0, torch.full_like(r.rays.maxt, math.inf), r.rays.maxt))
        assert int((sc.shape.ray_test(unbounded) != r.occluded).sum()) == changed
        assert changed >= (RS.FLOOR_CHANGED if plane == "cut" else 0), (eta, plane, changed)
        lit = r.byte.bool()
        assert bool((r.value[~lit] == 0).all()) and bool((r.pos[:, ~lit] == CR.NOWHERE).all()) and bool((r.value[lit] > 0).all())
        # (a) the rays against the restatement: the direction within the float32 error of dpos, the origin within 1e-6 and
        # maxt so that the landing point moves by at most TOL[pos] pixels, as in tests/test_gpu_caustic.py -- the last on
        # the lanes with |<wo, N>| and cos_theta_t of at least CAUSTIC_WELL.  On the others (a ray near the critical angle
        # that grazes the receiver has maxt = 169 with a float32 error of 0.07 in the restatement) maxt is held relative to
        # itself; on all of them the ray's END lies on the receiver's plane, at four times the restatement's own error
        assert np.array_equal(tr[r.sure], r.traced[r.sure]), (eta, plane)
        assert np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
        both = tr & r.traced
        both = both & r.sure
        with np.errstate(invalid="ignore"):
            well = both & (np.abs(r.v.b) >= RS.CAUSTIC_WELL) & (r.v.ct2 >= RS.CAUSTIC_WELL ** 2)
        ill = both & ~well
        per_unit = max(np.linalg.norm(r.rcv3[1]), np.linalg.norm(r.rcv3[2]))       # pixels per world unit
        err = {"unit": np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max(), "d": np.abs(d - r.wo)[:, both].max(),
               "o": np.abs(o - r.o)[:, both].max(), "maxt_well": np.abs(maxt - r.maxt)[well].max(),
               "maxt_ill": (np.abs(maxt - r.maxt)[ill] / r.maxt[ill]).max(initial=0.0),
               "end": RS.caustic_end(r, d.astype(np.float64), maxt.astype(np.float64))[both].max()}
        print(label, name, "eta %.3f %s" % (eta, plane), "changed by +inf", changed, "| ray errors: direction %.3g / %.3g, origin %.3g / 1e-6, "
              "maxt on %d well-conditioned lanes %.3g / %.3g, on the other %d %.3g / %.3g (relative), end %.3g / %.3g"
              % (err["d"], CTOL["dpos"], err["o"], well.sum(), err["maxt_well"], pos_tol / per_unit, ill.sum(), err["maxt_ill"],
                 CTOL["maxt"], err["end"], CTOL["end"]))
        assert both.sum() >= 300 and err["unit"] <= 1e-5 and err["d"] <= CTOL["dpos"] and err["o"] <= 1e-6, err
        assert well.sum() >= 0.9 * both.sum() and err["maxt_well"] <= pos_tol / per_unit, err
        assert err["maxt_ill"] <= CTOL["maxt"] and err["end"] <= CTOL["end"], err


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_caustic_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals):
    sc, runs = _caustic(hf, oracle, name, face_normals)
    _receiver_rays_checks(hf, sc, runs, name, "caustic", CTOL["pos"])


def _caustic_leaf(hf, sc):
    si = hf.SurfaceInteraction3f()
    si.p, si.n, si.t = sc.si.p.detach().clone().requires_grad_(True), sc.si.n.detach(), sc.si.t.detach()
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True))
    return si


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_caustic_values_adjoint_and_tangent_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    sc, runs = _caustic(hf, oracle, name, face_normals)
    w, gpos, gv, dn, dp, dw = RS.caustic_inputs(sc.n)
    worst = {k: 0.0 for k in CTOL if k not in ("maxt", "end")}
    for (eta, plane), r in runs.items():
        vis = r.vis
        keep = r.sure & (vis == (r.traced & vis))               # (a lane the GPU traced and the restatement did not is not sure)
        assert (~keep).mean() <= RS.UNSURE_CAP
        args = (*r.a, None, w, eta, 1.0, r.rref, vis)
        si = _caustic_leaf(hf, sc)
        wt = _cu(w).requires_grad_(True)
        pos, value, vis2 = hf.caustic_lighting(sc.shape, si, sc.ray, r.rcv, eta=eta, power=1.0, weight=wt, return_visibility=True)
        assert torch.equal(vis2, r.byte) and torch.equal(pos, r.pos)
        rp, rv = CR.forward(*args)
        err = {"pos": np.abs(_np(pos) - rp)[:, keep].max(), "value": np.abs(_np(value) - rv)[keep].max()}
        assert vis[keep].sum() >= 300 and rv[keep].max() > 0.5
        ((pos * _cu(gpos)).sum() + (value * _cu(gv)).sum()).backward()
        gm, gp, gw = CR.adjoint(*args, gpos, gv)
        got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad), "grad_weight": _np(wt.grad)}
        for k, ref in (("grad_sh_n", gm), ("grad_p", gp), ("grad_weight", gw)):
            assert not got[k][..., ~vis].any()                                      # exact zeros where vis = 0
            err[k] = _rel(got[k][..., keep], ref[..., keep])
        with fwAD.dual_level():
            sd = hf.SurfaceInteraction3f()
            sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), _cu(dp)), sc.si.n.detach(), sc.si.t.detach()
            sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(dn)))
            tp, tv = hf.caustic_lighting(sc.shape, sd, sc.ray, r.rcv, eta=eta, power=1.0, weight=fwAD.make_dual(_cu(w), _cu(dw)))
            tpos, tval = _np(fwAD.unpack_dual(tp).tangent).copy(), _np(fwAD.unpack_dual(tv).tangent).copy()
        dpos, dval = CR.tangent(*args, dn, dp, dw)
        assert not tpos[:, ~vis].any() and not tval[~vis].any()
        err["dpos"], err["dvalue"] = _rel(tpos[:, keep], dpos[:, keep]), _rel(tval[keep], dval[keep])
        gap = transposition_gap(((tpos, gpos), (tval, gv)), ((got["grad_sh_n"], dn), (got["grad_p"], dp), (got["grad_weight"], dw)))
        size = np.linalg.norm(dpos) * np.linalg.norm(gpos) + np.linalg.norm(dval) * np.linalg.norm(gv)
        print("caustic", name, "eta %.3f %s" % (eta, plane), {k: "%.3g" % v for k, v in err.items()}, "transposition %.3g / %.3g"
              % (gap / size, CTOL["dpos"] + CTOL["grad_sh_n"]))
        assert gap <= (CTOL["dpos"] + CTOL["grad_sh_n"]) * size, gap
        for k in err:
            worst[k] = max(worst[k], err[k])
    print("caustic", name, "worst", {k: "%.3g / %.3g" % (worst[k], CTOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= CTOL[k], (name, k, worst[k], CTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_caustic_chain_to_the_heights(hf, oracle, name, face_normals):
    """caustic_film -> loss -> backward() -> shape.heightfield.grad against the restatement's chain, as
    tests/test_gpu_caustic.py has it: film_ref's adjoint of the accumulated plane over the filter's mass, the restatement's
    grad_sh_n and grad_p (fed with the GPU's records and visibility), carried to the heights by the oracle's adjoint under
    the scene's to_world and flip_normals (flat shading) or by hf_adjoint (smooth).  eta 1 / 1.33, the far receiver.
    Bound: that test's: four times the float32 error of grad_sh_n + 1e-5"""
    sc, runs = _caustic(hf, oracle, name, face_normals)
    eta = RS.CAUSTIC_ETAS[1]
    r = runs[(eta, "far")]
    F = CHAIN_FILM
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    pos, value, vis = hf.caustic_lighting(shape, si, sc.ray, r.rcv, eta=eta, power=0.5, return_visibility=True)
    assert torch.equal(vis, r.byte)
    keep = r.sure & (r.vis == (r.traced & r.vis))
    value = value * _cu(keep.astype(np.float32))                                     # (lanes that rounding may decide deposit nothing)
    film = hf.caustic_film(pos, value, F, F)
    gi = np.random.default_rng(11).normal(size=F * F).astype(np.float32)
    (film * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(x) for x in (si.p, si.n, si.sh_frame.n, sc.ray.d, si.t))
    rp, rv = CR.forward(*a, None, keep.astype(np.float64), eta, 0.5, r.rref, r.vis)
    inside = r.vis & keep & (np.abs(rp - F / 2).max(0) < F / 2 - 2)
    assert inside.sum() >= 300, inside.sum()
    ref_film = film_ref.forward(rv[None], None, rp, F, F, 0.5)[0][0] / CR.filter_mass(0.5)
    assert np.abs(_np(film) - ref_film).max() <= 1e-4 * np.abs(ref_film).max()
    gvv, _, gpos = film_ref.adjoint(rv[None], None, rp, F, F, 0.5, (gi / CR.filter_mass(0.5))[None])
    gm, gp, _ = CR.adjoint(*a, None, keep.astype(np.float64), eta, 0.5, r.rref, r.vis, gpos, gvv[0])
    gh = _to_heights(hf, oracle, sc, shape, gm, gp, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("caustic", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, CTOL["grad_sh_n"] + 1e-5),
          "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= CTOL["grad_sh_n"] + 1e-5, err


# ---- the rect row: rays that end on the lamp, the steep view ---------------------------------------------------------------

RTOL = RS.TOL["rect"]
_RECT = {}


def _lamp(hf, lm, tex=None):
    return hf.RectLight(lm.center, lm.ex, lm.ey, lm.radiance, texture=tex)


def _rect(hf, oracle, name, face_normals):
    """{lamp: run} of a scene, once: the fused launch's 8 visibility bits of every sample, the restatement's draws, masks and
    rays on the GPU's records, and (g) the conditions of tests/test_row_scenes.py on the GPU's own records and bits"""
    key = (name, face_normals)
    if key not in _RECT:
        sc = _scene(hf, oracle, name, "steep", face_normals)
        runs = {}
        for lname in RS.RECT_LAMPS:
            light = _lamp(hf, RS.rect_lamp(sc, lname))
            _, vis = hf.rect_lighting(sc.shape, sc.si, sc.ray, light, albedo=AR.ALBEDO, spp=SPP, num_rays=RS.RECT_K, seed=RS.RECT_SEED,
                                      return_visibility=True)
            words = _np(vis).view(np.uint32).copy()
            r = RS.rect_run(sc, sc.np, sc.np["d"], sc.np["t"], lname, sc.field, bits=AR.unpack(words, RS.RECT_K))
            r.light, r.words = light, words
            print("rect", name, "face" if face_normals else "smooth", lname, r.counts)
            runs[lname] = r
        RS.rect_conditions(sc, runs)                                               # (g)
        _RECT[key] = (sc, runs)
    return _RECT[key]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_rect_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals):
    sc, runs = _rect(hf, oracle, name, face_normals)
    for lname, r in runs.items():
        assert not (r.words >> RS.RECT_K).any()                                      # no bit at or above num_rays
        assert not r.bits[:, ~r.eligible & r.sure].any()
        worst = {"o": 0.0, "d": 0.0, "maxt": 0.0}
        ended = changed = 0
        for k in range(RS.RECT_K):
            ray = hf.rect_rays(sc.si, sc.ray, r.light, k, seed=RS.RECT_SEED)
            o, d, maxt = _np(ray.o), _np(ray.d), _np(ray.maxt)
            tr = maxt >= 0
            two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
            assert np.array_equal(r.bits[k], two), (lname, k, int((r.bits[k] != two).sum()))                       # (b)
            r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
            occ = np.zeros(sc.n, bool)
            occ[tr] = sc.field.ray_test(r7[:, tr]).astype(bool)
            assert np.array_equal(r.bits[k], tr & ~occ), (lname, k, int((r.bits[k] != (tr & ~occ)).sum()))          # (c)
            inside = tr & r.ends_inside[k]
            far = r7[:, inside].copy()
            far[6] = np.inf
            ended += int(inside.sum())
            changed += int((sc.field.ray_test(far).astype(bool) != occ[inside]).sum())
            assert np.array_equal(tr[r.sure_k[k]], r.traced[k][r.sure_k[k]]), (lname, k)                            # (a)
            ro, rw, rmaxt = r.rays[k]
            both = tr & r.traced[k]
            worst["o"] = max(worst["o"], np.abs(o - ro)[:, both].max())
            worst["d"] = max(worst["d"], np.abs(d - rw)[:, both].max())
            worst["maxt"] = max(worst["maxt"], np.abs(maxt - rmaxt)[both].max() / rmaxt[both].max())
            assert not o[:, ~tr].any() and not d[:, ~tr].any() and (maxt[~tr] == -1).all()
        print("rect", name, lname, "worst ray error: origin %.3g / 1e-6, direction %.3g / 2e-6, maxt %.3g / 1e-5 (relative)"
              % (worst["o"], worst["d"], worst["maxt"]), "| rays that end inside the bound", ended, "of which +inf changes the oracle's answer on", changed)
        assert worst["o"] <= 1e-6 and worst["d"] <= 2e-6 and worst["maxt"] <= 1e-5, worst          # tests/test_gpu_rect.py's bounds
        if lname == "side":
            assert ended >= 100 and changed >= RS.FLOOR_CHANGED, (ended, changed)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_rect_values_adjoint_and_tangent_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    sc, runs = _rect(hf, oracle, name, face_normals)
    x = AR.inputs(sc.n, SPP, RS.RECT_TEX[::-1])
    smooth = AR.textures(*RS.RECT_TEX)["smooth"]
    worst = {k: 0.0 for k in RTOL}
    kw = dict(albedo=AR.ALBEDO, num_rays=RS.RECT_K, seed=RS.RECT_SEED)
    for lname, r in runs.items():
        sure, pix = r.sure, r.sure.reshape(-1, SPP).all(1)
        assert (~sure).mean() <= RS.UNSURE_CAP
        for tex in (None, smooth):
            ref = RS.rect_evaluate(r, sc.np, sc.np["d"], sc.np["t"], x, tex)
            si, wt = _leaf(hf, sc), _cu(x.w).requires_grad_(True)
            td = _cu(tex).requires_grad_(True) if tex is not None else None
            img, vis = hf.rect_lighting(sc.shape, si, sc.ray, _lamp(hf, r.lm, td), weight=wt, spp=SPP, return_visibility=True, **kw)
            assert np.array_equal(_np(vis).view(np.uint32), r.words)
            (img * _cu(x.gi)).sum().backward()
            got = {"image": _np(img.detach()), "grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad), "grad_weight": _np(wt.grad),
                   "grad_tex": _np(td.grad) if tex is not None else None}
            for k in ("grad_sh_n", "grad_p", "grad_weight"):
                assert not got[k][..., ~r.eligible & sure].any() and np.linalg.norm(ref[k]) > 0     # exact zeros where nothing is shaded
            # the per-sample values: spp = 1, the image is the wavefront
            got["value"] = _np(hf.rect_lighting(sc.shape, sc.si, sc.ray, _lamp(hf, r.lm, None if tex is None else _cu(tex)), weight=_cu(x.w),
                                                spp=1, **kw))
            assert not got["value"][~r.eligible & sure].any() and ref["value"].max() > 0.2
            with fwAD.dual_level():
                sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
                tdd = fwAD.make_dual(_cu(tex), _cu(x.dtex)) if tex is not None else None
                ti = hf.rect_lighting(sc.shape, sid, sc.ray, _lamp(hf, r.lm, tdd), weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), spp=SPP, **kw)
                got["dimage"] = _np(fwAD.unpack_dual(ti).tangent).copy()
            err = RS.rect_errors(got, ref, sure, pix)
            rhs = [(got["grad_sh_n"], x.dn), (got["grad_p"], x.dp), (got["grad_weight"], x.dw)] + ([(got["grad_tex"], x.dtex)] if tex is not None else [])
            gap = transposition_gap(((got["dimage"], x.gi),), rhs)
            size = np.linalg.norm(ref["dimage"]) * np.linalg.norm(x.gi)
            print("rect", name, lname, "textured" if tex is not None else "plain", {k: "%.3g" % v for k, v in err.items()},
                  "transposition %.3g / %.3g" % (gap / size, RTOL["dimage"] + RTOL["grad_p"]))
            assert gap <= (RTOL["dimage"] + RTOL["grad_p"]) * size, (gap, size)
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("rect", name, "worst", {k: "%.3g / %.3g" % (worst[k], RTOL[k]) for k in RTOL})
    for k in RTOL:
        assert worst[k] <= RTOL[k], (name, k, worst[k], RTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_rect_chain_to_the_heights(hf, oracle, name, face_normals):
    """rect_lighting under `side` -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n and
    grad_p (fed with the GPU's records and bits), carried to the heights by the oracle's adjoint under the scene's to_world
    and flip_normals (flat shading) or by hf_adjoint (smooth).  Bound: that of tests/test_gpu_rect.py's chain: four times
    the float32 error of grad_p + 1e-5"""
    sc, runs = _rect(hf, oracle, name, face_normals)
    r = runs["side"]
    x = AR.inputs(sc.n, SPP, RS.RECT_TEX[::-1])
    gi = np.where(r.sure.reshape(-1, SPP).all(1), x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.rect_lighting(shape, si, sc.ray, r.light, albedo=AR.ALBEDO, spp=SPP, num_rays=RS.RECT_K, seed=RS.RECT_SEED,
                                return_visibility=True)
    assert np.array_equal(_np(vis).view(np.uint32), r.words)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    gn, gp, _, _ = AR.adjoint(_np(si.p), _np(si.sh_frame.n), sc.np["d"], _np(si.t), None, r.bits, r.ids, RS.RECT_SEED, r.lm, None,
                              AR.ALBEDO, SPP, gi)
    gh = _to_heights(hf, oracle, sc, shape, gn, gp, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("rect", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, RTOL["grad_p"] + 1e-5), "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= RTOL["grad_p"] + 1e-5, err


# ---- the projector row: rays that end at the projector, the steep view ----------------------------------------------------

PTOL = RS.TOL["projector"]
PTEX = PJ.textures(*PJ.TEX)["random"]
PWRAPS = {"clamp": PJ.CLAMP, "repeat": PJ.REPEAT}
_PROJ = {}


def _projector(hf, pr, tex=None, wrap="repeat", **kw):
    a = dict(to_world=pr.to_world, fov=pr.fov, scale=pr.scale)
    a.update(kw)
    return hf.Projector(a["to_world"], a["fov"], tex, scale=a["scale"], wrap=wrap, resolution=None if tex is not None else pr.res)


def _proj(hf, oracle, name, face_normals):
    """{projector: run} of a scene, once: the fused launch's visibility, the restatement's masks and rays on the GPU's records,
    and (g) the conditions of tests/test_row_scenes.py on the GPU's own records and visibility"""
    key = (name, face_normals)
    if key not in _PROJ:
        sc = _scene(hf, oracle, name, "steep", face_normals)
        runs = {}
        for pname in RS.PROJ_NAMES:
            proj = _projector(hf, RS.projector_of(sc, pname))
            _, vis = hf.projector_lighting(sc.shape, sc.si, sc.ray, proj, albedo=PJ.ALBEDO, spp=SPP, return_visibility=True)
            r = RS.projector_run(sc, sc.np, sc.np["d"], sc.np["t"], pname, sc.field, vis=_np(vis).astype(bool))
            r.proj = proj
            print("projector", name, "face" if face_normals else "smooth", pname, {k: round(v, 4) for k, v in r.counts.items()})
            runs[pname] = r
        RS.projector_conditions(sc, runs)                                          # (g)
        _PROJ[key] = (sc, runs)
    return _PROJ[key]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_projector_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals):
    sc, runs = _proj(hf, oracle, name, face_normals)
    for pname, r in runs.items():
        ray = hf.projector_rays(sc.si, sc.ray, r.proj)
        o, d, maxt = _np(ray.o), _np(ray.d), _np(ray.maxt)
        tr = maxt >= 0
        two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
        assert np.array_equal(r.vis, two), (pname, int((r.vis != two).sum()))                                    # (b)
        r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
        occ = np.zeros(sc.n, bool)
        occ[tr] = sc.field.ray_test(r7[:, tr]).astype(bool)
        assert np.array_equal(r.vis, tr & ~occ), (pname, int((r.vis != (tr & ~occ)).sum()))                       # (c)
        assert np.array_equal(tr[r.sure], r.traced[r.sure]) and not r.vis[~r.eligible & r.sure].any(), pname      # (a)
        both = tr & r.traced
        err = (np.abs(o - r.o)[:, both].max(), np.abs(d - r.w)[:, both].max(), np.abs(maxt - r.maxt)[both].max() / r.maxt[both].max())
        print("projector", name, pname, "ray errors: origin %.3g / 1e-6, direction %.3g / 2e-6, maxt %.3g / 1e-5 (relative)" % err)
        assert err[0] <= 1e-6 and err[1] <= 2e-6 and err[2] <= 1e-5, err             # tests/test_gpu_projector.py's bounds
        assert not o[:, ~tr].any() and not d[:, ~tr].any() and (maxt[~tr] == -1).all()
        # the texture and the wrap do not enter the visibility
        _, v2 = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, r.pr, _cu(PTEX), "clamp"), spp=SPP, return_visibility=True)
        assert np.array_equal(_np(v2).astype(bool), r.vis)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_projector_values_uv_gradients_and_tangents_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    """through the public function: backward() and forward_ad.  The lanes within BORDER of a cell border of the lookup and
    those that rounding may decide get no upstream gradient and their tangents are not compared (the row's own file clears
    their visibility instead, through the C ABI)"""
    sc, runs = _proj(hf, oracle, name, face_normals)
    x = PJ.inputs(sc.n, SPP, PJ.TEX[::-1])
    worst = {k: 0.0 for k in PTOL}
    for pname, r in runs.items():
        pr = r.pr
        okl = r.steady | (~r.vis & r.sure)
        okpix = okl.reshape(-1, SPP).all(1)
        assert (~okl).mean() <= 3 * RS.UNSURE_CAP, (~okl).mean()
        gi, gv = np.where(okpix, x.gi, 0).astype(np.float32), np.where(okl, x.gv, 0).astype(np.float32)
        for wrap, textured in RS.PROJ_VARIANTS:
            tex = PTEX if textured else None
            si, wt = _leaf(hf, sc), _cu(x.w).requires_grad_(True)
            td = _cu(PTEX).requires_grad_(True) if textured else None
            tw, fov, scale = (_f64(v).requires_grad_(True) for v in (pr.to_world, pr.fov, pr.scale))
            img, val, vis, uv = hf.projector_lighting(sc.shape, si, sc.ray, _projector(hf, pr, td, wrap, to_world=tw, fov=fov, scale=scale),
                                                      albedo=PJ.ALBEDO, spp=SPP, weight=wt, return_value=True, return_visibility=True,
                                                      return_uv=True)
            assert np.array_equal(_np(vis).astype(bool), r.vis) and not _np(val.detach())[~r.vis].any()
            ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
            got = types.SimpleNamespace(image=_np(img.detach()).copy(), value=_np(val.detach()).copy(), uv=_np(uv.detach()).copy(),
                                        gn=_np(si.sh_frame.n.grad), gp=_np(si.p.grad), gw=_np(wt.grad),
                                        gtex=_np(td.grad) if textured else None)
            got.g14 = np.concatenate([_np(tw.grad).reshape(-1), [float(fov.grad) if fov.grad is not None else 0.0, float(scale.grad)]])
            with fwAD.dual_level():
                sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
                dual = _projector(hf, pr, fwAD.make_dual(_cu(PTEX), _cu(x.dtex)) if textured else None, wrap,
                                  to_world=fwAD.make_dual(_f64(pr.to_world), _f64(x.dtw).reshape(3, 4)),
                                  fov=fwAD.make_dual(_f64(pr.fov), _f64(x.dfov)), scale=fwAD.make_dual(_f64(pr.scale), _f64(x.dscale)))
                ti, tv = hf.projector_lighting(sc.shape, sid, sc.ray, dual, albedo=PJ.ALBEDO, spp=SPP,
                                               weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), return_value=True)
                full = (_np(fwAD.unpack_dual(ti).tangent).copy(), _np(fwAD.unpack_dual(tv).tangent).copy())
            got.dimage, got.dvalue = full
            a = (pr, sc.np["p"], sc.np["sh_n"], x.w, tex, PWRAPS[wrap], PJ.ALBEDO, r.vis, SPP)
            ref = types.SimpleNamespace()
            ref.image, ref.value, ref.uv = PJ.forward(*a)
            ref.dimage, ref.dvalue = PJ.tangent(*a, dn=x.dn, dp=x.dp, dw=x.dw, dtex=x.dtex if textured else None, d_to_world=x.dtw,
                                                d_fov=x.dfov, d_scale=x.dscale)
            g = PJ.adjoint(*a, grad_image=gi, grad_value=gv)
            ref.gn, ref.gp, ref.gw, ref.gtex, ref.g14 = g.gn, g.gp, g.gw, g.gtex, g.g14
            for ns in (got, ref):                           # (samples that rounding may decide, lanes at a cell border)
                ns.value, ns.image = np.where(r.sure, ns.value, 0.0), np.where(r.pix, ns.image, 0.0)
                ns.dvalue, ns.dimage = np.where(okl, ns.dvalue, 0.0), np.where(okpix, ns.dimage, 0.0)
            assert ref.value.max() > 0.05 and np.abs(np.delete(ref.g14, () if textured else 12)).min() > 0
            assert not got.gn[:, ~r.vis].any() and not got.gp[:, ~r.vis].any() and not full[1][~r.vis].any()
            assert not got.uv[:, sc.hit & ~r.lanes].any()                           # zeros behind the projector
            err = PJ.errors(got, ref, r.lanes & r.sure)
            rhs = [(got.gn, x.dn), (got.gp, x.dp), (got.gw, x.dw), (got.g14[:12], x.dtw), (got.g14[12], x.dfov), (got.g14[13], x.dscale)]
            gap = transposition_gap(((full[0], gi), (full[1], gv)), rhs + ([(got.gtex, x.dtex)] if textured else []))
            size = np.linalg.norm(full[1]) * np.linalg.norm(gv) + np.linalg.norm(full[0]) * np.linalg.norm(gi)
            print("projector", name, pname, wrap, textured, {k: "%.3g" % v for k, v in err.items()}, "transposition %.3g / %.3g"
                  % (gap / size, PTOL["dvalue"] + PTOL["grad_p"]))
            assert size > 0 and gap <= (PTOL["dvalue"] + PTOL["grad_p"]) * size, (gap, size)
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("projector", name, "worst", {k: "%.3g / %.3g" % (worst[k], PTOL[k]) for k in PTOL})
    for k in PTOL:
        assert worst[k] <= PTOL[k], (name, k, worst[k], PTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_projector_chain_to_the_heights(hf, oracle, name, face_normals):
    """projector_lighting under `side` with the texture -> loss -> backward() -> shape.heightfield.grad against the
    restatement's grad_sh_n and grad_p (fed with the GPU's records and visibility), carried to the heights by the oracle's
    adjoint under the scene's to_world and flip_normals (flat shading) or by hf_adjoint (smooth).  Bound: that of
    tests/test_gpu_projector.py's chain: four times the float32 error of grad_p + 1e-5"""
    sc, runs = _proj(hf, oracle, name, face_normals)
    r = runs["side"]
    x = PJ.inputs(sc.n, SPP, PJ.TEX[::-1])
    keep = r.steady | (~r.vis & r.sure)
    gi = np.where(keep.reshape(-1, SPP).all(1), x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.projector_lighting(shape, si, sc.ray, _projector(hf, r.pr, _cu(PTEX), "repeat"), albedo=PJ.ALBEDO, spp=SPP,
                                     return_visibility=True)
    assert np.array_equal(_np(vis).astype(bool), r.vis)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = PJ.adjoint(r.pr, _np(si.p), _np(si.sh_frame.n), None, PTEX, PJ.REPEAT, PJ.ALBEDO, r.vis, SPP, gi)
    gh = _to_heights(hf, oracle, sc, shape, g.gn, g.gp, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("projector", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, PTOL["grad_p"] + 1e-5), "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= PTOL["grad_p"] + 1e-5, err


# ---- the reflect row: rays with maxt = inf, the oblique view -----------------------------------------------------------------

FTOL = RS.TOL["reflect"]
_REFLECT = {}


def _reflect(hf, oracle, name, face_normals):
    """the reflected rays, the two-call answer and the fused visibility of a scene, once; (g) the conditions of
    tests/test_row_scenes.py on the GPU's own records and visibility"""
    key = (name, face_normals)
    if key not in _REFLECT:
        sc = _scene(hf, oracle, name, "oblique", face_normals)
        env, _, _ = envmap(hf, RS.REFLECT_MAPS, RS.reflect_rots(), "gradient", "identity")
        _, vis = hf.reflection_lighting(sc.shape, sc.si, sc.ray, env, spp=SPP, return_visibility=True)
        r = RS.reflect_run(sc, sc.np, sc.np["d"], sc.np["t"], sc.field, vis=_np(vis).astype(bool))
        r.byte = vis
        r.rays = hf.reflection_rays(sc.si, sc.ray)
        r.occluded = sc.shape.ray_test(r.rays)
        print("reflect", name, "face" if face_normals else "smooth", r.counts)
        RS.reflect_conditions(sc, r)                                               # (g)
        _REFLECT[key] = (sc, r)
    return _REFLECT[key]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_reflect_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals):
    sc, r = _reflect(hf, oracle, name, face_normals)
    o, d, maxt = _np(r.rays.o), _np(r.rays.d), _np(r.rays.maxt)
    tr = maxt >= 0
    two = (r.rays.maxt >= 0) & ~r.occluded
    assert torch.equal(r.byte.bool(), two), int((r.byte.bool() != two).sum())                                    # (b)
    r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
    occ = sc.field.ray_test(r7[:, tr]).astype(bool)
    assert np.array_equal(r.vis[tr], ~occ) and not r.vis[~tr].any(), int((r.vis[tr] == occ).sum())                # (c)
    assert np.array_equal(tr[r.sure], r.traced[r.sure])                                                          # (a)
    assert np.all(maxt[tr] == np.inf) and np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
    both = tr & r.traced
    err = (np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max(), np.abs(d - r.wr)[:, both].max(), np.abs(o - r.o)[:, both].max())
    print("reflect", name, "ray errors: unit %.3g / 1e-5, direction %.3g / 1e-6, origin %.3g / 1e-6" % err)
    assert both.sum() >= 1000 and err[0] <= 1e-5 and err[1] <= 1e-6 and err[2] <= 1e-6, err    # tests/test_gpu_reflect.py's bounds


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_reflect_values_adjoint_and_tangent_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    sc, r = _reflect(hf, oracle, name, face_normals)
    worst = {k: 0.0 for k in FTOL}
    for mname, rname in RS.REFLECT_PAIRS:
        for eta in RS.REFLECT_ETAS:
            env, full, rot = envmap(hf, RS.REFLECT_MAPS, RS.reflect_rots(), mname, rname, requires_grad=True)
            x = RS.reflect_inputs(sc.n, full.shape)
            w, gi, gv, dn, dw, dd = x
            keep = RS.reflect_keep(r, full, rot)
            assert float((r.vis & ~keep).mean()) <= RS.REFLECT_LEFT_OUT_CAP
            ref = RS.reflect_evaluate(r, eta, full, rot, x, keep)
            ref["grad_data"] = _fold(ref["grad_data"])
            si, wt = leaf_si(hf, sc), _cu(w).requires_grad_(True)
            img, val, vis = hf.reflection_lighting(sc.shape, si, sc.ray, env, eta=eta, spp=SPP, weight=wt, return_value=True,
                                                   return_visibility=True)
            assert torch.equal(vis, r.byte) and not _np(val.detach())[~r.vis].any()
            if eta == 0.0:                                                          # a mirror: value = weight * Envmap.eval(rays.d)
                lit = vis.bool()
                assert torch.equal(val.detach()[lit], (wt.detach() * env.eval(r.rays.d).detach())[lit])
            assert r.vis[keep].sum() >= 500 and ref["value"].max() > 0.01
            ((img * _cu(gi)).sum() + (val * _cu(gv)).sum()).backward()
            got = {"image": _np(img.detach()), "value": _np(val.detach()), "grad_sh_n": _np(si.sh_frame.n.grad), "grad_weight": _np(wt.grad),
                   "grad_data": _np(env.data.grad)}
            assert not got["grad_sh_n"][:, ~r.vis].any() and not got["grad_weight"][~r.vis].any()       # exact zeros where vis = 0
            with fwAD.dual_level():
                sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu((dn * keep).astype(np.float32))))
                envd = hf.Envmap(fwAD.make_dual(env.data.detach(), _cu(dd[:, :-1])), to_world=rot)
                ti, tv = hf.reflection_lighting(sc.shape, sd, sc.ray, envd, eta=eta, spp=SPP, weight=fwAD.make_dual(_cu(w), _cu(dw)),
                                                return_value=True)
                got["dimage"], got["dvalue"] = _np(fwAD.unpack_dual(ti).tangent).copy(), _np(fwAD.unpack_dual(tv).tangent).copy()
            assert not got["dvalue"][~r.vis].any()
            err = RS.reflect_errors(got, ref, keep, r.vis)
            gap = transposition_gap(((got["dimage"], gi), (got["dvalue"], gv)),
                                    ((got["grad_sh_n"], dn * keep), (got["grad_weight"], dw), (got["grad_data"], dd[:, :-1])))
            size = np.linalg.norm(ref["dimage"]) * np.linalg.norm(gi) + np.linalg.norm(ref["dvalue"]) * np.linalg.norm(gv)
            print("reflect", name, mname, rname, "eta", eta, {k: "%.3g" % v for k, v in err.items()}, "transposition %.3g / %.3g"
                  % (gap / size, FTOL["dvalue"] + FTOL["grad_sh_n"]))
            assert gap <= (FTOL["dvalue"] + FTOL["grad_sh_n"]) * size, (gap, size)
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("reflect", name, "worst", {k: "%.3g / %.3g" % (worst[k], FTOL[k]) for k in FTOL})
    for k in FTOL:
        assert worst[k] <= FTOL[k], (name, k, worst[k], FTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_reflect_chain_to_the_heights(hf, oracle, name, face_normals):
    """reflection_lighting (eta 1.5, the sun map rotated) -> loss -> backward() -> shape.heightfield.grad against the
    restatement's grad_sh_n (fed with the GPU's records and visibility; upstream gradients only on pixels all of whose samples
    are kept), carried to the heights by the oracle's adjoint under the scene's to_world and flip_normals (flat shading) or
    by hf_adjoint (smooth).  Bound: four times the float32 error of grad_sh_n + the 1e-5 of the sky row's chain"""
    sc, r = _reflect(hf, oracle, name, face_normals)
    env, full, rot = envmap(hf, RS.REFLECT_MAPS, RS.reflect_rots(), "sun", "rotated")
    _, gi, _, _, _, _ = RS.reflect_inputs(sc.n, full.shape)
    keep = RS.reflect_keep(r, full, rot) | ~r.vis
    gi = np.where(keep.reshape(-1, SPP).all(1), gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.reflection_lighting(shape, si, sc.ray, env, eta=1.5, spp=SPP, return_visibility=True)
    assert torch.equal(vis, r.byte)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    gm, _, _ = RF.adjoint(_np(si.n), _np(si.sh_frame.n), sc.np["d"], _np(si.t), None, None, 1.5, full, rot, r.vis, SPP, gi, None)
    gh = _to_heights(hf, oracle, sc, shape, gm, None, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("reflect", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, FTOL["grad_sh_n"] + 1e-5), "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= FTOL["grad_sh_n"] + 1e-5, err


# ---- the refract row: the caustic row's rays onto a textured receiver, the oblique view -----------------------------------
XTOL = RS.TOL["refract"]
XTEX = RR.textures(*RS.REFRACT_TEX)
XWRAPS = {"clamp": RR.CLAMP, "repeat": RR.REPEAT}
_REFRACT = {}


def _refract(hf, oracle, name, face_normals):
    """{(eta, plane): run} of a scene on the textured receivers, once: what _caustic() builds, with hf_caustic_lighting's
    outputs for that receiver, and (g) the conditions of tests/test_row_scenes.py on the GPU's own records and visibility"""
    key = (name, face_normals)
    if key not in _REFRACT:
        sc = _scene(hf, oracle, name, "oblique", face_normals)
        runs = {}
        for eta, plane in RS.caustic_runs(face_normals):
            rcv = hf.Receiver(*(tuple(float(c) for c in v) for v in RS.refract_receiver(sc, plane)))
            pos, value, vis = hf.caustic_lighting(sc.shape, sc.si, sc.ray, rcv, eta=eta, power=1.0, return_visibility=True)
            r = RS.refract_run(sc, sc.np, sc.np["d"], sc.np["t"], eta, plane, sc.field, vis=_np(vis).astype(bool))
            r.rcv, r.pos, r.value, r.byte = rcv, pos, value, vis
            r.rays = hf.caustic_rays(sc.si, sc.ray, rcv, eta)
            r.occluded = sc.shape.ray_test(r.rays)
            print("refract", name, "face" if face_normals else "smooth", "eta %.3f %s" % (eta, plane), r.counts)
            runs[(eta, plane)] = r
        RS.refract_conditions(sc, runs)                                            # (g)
        _REFRACT[key] = (sc, runs)
    return _REFRACT[key]


def _bitmap(hf, tname, wrap, requires_grad=False):
    data = _cu(XTEX[tname])
    return hf.Bitmap(data.requires_grad_(True) if requires_grad else data, wrap=wrap)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_refract_rays_visibility_and_positions_are_the_caustic_rows_and_the_oracles(hf, oracle, name, face_normals):
    """(a), (b), (c) on the textured receivers, and hf_refract_lighting's visibility and landing positions bit for bit
    hf_caustic_lighting's, for every variant"""
    sc, runs = _refract(hf, oracle, name, face_normals)
    _receiver_rays_checks(hf, sc, runs, name, "refract", XTOL["pos"])
    for (eta, plane), r in runs.items():
        for sigma_t, tname, wrap in RS.REFRACT_VARIANTS:
            img, val, vis, pos = hf.refraction_lighting(sc.shape, sc.si, sc.ray, r.rcv, _bitmap(hf, tname, wrap), eta=eta, sigma_t=sigma_t,
                                                        spp=SPP, return_value=True, return_visibility=True, return_position=True)
            assert torch.equal(vis, r.byte) and torch.equal(pos, r.pos) and bool((val[~vis.bool()] == 0).all()), (eta, plane, tname)
            assert float((img - val.reshape(-1, SPP).double().mean(1)).abs().max()) <= 2.5e-7 * float(val.abs().max())


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_refract_values_adjoint_and_tangent_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    sc, runs = _refract(hf, oracle, name, face_normals)
    x = RR.inputs(sc.n, SPP, RS.REFRACT_TEX[::-1])
    worst = {k: 0.0 for k in XTOL if k != "pos"}
    for (eta, plane), r in runs.items():
        keep, pix, vis = r.keep, r.pix, r.vis
        assert keep.sum() >= 300 and pix.sum() >= 150
        for sigma_t, tname, wrap in RS.REFRACT_VARIANTS:
            ref = RS.refract_evaluate(r, eta, sigma_t, XTEX[tname], XWRAPS[wrap], x)
            si, wt, bm = _caustic_leaf(hf, sc), _cu(x.w).requires_grad_(True), _bitmap(hf, tname, wrap, requires_grad=True)
            img, val, vis2, pos = hf.refraction_lighting(sc.shape, si, sc.ray, r.rcv, bm, eta=eta, sigma_t=sigma_t, spp=SPP, weight=wt,
                                                         return_value=True, return_visibility=True, return_position=True)
            assert torch.equal(vis2, r.byte) and ref["value"][keep].max() > 0.2
            perr = np.abs(_np(pos.detach()) - RR.forward(*r.a, None, None, eta, 0.0, r.rref, XTEX[tname], RR.CLAMP, vis)[2])[:, keep].max()
            assert perr <= XTOL["pos"], (perr, XTOL["pos"])                          # the landing position, texels
            ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
            got = {"value": _np(val.detach()), "image": _np(img.detach()), "grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad),
                   "grad_weight": _np(wt.grad), "grad_tex": _np(bm.data.grad)}
            for k in ("grad_sh_n", "grad_p", "grad_weight"):
                assert not got[k][..., ~vis].any()                                  # exact zeros where vis = 0
            with fwAD.dual_level():
                sd = hf.SurfaceInteraction3f()
                sd.p, sd.n, sd.t = fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)), sc.si.n.detach(), sc.si.t.detach()
                sd.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)))
                bd = hf.Bitmap(fwAD.make_dual(_cu(XTEX[tname]), _cu(x.dtex)), wrap=wrap)
                ti, tv = hf.refraction_lighting(sc.shape, sd, sc.ray, r.rcv, bd, eta=eta, sigma_t=sigma_t, spp=SPP,
                                                weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), return_value=True)
                got["dimage"], got["dvalue"] = _np(fwAD.unpack_dual(ti).tangent).copy(), _np(fwAD.unpack_dual(tv).tangent).copy()
            assert not got["dvalue"][~vis].any()
            err = RS.refract_errors(got, ref, keep, pix)
            gap = transposition_gap(((got["dimage"], x.gi), (got["dvalue"], x.gv)),
                                    ((got["grad_sh_n"], x.dn), (got["grad_p"], x.dp), (got["grad_weight"], x.dw), (got["grad_tex"], x.dtex)))
            size = np.linalg.norm(ref["dimage"]) * np.linalg.norm(x.gi) + np.linalg.norm(ref["dvalue"]) * np.linalg.norm(x.gv)
            print("refract", name, "eta %.3f %s" % (eta, plane), sigma_t, tname, wrap, {k: "%.3g" % v for k, v in err.items()},
                  "pos %.3g / %.3g" % (perr, XTOL["pos"]), "transposition %.3g / %.3g" % (gap / size, XTOL["dvalue"] + XTOL["grad_sh_n"]))
            assert gap <= (XTOL["dvalue"] + XTOL["grad_sh_n"]) * size, (gap, size)
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("refract", name, "worst", {k: "%.3g / %.3g" % (worst[k], XTOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= XTOL[k], (name, k, worst[k], XTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_refract_chain_to_the_heights(hf, oracle, name, face_normals):
    """refraction_lighting (eta 1 / 1.33, the far receiver, sigma_t 0.7, the smooth texture clamped) -> loss -> backward() ->
    shape.heightfield.grad against the restatement's grad_sh_n and grad_p (fed with the GPU's records and visibility;
    upstream gradients only on the pixels all of whose samples are kept).  Bound: four times the float32 error of grad_sh_n
    + the 1e-5 of the sky row's chain, as the caustic row's chain has it"""
    sc, runs = _refract(hf, oracle, name, face_normals)
    eta = RS.CAUSTIC_ETAS[1]
    r = runs[(eta, "far")]
    x = RR.inputs(sc.n, SPP, RS.REFRACT_TEX[::-1])
    gi = np.where(r.pix, x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.refraction_lighting(shape, si, sc.ray, r.rcv, _bitmap(hf, "smooth", "clamp"), eta=eta, sigma_t=0.7, spp=SPP,
                                      return_visibility=True)
    assert torch.equal(vis, r.byte)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(v) for v in (si.p, si.n, si.sh_frame.n, sc.ray.d, si.t))
    gm, gp, _, _ = RR.adjoint(*a, None, None, eta, 0.7, r.rref, XTEX["smooth"], RR.CLAMP, r.vis, gi, None, SPP)
    gh = _to_heights(hf, oracle, sc, shape, gm, gp, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("refract", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, XTOL["grad_sh_n"] + 1e-5),
          "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= XTOL["grad_sh_n"] + 1e-5, err


# ---- the glossy row: GLOSSY_K mirror rays per sample about drawn microfacet normals, the oblique view ---------------------
GTOL = RS.TOL["glossy"]
GK = RS.GLOSSY_K
_GLOSSY = {}


def _glossy(hf, oracle, name, face_normals, akind):
    """the GLOSSY_K materialised rays and normals, their any-hit answers and the fused word of a scene under one roughness row,
    once; (g) the conditions of tests/test_row_scenes.py on the GPU's own records and bits"""
    key = (name, face_normals, akind)
    if key not in _GLOSSY:
        sc = _scene(hf, oracle, name, "oblique", face_normals)
        alpha_t = _cu(GL.alpha_row(akind, sc.n))
        env, _, _ = envmap(hf, GL.MAP_SIZES, GL.ROTS, "gradient", "identity")
        _, words = hf.glossy_lighting(sc.shape, sc.si, sc.ray, env, alpha_t, spp=SPP, num_rays=GK, seed=RS.GLOSSY_SEED, return_visibility=True)
        r = RS.glossy_run(sc, sc.np, sc.np["d"], sc.np["t"], akind, sc.field, bits=GL.unpack(_np(words), GK))
        r.alpha_t, r.words = alpha_t, words
        r.rr, r.hh = zip(*[hf.glossy_rays(sc.si, sc.ray, alpha_t, k, seed=RS.GLOSSY_SEED, return_normal=True) for k in range(GK)])
        r.occluded = [sc.shape.ray_test(q) for q in r.rr]
        print("glossy", name, "face" if face_normals else "smooth", "alpha", akind, r.counts)
        RS.glossy_conditions(sc, r)                                                # (g)
        _GLOSSY[key] = (sc, r)
    return _GLOSSY[key]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_glossy_rays_against_the_restatement_and_visibility_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals):
    worst = {"ray_d": 0.0, "ray_h": 0.0}
    for akind, _, _ in RS.GLOSSY_COMBOS:
        sc, r = _glossy(hf, oracle, name, face_normals, akind)
        assert not bool((r.words >> GK).any())                                       # no bit at or above num_rays
        num = np.zeros(4)
        for k in range(GK):
            o, d, maxt, h = _np(r.rr[k].o), _np(r.rr[k].d), _np(r.rr[k].maxt), _np(r.hh[k])
            tr = maxt >= 0
            two = (r.rr[k].maxt >= 0) & ~r.occluded[k]
            fused = ((r.words >> k) & 1).bool()
            assert torch.equal(fused, two), (akind, k, int((fused != two).sum()))                                # (b)
            r7 = np.concatenate([o, d, maxt[None]]).astype(np.float32)
            occ = sc.field.ray_test(r7[:, tr]).astype(bool)
            assert np.array_equal(r.bits[k][tr], ~occ) and not r.bits[k][~tr].any(), (akind, k)                  # (c)
            sure = r.sure_k[k]
            assert np.array_equal(tr[sure], r.traced[k][sure]), (akind, k)                                       # (a)
            assert np.all(maxt[tr] == np.inf) and np.all(maxt[~tr] == -1.0) and not o[:, ~tr].any() and not d[:, ~tr].any()
            assert not h[:, ~sc.hit].any()
            both = tr & r.traced[k] & sure
            assert np.abs(np.linalg.norm(d[:, both], axis=0) - 1).max() <= 1e-5 and np.abs(o - r.o[k])[:, both].max() <= 1e-6
            num += RS.glossy_ray_errors(d, h, r, k, both)
        assert num[1] > 1000
        worst["ray_d"], worst["ray_h"] = max(worst["ray_d"], math.sqrt(num[0] / num[1])), max(worst["ray_h"], math.sqrt(num[2] / num[3]))
    print("glossy", name, "worst", {k: "%.3g / %.3g" % (worst[k], GTOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= GTOL[k], (name, k, worst[k], GTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_glossy_values_adjoint_and_tangent_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    worst = {k: 0.0 for k in GTOL if not k.startswith("ray")}
    for akind, mname, rname in RS.GLOSSY_COMBOS:
        sc, r = _glossy(hf, oracle, name, face_normals, akind)
        keep = r.keep
        kp = keep.reshape(-1, SPP).all(1)
        assert float((~keep).mean()) <= RS.UNSURE_CAP
        for eta in RS.GLOSSY_ETAS:
            env, full, rot = envmap(hf, GL.MAP_SIZES, GL.ROTS, mname, rname, requires_grad=True)
            x = GL.test_inputs(sc.n, full.shape)
            w, gi, gv, dn, dw, da, dd = x
            ref = RS.glossy_evaluate(r, eta, full, rot, x)
            ref["grad_data"] = _fold(ref["grad_data"])
            si = leaf_si(hf, sc)
            wt, at = _cu(w).requires_grad_(True), r.alpha_t.clone().requires_grad_(True)
            img, val, words = hf.glossy_lighting(sc.shape, si, sc.ray, env, at, eta=eta, spp=SPP, num_rays=GK, seed=RS.GLOSSY_SEED, weight=wt,
                                                 return_value=True, return_visibility=True)
            assert torch.equal(words, r.words)
            lit = r.bits.any(0)
            assert not _np(val.detach())[~lit].any() and lit[keep].sum() >= 200 and ref["value"].max() > 0.01
            ((img * _cu((gi * kp).astype(np.float32))).sum() + (val * _cu((gv * keep).astype(np.float32))).sum()).backward()
            got = {"value": _np(val.detach()), "image": _np(img.detach()), "grad_sh_n": _np(si.sh_frame.n.grad), "grad_weight": _np(wt.grad),
                   "grad_alpha": _np(at.grad), "grad_data": _np(env.data.grad)}
            for k in ("grad_sh_n", "grad_weight", "grad_alpha"):
                assert not got[k][..., ~lit].any()                                  # exact zeros where no bit is set
            with fwAD.dual_level():
                sd = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu((dn * keep).astype(np.float32))))
                envd = hf.Envmap(fwAD.make_dual(env.data.detach(), _cu(dd[:, :-1])), to_world=rot)
                ti, tv = hf.glossy_lighting(sc.shape, sd, sc.ray, envd, fwAD.make_dual(r.alpha_t, _cu((da * keep).astype(np.float32))), eta=eta,
                                            spp=SPP, num_rays=GK, seed=RS.GLOSSY_SEED,
                                            weight=fwAD.make_dual(_cu(w), _cu((dw * keep).astype(np.float32))), return_value=True)
                got["dimage"], got["dvalue"] = _np(fwAD.unpack_dual(ti).tangent).copy(), _np(fwAD.unpack_dual(tv).tangent).copy()
            assert not got["dvalue"][~lit].any()
            err = RS.glossy_errors(got, ref, keep)
            gap = transposition_gap(((got["dimage"], gi * kp), (got["dvalue"], gv * keep)),
                                    ((got["grad_sh_n"], dn * keep), (got["grad_weight"], dw * keep), (got["grad_alpha"], da * keep),
                                     (got["grad_data"], dd[:, :-1])))
            size = np.linalg.norm(ref["dimage"]) * np.linalg.norm(gi * kp) + np.linalg.norm(ref["dvalue"]) * np.linalg.norm(gv * keep)
            print("glossy", name, "alpha", akind, mname, rname, "eta", eta, {k: "%.3g" % v for k, v in err.items()},
                  "transposition %.3g / %.3g" % (gap / size, GTOL["dvalue"] + GTOL["grad_sh_n"]))
            assert gap <= (GTOL["dvalue"] + GTOL["grad_sh_n"]) * size, (gap, size)
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("glossy", name, "worst", {k: "%.3g / %.3g" % (worst[k], GTOL[k]) for k in worst})
    for k in worst:
        assert worst[k] <= GTOL[k], (name, k, worst[k], GTOL[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_glossy_chain_to_the_heights(hf, oracle, name, face_normals):
    """glossy_lighting (alpha 0.3, eta 1.5, the gradient map rotated) -> loss -> backward() -> shape.heightfield.grad against
    the restatement's grad_sh_n (fed with the GPU's records and bits; upstream gradients only on the pixels all of whose
    samples are kept).  Bound: four times the float32 error of grad_sh_n + the 1e-5 of the sky row's chain, as
    tests/test_gpu_glossy.py has it"""
    sc, r = _glossy(hf, oracle, name, face_normals, 0.3)
    env, full, rot = envmap(hf, GL.MAP_SIZES, GL.ROTS, "gradient", "rotated")
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, words = hf.glossy_lighting(shape, si, sc.ray, env, 0.3, eta=1.5, spp=SPP, num_rays=GK, seed=RS.GLOSSY_SEED, return_visibility=True)
    assert torch.equal(words, r.words) and float(img.detach().sum()) > 0
    gi = (np.random.default_rng(11).normal(size=sc.n // SPP) * r.keep.reshape(-1, SPP).all(1)).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = tuple(_np(v) for v in (si.n, si.sh_frame.n, sc.ray.d, si.t))
    gm, _, _, _ = GL.adjoint(*a, None, None, 0.3, 1.5, GK, RS.GLOSSY_SEED, None, full, rot, r.bits, SPP, gi, None)
    gh = _to_heights(hf, oracle, sc, shape, gm, None, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("glossy", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, GTOL["grad_sh_n"] + 1e-5),
          "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= GTOL["grad_sh_n"] + 1e-5, err


# ---- the specular row: traces nothing; the directional row's byte, the steep view -----------------------------------------
STOL = RS.TOL["specular"]
_SPECULAR = {}


def _specular(hf, oracle, name, face_normals):
    """the directional row's launch of the scene (_rigged: its byte, its lights, its conditions), the roughness rows and the
    K = 8 specular launch under "row" with a weight; (g) the conditions of tests/test_row_scenes.py on the GPU's own records,
    byte and values, asserted before anything is compared"""
    key = (name, face_normals)
    if key not in _SPECULAR:
        q = _rigged(hf, oracle, "directional", name, face_normals)
        sc = q.sc
        s = types.SimpleNamespace(q=q, sc=sc, x=SP.inputs(sc.n, SPP, q.K), byte=_cu(q.byte))
        assert np.array_equal(s.x.w, q.x.w)
        s.alpha = {kind: SP.alpha_row(kind, sc.n) for kind in RS.specular_kinds(name, face_normals)}
        img, val = hf.specular_lighting(sc.si, sc.ray, q.lights, s.byte, _cu(s.alpha["row"]), eta=SP.ETA, spp=SPP, weight=_cu(s.x.w),
                                        return_value=True)
        s.img, s.val = _np(img).copy(), _np(val).copy()
        s.lit = RS.specular_lit(q.names, s.val)
        print("specular", name, "face" if face_normals else "smooth", "share of samples with a highlight", {k: round(v, 3) for k, v in s.lit.items()})
        RS.specular_conditions(sc, q.pop, s.lit)                                    # (g)
        _SPECULAR[key] = s
    return _SPECULAR[key]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_specular_values_gradients_and_tangents_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals):
    """(d), (e), (g): through the public function, backward() and forward_ad, every light's numbers and the roughness row
    the user's own tensors; specular_ref.errors()' measures, NO sample left out"""
    s = _specular(hf, oracle, name, face_normals)
    sc, q, x = s.sc, s.q, s.x
    K = q.K
    for kind, alpha in s.alpha.items():
        tol = STOL[kind]
        worst = {k: 0.0 for k in tol}
        for weighted in ((True, False) if kind == "row" else (True,)):
            si = leaf_si(hf, sc)
            wt = _cu(x.w).requires_grad_(True) if weighted else None
            at = _cu(alpha).requires_grad_(True)
            par = [[_f64(v).requires_grad_(True) for v in (L.to_light, L.irradiance)] for L in q.ref]
            img, val = hf.specular_lighting(si, sc.ray, [hf.DirectionalLight(*p) for p in par], s.byte, at, eta=SP.ETA, spp=SPP, weight=wt,
                                            return_value=True)
            ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
            got = types.SimpleNamespace(image=_np(img.detach()).copy(), value=_np(val.detach()).copy(), gn=_np(si.sh_frame.n.grad),
                                        gw=_np(wt.grad) if weighted else None, ga=_np(at.grad),
                                        g4=_np(torch.stack([_flat([t.grad for t in p]) for p in par])))
            assert got.g4.shape == (K, SP.PARAMS)
            if kind == "row" and weighted:
                assert np.array_equal(got.image, s.img) and np.array_equal(got.value, s.val)
            with fwAD.dual_level():
                sid = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)))
                dual = [hf.DirectionalLight(fwAD.make_dual(_f64(L.to_light), _f64(x.dl[k, :3])),
                                            fwAD.make_dual(_f64(L.irradiance), _f64(x.dl[k, 3]))) for k, L in enumerate(q.ref)]
                out = hf.specular_lighting(sid, sc.ray, dual, s.byte, fwAD.make_dual(_cu(alpha), _cu(x.da)), eta=SP.ETA, spp=SPP,
                                           weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)) if weighted else None, return_value=True)
                got.dimage, got.dvalue = (_np(fwAD.unpack_dual(o).tangent).copy() for o in out)
            ref = RS.specular_evaluate(q.ref, sc.np, sc.np["d"], x, kind, q.vis, weighted=weighted)
            # every sample takes part: the masks of both sides are the byte and the double cosines
            assert got.value.shape == ref.value.shape == (K, sc.n) and np.array_equal(got.value > 0, ref.value > 0)
            assert not got.value[~q.vis].any() and not got.dvalue[~q.vis].any()     # exactly 0 where the byte's bit is clear
            dark = ~q.vis.any(0)
            for k in ("gn", "gw", "ga"):
                assert getattr(got, k) is None or not getattr(got, k)[..., dark].any()
            assert not got.g4[q.names.index("below")].any() or q.vis[q.names.index("below")].any()
            assert ref.value.max() > 0.05 and np.abs(ref.ga).max() > 0 and (np.abs(ref.g4).max(1) > 0).sum() >= K - 1
            err = SP.errors(got, ref)
            print("specular", name, kind, "weighted" if weighted else "unweighted", {k: "%.3g" % v for k, v in err.items()})
            for k, v in err.items():
                worst[k] = max(worst[k], v)
            if weighted:
                # the bound of tests/test_gpu_specular.py: the device's own rounding, 8 ulp per element on the tangent side and
                # the project's factor 4 for the adjoint side's regrouping, of the mass sum |tangent| |upstream|
                gap = transposition_gap(((got.dimage, x.gi), (got.dvalue, x.gv)),
                                        ((got.gn, x.dn), (got.gw, x.dw), (got.ga, x.da), (got.g4, x.dl)))
                mass = np.abs(got.dvalue.astype(np.float64) * x.gv).sum() + np.abs(got.dimage.astype(np.float64) * x.gi).sum()
                bound = (8 + 4 * 8) * 2.0 ** -24 * mass
                print("specular", name, kind, "transposition gap %.3g / %.3g" % (gap, bound))
                assert mass > 0 and gap <= bound, (gap, mass, bound)
        print("specular", name, kind, "worst", {k: "%.3g / %.3g" % (worst[k], tol[k]) for k in tol})
        for k in tol:
            assert worst[k] <= tol[k], (name, kind, k, worst[k], tol[k])


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_specular_chain_to_the_heights(hf, oracle, name, face_normals):
    """(f): ray_intersect -> directional_lighting (visibility) -> specular_lighting -> loss -> backward() -> shape.heightfield.grad
    against the restatement's grad_sh_n (fed with the GPU's records and byte) carried to the heights by _to_heights under the
    scene's to_world and flip_normals.  Bound: RS.CHAIN, the directional row's for its chain"""
    s = _specular(hf, oracle, name, face_normals)
    sc, q, x = s.sc, s.q, s.x
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    _, vis = hf.directional_lighting(shape, si, sc.ray, q.lights, spp=SPP, return_visibility=True)
    assert np.array_equal(_np(vis), q.byte)
    img = hf.specular_lighting(si, sc.ray, q.lights, vis, _cu(s.alpha["row"]), eta=SP.ETA, spp=SPP)
    (img * _cu(x.gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = SP.adjoint(q.ref, _np(si.sh_frame.n), sc.np["d"], None, s.alpha["row"], SP.ETA, q.vis, SPP, x.gi)
    gh = _to_heights(hf, oracle, sc, shape, g.gn, None, face_normals)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("specular", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, RS.CHAIN), "norm", np.linalg.norm(gh))
    assert got.shape == (sc.H, sc.W) and np.linalg.norm(gh) > 0 and err <= RS.CHAIN, err


# ---- the medium row: shadow rays that start in free space, on the primary ray, under a world-space top plane --------------
MTOL = RS.TOL["medium"]
MK, MSEED = RS.MEDIUM_K, RS.MEDIUM_SEED
MEDIUM_CASES = [(name, fn, mname) for name, fn in RS.CASES for mname in RS.MEDIUM_NAMES]
_MEDIUM = {}


def _medium_objects(hf, r, scalars=None, irradiances=None):
    """(hf.Medium, the eight hf.DirectionalLights) of the run r; scalars, irradiances: the user's tensors in their place"""
    M = r.M
    med = hf.Medium(*((M.sigma_t, M.albedo, M.g) if scalars is None else scalars), top_origin=M.top_origin, top_normal=M.top_normal)
    return med, [hf.DirectionalLight(L.to_light, L.irradiance if irradiances is None else irradiances[j]) for j, L in enumerate(r.lights)]


def _medium(hf, oracle, name, face_normals, mname):
    """a (case, medium), once: all eight lights in one fused launch with a weight, the 8 x MK materialised rays, the run of
    tests/row_scenes.py on the GPU's own primary rays, origins and words; (g) its conditions, asserted before anything is
    compared"""
    key = (name, face_normals, mname)
    if key not in _MEDIUM:
        sc = _scene(hf, oracle, name, RS.MEDIA[mname]["view"], face_normals)
        o, d, t = sc.rays[0:3], sc.np["d"], sc.np["t"]
        assert np.array_equal(d, sc.rays[3:6])
        r = RS.medium_run(sc, mname, o, d, t, sc.field)                              # (the restatement's origins: replaced below)
        x = MR.inputs(sc.n, SPP, len(r.lights))
        med, lights = _medium_objects(hf, r)
        img, val, words = hf.medium_lighting(sc.shape, sc.si, sc.ray, lights, med, spp=SPP, num_steps=MK, seed=MSEED, weight=_cu(x.w),
                                             return_value=True, return_visibility=True)
        rays = [[hf.medium_rays(sc.si, sc.ray, lights[j], med, k, seed=MSEED) for k in range(MK)] for j in range(len(lights))]
        first = int(np.argmax(r.shines))
        for j in np.flatnonzero(r.shines):                                           # the point does not depend on the light
            assert all(torch.equal(rays[j][k].o, rays[first][k].o) for k in range(MK)), r.names[j]
        q = RS.medium_run(sc, mname, o, d, t, sc.field, words=_np(words).view(np.uint32), origins=np.stack([_np(rays[first][k].o) for k in range(MK)]))
        q.sc, q.x, q.med, q.gpu_lights, q.rays, q.words_t = sc, x, med, lights, rays, words
        q.img, q.val = _np(img).copy(), _np(val).copy()
        print("medium", name, "face" if face_normals else "smooth", mname, RS.medium_describe(q))
        RS.medium_conditions(sc, q)                                                  # (g)
        _MEDIUM[key] = q
    return _MEDIUM[key]


@pytest.mark.parametrize("name,face_normals,mname", MEDIUM_CASES)
def test_medium_rays_against_the_restatement_and_words_against_the_two_call_sequence_and_the_oracle(hf, oracle, name, face_normals, mname):
    q = _medium(hf, oracle, name, face_normals, mname)
    sc, J = q.sc, len(q.lights)
    words = q.words
    # (a) every (light, point): masks, directions and maxt exactly, origins within four times the float32 restatement's error
    worst = 0.0
    for j, L in enumerate(q.lights):
        lf = MR.unit(L)[0].astype(np.float32)
        for k in range(MK):
            o, d, maxt = _np(q.rays[j][k].o), _np(q.rays[j][k].d), _np(q.rays[j][k].maxt)
            ro, _, rmaxt, tr = MR.rays(q.M, L, q.o, q.d, q.t, k, MSEED)
            assert np.array_equal(tr, q.traced[j]) and np.array_equal(maxt, rmaxt) and np.isin(maxt, (np.inf, -1.0)).all(), (q.names[j], k)
            assert np.array_equal(d, np.where(tr[None], lf[:, None], np.float32(0))) and not o[:, ~tr].any(), (q.names[j], k)
            if tr.any():
                worst = max(worst, float(np.abs(o - ro)[:, tr].max()))
    print("medium", name, mname, "largest origin difference %.3g / %.3g" % (worst, MTOL["origin"]))
    assert 0 < worst <= MTOL["origin"], worst
    # (b) the fused words against medium_rays + shape.ray_test, bit for bit, in both coherence modes; nothing where no light shines in
    assert not (words >> np.uint32(MK)).any()                                        # no bit at or above num_steps
    assert not words[q.names.index("below")].any() and (mname != "tilted" or not words[q.names.index("graze")].any())
    old = sc.shape.ray_coherence()
    for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
        sc.shape.set_ray_coherence(mode)
        try:
            _, again = hf.medium_lighting(sc.shape, sc.si, sc.ray, q.gpu_lights, q.med, spp=SPP, num_steps=MK, seed=MSEED, return_visibility=True)
            two = np.stack([np.stack([_np((q.rays[j][k].maxt >= 0) & ~sc.shape.ray_test(q.rays[j][k])) for k in range(MK)]) for j in range(J)])
        finally:
            sc.shape.set_ray_coherence(old)
        assert torch.equal(again, q.words_t), mode
        assert np.array_equal(two, q.bits), (mode, int((two != q.bits).sum()))
    # (c) the words against the oracle's ray_test (the same to_world and flip_normals) on the GPU's own rays: exactly, but for
    # the lanes whose origin lies closer to the primary hit than the sky row's spawn offset
    keep = ~q.near[None]
    assert np.array_equal((q.bits & keep), (q.oracle & keep)), int(((q.bits != q.oracle) & keep).sum())
    print("medium", name, mname, "left out of the comparison with the oracle: %d lanes, share %.3g / %.3g; they differ on %d"
          % (q.counts["near_lanes"], q.counts["near"], RS.UNSURE_CAP, int((q.bits != q.oracle).sum())))
    assert q.counts["near"] <= RS.UNSURE_CAP


def _medium_params_bound(ref, n):
    """tests/test_gpu_medium.py's _check_params: the kernel adds n double terms in double and rounds the sum to float32 once"""
    return 2.0 ** -23 * np.abs(ref.gp) + (n + 64) * 2.0 ** -53 * ref.gp_abs


def _medium_slack(p):
    """what the row's rule allows an element of the float32 result p: rtol |p| + atol max(1, largest |p|)"""
    p = np.abs(np.asarray(p, np.float64))
    return RS.MEDIUM_RTOL * p + RS.MEDIUM_ATOL * max(1.0, p.max())


@pytest.mark.parametrize("name,face_normals,mname", MEDIUM_CASES)
def test_medium_values_gradients_and_tangents_against_the_restatement_and_the_transposition_gap(hf, oracle, name, face_normals, mname):
    """(d), (e): through the public function, backward() and forward_ad; sigma_t, albedo, g and the eight irradiances are
    float64 host leaves (duals).  The row's own rule: rtol 1e-5, atol 1e-7 max(1, largest |reference|); the reduced numbers
    within the bound of tests/test_gpu_medium.py's _check_params"""
    q = _medium(hf, oracle, name, face_normals, mname)
    sc, x, M, J, n = q.sc, q.x, q.M, len(q.lights), q.sc.n
    a = (M, q.lights, q.o, q.d, q.t, x.w, q.words, MK, MSEED)
    rimg, rval = MR.forward(*a, spp=SPP)
    close = {"value": RS.medium_close(q.val, rval), "image": RS.medium_close(q.img, rimg)}
    print("medium", name, mname, "largest |value| %.3g |image| %.3g" % (np.abs(rval).max(), np.abs(rimg).max()))
    assert np.abs(rval).max() > 1e-3 and np.abs(rimg).max() > 1e-3
    assert not q.val[q.words == 0].any() and (q.val[q.words != 0] > 0).all()         # exact zeros where no bit is set
    # ---- backward()
    si = hf.SurfaceInteraction3f()
    si.p, si.n, si.sh_frame = sc.si.p.detach(), sc.si.n.detach(), sc.si.sh_frame
    si.t = sc.si.t.detach().clone().requires_grad_(True)
    wt = _cu(x.w).requires_grad_(True)
    scal = [_f64(v).requires_grad_(True) for v in (M.sigma_t, M.albedo, M.g)]
    E = [_f64(L.irradiance).requires_grad_(True) for L in q.lights]
    med, lights = _medium_objects(hf, q, scal, E)
    img, val, words = hf.medium_lighting(sc.shape, si, sc.ray, lights, med, spp=SPP, num_steps=MK, seed=MSEED, weight=wt, return_value=True,
                                         return_visibility=True)
    assert torch.equal(words, q.words_t) and np.array_equal(_np(val.detach()), q.val) and np.array_equal(_np(img.detach()), q.img)
    ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
    gw, gt = _np(wt.grad), _np(si.t.grad)
    gp = np.array([float(v.grad) for v in scal + E])
    ref = MR.adjoint(*a, spp=SPP, grad_image=x.gi, grad_value=x.gv)
    close["grad_weight"], close["grad_t"] = RS.medium_close(gw, ref.gw), RS.medium_close(gt, ref.gt)
    none = (q.words == 0).all(0)
    assert not gw[none].any() and not gt[none].any() and not gt[~np.isfinite(q.t)].any()     # grad_t exactly zero where t = inf
    assert np.abs(ref.gt).max() > 0 and np.abs(ref.gw).max() > 0
    bound = _medium_params_bound(ref, n)
    print("medium", name, mname, "the 3 + 8 reduced numbers", gp, "float64", ref.gp, "allowed", bound)
    shines = np.concatenate([[True] * MR.PARAMS, q.shines])
    assert (ref.gp_abs[shines] > 0).all() and not gp[~shines].any() and not ref.gp_abs[~shines].any()
    assert (np.abs(gp - ref.gp) <= bound).all(), (gp, ref.gp, bound)
    # ---- forward_ad
    with fwAD.dual_level():
        sid = hf.SurfaceInteraction3f()
        sid.p, sid.n, sid.sh_frame = sc.si.p.detach(), sc.si.n.detach(), sc.si.sh_frame
        sid.t = fwAD.make_dual(sc.si.t.detach(), _cu(x.dt))
        dscal = [fwAD.make_dual(_f64(v), _f64(x.dp[i])) for i, v in enumerate((M.sigma_t, M.albedo, M.g))]
        dE = [fwAD.make_dual(_f64(L.irradiance), _f64(x.dp[MR.PARAMS + j])) for j, L in enumerate(q.lights)]
        med, lights = _medium_objects(hf, q, dscal, dE)
        out = hf.medium_lighting(sc.shape, sid, sc.ray, lights, med, spp=SPP, num_steps=MK, seed=MSEED, weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)),
                                 return_value=True)
        dimg, dval = (_np(fwAD.unpack_dual(v).tangent).copy() for v in out)
    rdimg, rdval = MR.tangent(*a, spp=SPP, dw=x.dw, dt=x.dt, d_params=x.dp)
    close["dimage"], close["dvalue"] = RS.medium_close(dimg, rdimg), RS.medium_close(dval, rdval)
    assert not dval[q.words == 0].any() and np.abs(rdval).max() > 0
    print("medium", name, mname, "worst (|difference| - rtol |reference|) / (atol max(1, largest |reference|)), allowed 1:",
          {k: "%.3g" % v for k, v in close.items()})
    for k, v in close.items():
        assert v <= 1.0, (name, mname, k, v)
    # ---- the transposition gap on the device, the bound built from the tolerances above
    lhs = [(dimg, x.gi), (dval, x.gv)]
    rhs = [(gt, x.dt), (gw, x.dw)]
    gap = transposition_gap(lhs, rhs + [(gp, x.dp)])
    allowed = sum((_medium_slack(p) * np.abs(v)).sum() for p, v in lhs + rhs) + (bound * np.abs(x.dp)).sum()
    print("medium", name, mname, "transposition gap %.3g / %.3g" % (gap, allowed))
    assert gap <= allowed, (gap, allowed)


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_medium_chain_to_the_heights(hf, oracle, name, face_normals):
    """(f): medium_lighting under `skim` -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_t (fed
    with the GPU's t and words) carried to the heights: by the oracle's adjoint of t under the scene's to_world and
    flip_normals (flat shading) or by shape.adjoint with ybar[0] = grad_t (smooth).  Bound: RS.CHAIN"""
    q = _medium(hf, oracle, name, face_normals, "skim")
    sc, x = q.sc, q.x
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, words = hf.medium_lighting(shape, si, sc.ray, q.gpu_lights, q.med, spp=SPP, num_steps=MK, seed=MSEED, return_visibility=True)
    assert torch.equal(words, q.words_t) and np.array_equal(_np(si.t), q.t)
    (img * _cu(x.gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    gt = MR.adjoint(q.M, q.lights, q.o, q.d, q.t, None, q.words, MK, MSEED, spp=SPP, grad_image=x.gi).gt
    assert not gt[~sc.hit].any()
    if face_normals:
        t, u, v, prim = sc.pi_oracle
        gh = sc.field.adjoint(sc.rays, t, u, v, prim, {"t": gt.astype(np.float32)[None]}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[0] = _cu(gt.astype(np.float32))
        gh = _np(shape.adjoint(sc.ray, shape.ray_intersect_preliminary(sc.ray), ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("medium", name, "face_normals", face_normals, "dL/dheight relative L2 error %.3g / %.3g" % (err, RS.CHAIN), "norm", np.linalg.norm(gh))
    assert got.shape == (sc.H, sc.W) and np.linalg.norm(gh) > 0 and err <= RS.CHAIN, err

"""The medium row on the device (hf_medium_rays, hf_medium_lighting, _adjoint, _tangent) against tests/medium_ref.py; under to_world, flip_normals and odd grids: tests/test_gpu_row_scenes.py.
The scene here: row_helpers.base_scene (sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic
wavefront) from medium_ref.ORIGIN plus a second wavefront of the same direction centred over the terrain's +x edge, of
which most passes beside the terrain (t = inf): 32768 samples, K = 4 points, 131072 shadow rays per light.  Two lights
(medium_ref.RIG: a raking one and a high one) and three media (medium_ref.MEDIA): top plane z = 1.5 below the camera
(u_in > 0, D = 0, S >= 1), top plane z = 3 above it (u_in = 0, D > 0), and a tilted top.

  (a) materialised rays against the restatement: directions exact, origins within four times the float32 restatement's
      own error (profiles/medium/f32_error.json, scripts/medium_f32_error.py), maxt in {inf, -1}, a permuted ray_id
  (b) the fused bits against hf_medium_rays + hf_ray_test, bit for bit, for every (j, k)
  (c) the bits against the oracle's ray_test on the GPU's own rays, exactly, but for the lanes whose origin lies closer
      to the primary hit than the sky row's spawn offset (at most row_helpers.UNSURE_CAP of the traced lanes)
  (d) image, value, adjoint and tangent against the restatement fed with the GPU's bits: rtol 1e-5, atol 1e-7 with
      |value| <= 1 (the rule of tests/test_gpu_sky_lighting.py); the reduced numbers against the float64 sums
  (e) the transposition gap, (f) autograd down to the heights, (g) robustness, (h) examples/inverse_fog.py"""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import medium_ref as R
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, base_scene, intact, transposition_gap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
F32 = json.load(open(os.path.join(ROOT, "profiles", "medium", "f32_error.json")))["maxima"]
ORIGIN_TOL = 4 * F32["origin_max"]   # the margin the reflection row uses over its float32 restatement
RTOL, ATOL = 1e-5, 1e-7
K, SEED = R.K, R.SEED
_SCENE = {}


def _scene(hf, oracle):
    if "sc" not in _SCENE:
        sc = base_scene(hf, oracle, R.FILM, R.ORIGIN)
        rays = torch.cat([sc.rays, R.wide_rays(hf.workload.ortho_rays, "cuda")], 1).contiguous()
        sc.rays, sc.ray = rays, hf.Ray3f(rays[0:3], rays[3:6], rays[6])
        sc.si = sc.shape.ray_intersect(sc.ray, hf.RayFlags.All)
        sc.n = rays.shape[1]
        sc.o, sc.d, sc.t, sc.p = _np(rays[0:3]), _np(rays[3:6]), _np(sc.si.t), _np(sc.si.p)
        sc.hit = np.isfinite(sc.t)
        assert 0.05 <= sc.hit.mean() <= 0.95 and sc.n == 2 * 64 * 64 * 4, sc.hit.mean()
        sc.lights = R.rig()
        sc.media = {k: R.medium(**v) for k, v in R.MEDIA.items()}
        for k, M in sc.media.items():
            R.assert_scene(k, R.segment(M, sc.o, sc.d, sc.t), sc.t)
        sc.bits = {}
        _SCENE["sc"] = sc
    return _SCENE["sc"]


def _light(hf, L):
    return hf.DirectionalLight(L.to_light, L.irradiance)


def _medium(hf, M):
    return hf.Medium(M.sigma_t, M.albedo, M.g, top_origin=M.top_origin, top_normal=M.top_normal)


def _structs(hf, M, lights):
    cap = hf._capi
    m = cap.hf_medium_t((C.c_double * 3)(*M.top_origin), (C.c_double * 3)(*M.top_normal), M.sigma_t, M.albedo, M.g)
    L = (cap.hf_directional_light_t * len(lights))()
    for j, s in enumerate(lights):
        L[j] = cap.hf_directional_light_t((C.c_double * 3)(*s.to_light), s.irradiance)
    return m, L


def _p(x):
    return None if x is None else x.data_ptr()


def _p3(hf, x):
    return (hf._capi._fp * 3)(*[x[c].data_ptr() for c in range(3)])


class _Wave:
    """the samples [lo, hi) of the scene as device rows of their own and the raw entry points on them"""

    def __init__(self, hf, sc, lo=0, hi=None, o=None, d=None, t=None):
        hi = sc.n if hi is None else hi
        cut = lambda x: x[..., lo:hi].contiguous()
        self.hf, self.shape = hf, sc.shape
        self.o = cut(sc.rays[0:3]) if o is None else _cu(o.astype(np.float32))
        self.d = cut(sc.rays[3:6]) if d is None else _cu(d.astype(np.float32))
        self.t = cut(sc.si.t.detach()) if t is None else _cu(t.astype(np.float32))
        self.n = self.o.shape[1]
        self.np = {"o": _np(self.o), "d": _np(self.d), "t": _np(self.t)}

    def _head(self, M, lights, spp, w, K, seed, rid):
        m, L = _structs(self.hf, M, lights)
        self.keep = (m, L, w, rid)
        return (self.n, spp, _p3(self.hf, self.o), _p3(self.hf, self.d), self.t.data_ptr(), _p(w), C.byref(m), len(lights), L, K, seed,
                _p(rid))

    def forward(self, M, lights, K=K, seed=SEED, spp=1, w=None, rid=None, want=(True, True, True)):
        J, n = len(lights), self.n
        img = torch.full((J, n // spp), GUARD, device="cuda") if want[0] else None
        val = torch.full((J, n), GUARD, device="cuda") if want[1] else None
        bits = torch.full((J, n), -7, dtype=torch.int32, device="cuda") if want[2] else None
        self.hf._capi.check(self.hf._capi.lib().hf_medium_lighting(self.shape._h, *self._head(M, lights, spp, w, K, seed, rid), _p(img), _p(val),
                                                                   _p(bits), None))
        torch.cuda.synchronize()
        return img, val, bits

    def adjoint(self, M, lights, bits, gi, gv, K=K, seed=SEED, spp=1, w=None, rid=None, want=(True, True, True)):
        J = len(lights)
        gw = torch.full((self.n,), GUARD, device="cuda") if want[0] else None
        gt = torch.full((self.n,), GUARD, device="cuda") if want[1] else None
        gp = torch.zeros(R.PARAMS + J, device="cuda") if want[2] else None
        lib = self.hf._capi.lib()
        ws = torch.empty(lib.hf_medium_workspace_floats(J), device="cuda") if want[2] else None
        self.hf._capi.check(lib.hf_medium_lighting_adjoint(*self._head(M, lights, spp, w, K, seed, rid), bits.data_ptr(), _p(gi), _p(gv),
                                                           _p(gw), _p(gt), _p(gp), _p(ws), None))
        torch.cuda.synchronize()
        return gw, gt, gp

    def tangent(self, M, lights, bits, dw, dt, dp, K=K, seed=SEED, spp=1, w=None, rid=None, want=(True, True)):
        J = len(lights)
        dimg = torch.full((J, self.n // spp), GUARD, device="cuda") if want[0] else None
        dval = torch.full((J, self.n), GUARD, device="cuda") if want[1] else None
        self.hf._capi.check(self.hf._capi.lib().hf_medium_lighting_tangent(*self._head(M, lights, spp, w, K, seed, rid), bits.data_ptr(), _p(dw),
                                                                           _p(dt), _p(dp), _p(dimg), _p(dval), None))
        torch.cuda.synchronize()
        return dimg, dval


def _bits(hf, sc, name):
    """the fused launch's words of the scene under medium `name` and the rig, [2, n] (computed once, shared)"""
    if name not in sc.bits:
        sc.bits[name] = _Wave(hf, sc).forward(sc.media[name], sc.lights)[2]
    return sc.bits[name]


@pytest.mark.parametrize("name", list(R.MEDIA))
def test_materialised_rays_against_the_restatement(hf, oracle, name):
    sc = _scene(hf, oracle)
    M, med = sc.media[name], _medium(hf, sc.media[name])
    perm = np.random.default_rng(3).permutation(sc.n).astype(np.int32)
    worst = 0.0
    for L in sc.lights:
        lf = R.unit(L)[0].astype(np.float32)
        for k in range(K):
            r = hf.medium_rays(sc.si, sc.ray, _light(hf, L), med, k, seed=SEED)
            ro, w, maxt, tr = R.rays(M, L, sc.o, sc.d, sc.t, k, SEED)
            assert tr.all() and np.array_equal(_np(r.maxt), maxt) and np.isin(_np(r.maxt), (np.inf, -1.0)).all()
            assert (_np(r.d) == lf[:, None]).all()                       # directions: exact
            worst = max(worst, float(np.abs(_np(r.o) - ro).max()))
    print(name, "largest origin difference", worst, "allowed", ORIGIN_TOL)
    assert worst <= ORIGIN_TOL
    r = hf.medium_rays(sc.si, sc.ray, _light(hf, sc.lights[0]), med, 2, seed=SEED, ray_index=_cu(perm))
    ro = R.rays(M, sc.lights[0], sc.o, sc.d, sc.t, 2, SEED, ray_id=perm)[0]
    same = R.rays(M, sc.lights[0], sc.o, sc.d, sc.t, 2, SEED)[0]
    assert np.abs(_np(r.o) - ro).max() <= ORIGIN_TOL and np.abs(ro - same).max() > 0.1     # the draw follows the id
    r = hf.medium_rays(sc.si, sc.ray, _light(hf, R.light(*R.BELOW)), med, 0, seed=SEED)     # a light that does not shine in
    assert (_np(r.maxt) == -1).all() and not _np(r.o).any() and not _np(r.d).any()


@pytest.mark.parametrize("name", list(R.MEDIA))
def test_fused_bits_equal_rays_plus_ray_test_bit_for_bit_and_the_oracle(hf, oracle, name):
    sc = _scene(hf, oracle)
    M, med = sc.media[name], _medium(hf, sc.media[name])
    lights = sc.lights + [R.light(*R.BELOW)]
    bits = _np(_Wave(hf, sc).forward(M, lights)[2]).astype(np.uint32)
    assert np.array_equal(bits[:2], _np(_bits(hf, sc, name)).astype(np.uint32))              # the rig of two: the same words
    assert not (bits >> np.uint32(K)).any() and not bits[2].any()                            # no bit at or beyond num_steps; nu <= 0: zeros
    near = traced = seen = 0
    for j, L in enumerate(sc.lights):
        for k in range(K):
            r = hf.medium_rays(sc.si, sc.ray, _light(hf, L), med, k, seed=SEED)
            vis = ~_np(sc.shape.ray_test(r))
            got = ((bits[j] >> np.uint32(k)) & 1).astype(bool)
            assert np.array_equal(got, vis), (j, k, int((got != vis).sum()))                # (b) bit for bit
            # (c) the oracle on the GPU's own rays
            rows = np.concatenate([_np(r.o), _np(r.d), _np(r.maxt)[None]]).astype(np.float32)
            want = ~sc.field.ray_test(rows).astype(bool)
            with np.errstate(invalid="ignore"):
                out = sc.hit & (np.sqrt(((_np(r.o).astype(np.float64) - sc.p) ** 2).sum(0)) < R.spawn_offset(sc.p))
            assert np.array_equal(got[~out], want[~out]), (j, k, int((got != want)[~out].sum()))
            near += int(out.sum()); traced += sc.n; seen += int(got.sum())
    print(name, "left out", near, "of", traced, "visible share", seen / traced)
    assert near <= UNSURE_CAP * traced
    assert 0.05 <= seen / traced <= 0.95                                                     # both outcomes occur


def _check(got, ref, what):
    got, ref = _np(got).astype(np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) - RTOL * np.abs(ref)
    print(what, "largest |difference|", float(np.abs(got - ref).max()), "largest |difference| - rtol |ref|", float(err.max()),
          "largest |ref|", float(np.abs(ref).max()))
    assert (err <= ATOL).all(), (what, float(err.max()))


def _check_params(got, ref, n, what):
    """the reduced numbers: the kernel adds double terms in double (n of them, each a few dozen roundings from the
    restatement's) and rounds the sum to float32 once"""
    got = _np(got).astype(np.float64)
    tol = 2.0 ** -23 * np.abs(ref.gp) + (n + 64) * 2.0 ** -53 * ref.gp_abs
    print(what, "grad_params", got, "float64", ref.gp, "allowed", tol)
    assert (np.abs(got - ref.gp) <= tol).all() and (ref.gp_abs > 0).all(), (got, ref.gp, tol)


CASES = [("above", 4, 4, True), ("inside", 4, 4, False), ("tilted", 4, 4, True), ("above", 1, 1, False), ("inside", 32, 3, True),
         ("tilted", 32, 1, False), ("above", 4, 3, True)]


@pytest.mark.parametrize("name,steps,spp,weighted", CASES)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, name, steps, spp, weighted):
    sc = _scene(hf, oracle)
    n = sc.n - sc.n % spp
    wv = _Wave(hf, sc, 0, n)
    M, lights, J = sc.media[name], sc.lights, len(sc.lights)
    x = R.inputs(n, spp, J)
    w = _cu(x.w) if weighted else None
    img, val, bits = wv.forward(M, lights, K=steps, spp=spp, w=w)
    b = _np(bits).astype(np.uint32)
    if steps == K:
        assert np.array_equal(b, _np(_bits(hf, sc, name)).astype(np.uint32)[:, :n])
    a = (M, lights, wv.np["o"], wv.np["d"], wv.np["t"], x.w if weighted else None, b, steps, SEED)
    rimg, rval = R.forward(*a, spp=spp)
    assert np.abs(rval).max() <= 1.0 and np.abs(rval).max() > 1e-3
    _check(val, rval, "value"); _check(img, rimg, "image")
    assert not _np(val)[b == 0].any()                                                        # exact zeros where no bit is set
    gw, gt, gp = wv.adjoint(M, lights, bits, _cu(x.gi), _cu(x.gv), K=steps, spp=spp, w=w)
    ref = R.adjoint(*a, spp=spp, grad_image=x.gi, grad_value=x.gv)
    _check(gw, ref.gw, "grad_weight"); _check(gt, ref.gt, "grad_t")
    none = (b == 0).all(0)
    assert not _np(gw)[none].any() and not _np(gt)[none].any() and not _np(gt)[~np.isfinite(wv.np["t"])].any()
    _check_params(gp, ref, n, "%s K=%d spp=%d" % (name, steps, spp))
    dw = _cu(x.dw) if weighted else None
    dimg, dval = wv.tangent(M, lights, bits, dw, _cu(x.dt), _cu(x.dp), K=steps, spp=spp, w=w)
    rdimg, rdval = R.tangent(*a, spp=spp, dw=x.dw if weighted else None, dt=x.dt, d_params=x.dp)
    _check(dval, rdval, "dvalue"); _check(dimg, rdimg, "dimage")
    # (e) <J u, v> = <u, J^T v> on the device, the bound built from the tolerances above
    lhs = [(_np(dimg), x.gi), (_np(dval), x.gv)]
    rhs = [(_np(gt), x.dt), (_np(gp), x.dp)] + ([(_np(gw), x.dw)] if weighted else [])
    bound = sum(((RTOL * np.abs(np.asarray(p, np.float64)) + ATOL) * np.abs(q)).sum() for p, q in lhs + rhs)
    gap = transposition_gap(lhs, rhs)
    print("transposition gap", gap, "bound", bound)
    assert gap <= bound


def test_autograd_reaches_the_heights_through_t_and_forward_mode_agrees(hf, oracle):
    sc = _scene(hf, oracle)
    M, name = sc.media["above"], "above"
    x = R.inputs(sc.n, 4, 2, seed=7)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=True)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    sigma = torch.tensor(M.sigma_t, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(M.g, dtype=torch.float64, requires_grad=True)
    E = [torch.tensor(L.irradiance, dtype=torch.float64, requires_grad=True) for L in sc.lights]
    albedo = torch.tensor(M.albedo, dtype=torch.float64, requires_grad=True)
    med = hf.Medium(sigma, albedo, g, top_origin=M.top_origin, top_normal=M.top_normal)
    lights = [hf.DirectionalLight(L.to_light, e) for L, e in zip(sc.lights, E)]
    img, bits = hf.medium_lighting(shape, si, sc.ray, lights, med, spp=4, num_steps=K, seed=SEED, return_visibility=True)
    assert torch.equal(bits, _bits(hf, sc, name))
    (img * _cu(x.gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    b = _np(bits).astype(np.uint32)
    ref = R.adjoint(M, sc.lights, sc.o, sc.d, sc.t, None, b, K, SEED, spp=4, grad_image=x.gi)
    _check_params(torch.stack([sigma.grad, albedo.grad, g.grad] + [e.grad for e in E]), ref, sc.n, "autograd")
    # the heights: the checked grad_t row fed through the existing adjoint by hand
    _, gt, _ = _Wave(hf, sc).adjoint(M, sc.lights, bits, _cu(x.gi), None, spp=4, want=(False, True, False))
    _check(gt, ref.gt, "grad_t")
    ybar = torch.zeros((18, sc.n), device="cuda")
    ybar[0] = gt
    shape2 = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=True)
    gh = _np(shape2.adjoint(sc.ray, shape2.ray_intersect_preliminary(sc.ray), ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("dL/dheight: relative L2 difference of backward() and the adjoint by hand", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= 1e-5, err      # the same kernel on the same row; float atomics in another order
    # forward mode against reverse mode: <J u, v> with u = (dt, dsigma), v = gi
    with fwAD.dual_level():
        si2 = hf.SurfaceInteraction3f()
        si2.p, si2.n, si2.sh_frame = sc.si.p, sc.si.n, sc.si.sh_frame
        si2.t = fwAD.make_dual(sc.si.t.detach(), _cu(x.dt))
        med2 = hf.Medium(fwAD.make_dual(torch.tensor(M.sigma_t, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64)), M.albedo,
                         M.g, top_origin=M.top_origin, top_normal=M.top_normal)
        out = hf.medium_lighting(sc.shape, si2, sc.ray, [_light(hf, L) for L in sc.lights], med2, spp=4, num_steps=K, seed=SEED)
        dimg = fwAD.unpack_dual(out).tangent
    lhs = float((_np(dimg).astype(np.float64) * x.gi).sum())
    rhs = float((_np(gt).astype(np.float64) * x.dt).sum() + float(sigma.grad) * 0.3)
    bound = ((RTOL * np.abs(_np(dimg)) + ATOL) * np.abs(x.gi)).sum() + ((RTOL * np.abs(_np(gt)) + ATOL) * np.abs(x.dt)).sum() \
        + RTOL * abs(float(sigma.grad) * 0.3)
    print("forward mode", lhs, "reverse mode", rhs, "bound", bound)
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0


def test_repeatability_empty_and_ineligible_wavefronts(hf, oracle):
    sc = _scene(hf, oracle)
    M, lights = sc.media["inside"], sc.lights
    x = R.inputs(sc.n, 4, 2)
    wv = _Wave(hf, sc)
    runs = []
    for _ in range(2):
        img, val, bits = wv.forward(M, lights, spp=4, w=_cu(x.w))
        gw, gt, gp = wv.adjoint(M, lights, bits, _cu(x.gi), _cu(x.gv), spp=4, w=_cu(x.w))
        dimg, dval = wv.tangent(M, lights, bits, _cu(x.dw), _cu(x.dt), _cu(x.dp), spp=4, w=_cu(x.w))
        runs.append((img, val, bits, gw, gt, gp, dimg, dval))
    for p, q in zip(*runs):
        assert torch.equal(p, q)                                                             # bit for bit, grad_params included
    # n = 0 through the Python entry
    si0, ray0 = hf.SurfaceInteraction3f(), hf.Ray3f(sc.rays[0:3, :0].contiguous(), sc.rays[3:6, :0].contiguous())
    si0.t = sc.si.t[:0]
    img0, val0, vis0 = hf.medium_lighting(sc.shape, si0, ray0, [_light(hf, L) for L in lights], _medium(hf, M), return_value=True,
                                          return_visibility=True)
    assert img0.shape == (2, 0) and val0.shape == (2, 0) and vis0.shape == (2, 0)
    # camera and rays above the top, heading up: nothing is eligible, every output is an exact zero
    n = 512 + 37
    o = np.stack([np.linspace(-1, 1, n), np.zeros(n), np.full(n, 4.0)])
    d = np.repeat(np.array([[0.1], [0.0], [1.0]]) / np.sqrt(1.01), n, 1)
    up = _Wave(hf, sc, o=o, d=d, t=np.full(n, np.inf))
    assert not R.segment(M, up.np["o"], up.np["d"], up.np["t"]).elig.any()
    img, val, bits = up.forward(M, lights)
    gw, gt, gp = up.adjoint(M, lights, bits, _cu(x.gv[:, :n].copy()), None)
    dimg, dval = up.tangent(M, lights, bits, None, _cu(x.dt[:n].copy()), _cu(x.dp))
    for z in (img, val, bits, gw, gt, gp, dimg, dval):
        assert not z.any()


@pytest.mark.parametrize("n,spp", [(1, 1), (63, 1), (257, 1), (3 * 151, 3), (4 * 65, 4)])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, n, spp):
    sc = _scene(hf, oracle)
    M, lights, J, G = sc.media["tilted"], sc.lights, 2, 64
    lo = 16384 + 4096                                       # in the second wavefront: hits and misses
    wv = _Wave(hf, sc, lo, lo + n)
    x = R.inputs(n, spp, J)
    full = wv.forward(M, lights, spp=spp)
    b = _np(full[2]).astype(np.uint32)
    rimg, rval = R.forward(M, lights, wv.np["o"], wv.np["d"], wv.np["t"], None, b, K, SEED, spp=spp)
    _check(full[1], rval, "value"); _check(full[0], rimg, "image")
    lib, head = hf._capi.lib(), wv._head(M, lights, spp, None, K, SEED, None)
    # guard bands around every output row: one buffer of J rows of n elements, G guard elements before and after
    def band(m, dtype=torch.float32):
        buf = torch.full((1, J * m + 2 * G), GUARD, device="cuda").to(dtype)
        return buf, buf.data_ptr() + 4 * G
    bi, pi = band(n // spp); bv, pv = band(n); bb, pb = band(n, torch.int32)
    hf._capi.check(lib.hf_medium_lighting(sc.shape._h, *head, pi, pv, pb, None))
    torch.cuda.synchronize()
    assert intact(bi, J * (n // spp), G) and intact(bv, J * n, G) and intact(bb, J * n, G)
    assert torch.equal(bv[0, G:G + J * n].reshape(J, n), full[1]) and torch.equal(bb[0, G:G + J * n].reshape(J, n), full[2])
    bw, pw = band(n); bt, pt = band(n); bp, pp = band(R.PARAMS + J)
    ws = torch.empty(lib.hf_medium_workspace_floats(J), device="cuda")
    gi, gv = _cu(x.gi), _cu(x.gv)
    hf._capi.check(lib.hf_medium_lighting_adjoint(*head, full[2].data_ptr(), gi.data_ptr(), gv.data_ptr(), pw, pt, None, None, None))
    bp[0, G:G + R.PARAMS + J] = 0.0
    hf._capi.check(lib.hf_medium_lighting_adjoint(*head, full[2].data_ptr(), gi.data_ptr(), gv.data_ptr(), None, None, pp, ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert intact(bw, n, G) and intact(bt, n, G) and (bp[0, :G] == GUARD).all() and (bp[0, G + R.PARAMS + J:] == GUARD).all()
    ref = R.adjoint(M, lights, wv.np["o"], wv.np["d"], wv.np["t"], None, b, K, SEED, spp=spp, grad_image=x.gi, grad_value=x.gv)
    _check(bw[0, G:G + n], ref.gw, "grad_weight")
    _check(bt[0, G:G + n], ref.gt, "grad_t")
    if ref.gp_abs.all():
        _check_params(bp[0, G:G + R.PARAMS + J], ref, n, "n=%d" % n)
    bdi, pdi = band(n // spp); bdv, pdv = band(n)
    dt, dp = _cu(x.dt), _cu(x.dp)
    hf._capi.check(lib.hf_medium_lighting_tangent(*head, full[2].data_ptr(), None, dt.data_ptr(), dp.data_ptr(), pdi, pdv, None))
    torch.cuda.synchronize()
    assert intact(bdi, J * (n // spp), G) and intact(bdv, J * n, G)
    # each output NULL in turn: the others are what they were
    for drop in range(3):
        want = tuple(i != drop for i in range(3))
        got = wv.forward(M, lights, spp=spp, want=want)
        for i in range(3):
            assert got[i] is None if i == drop else (torch.equal(got[i], full[i]) if (i or spp != 3) else
                                                     torch.allclose(got[i], full[i], rtol=RTOL, atol=ATOL))
    a = wv.adjoint(M, lights, full[2], gi, gv, spp=spp)
    for drop in range(3):
        got = wv.adjoint(M, lights, full[2], gi, gv, spp=spp, want=tuple(i != drop for i in range(3)))
        assert all(got[i] is None if i == drop else torch.equal(got[i], a[i]) for i in range(3))
    tg = wv.tangent(M, lights, full[2], None, dt, dp, spp=spp)
    for drop in range(2):
        got = wv.tangent(M, lights, full[2], None, dt, dp, spp=spp, want=tuple(i != drop for i in range(2)))
        assert all(got[i] is None if i == drop else torch.equal(got[i], tg[i]) for i in range(2))


@contextlib.contextmanager
def _grid(blocks):
    """HF_FORCE_GRID = blocks for the launches inside; restored afterwards (tests/test_gpu_grid_stride.py's hook)"""
    old = os.environ.get("HF_FORCE_GRID")
    os.environ["HF_FORCE_GRID"] = str(blocks)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("HF_FORCE_GRID", None)
        else:
            os.environ["HF_FORCE_GRID"] = old


def test_a_forced_grid_loops_the_adjoint(hf, oracle):
    """HF_FORCE_GRID = C with n = 256 C 3 + 256 + 37: every lane of the adjoint loops at least three times, the last round
    is ragged; the per-sample rows are bitwise those of the unforced launch, the reduced numbers the same sums in another
    order, within the tolerance of the float64 sums"""
    sc = _scene(hf, oracle)
    Cb = 5
    n = 256 * Cb * 3 + 256 + 37
    lo = 16384 - n // 2                                     # across the seam of the two wavefronts
    wv = _Wave(hf, sc, lo, lo + n)
    M, lights = sc.media["above"], sc.lights
    x = R.inputs(n, 1, 2)
    lib = hf._capi.lib()
    bits = wv.forward(M, lights, want=(False, False, True))[2]
    assert lib.hf_grid_blocks(n, 2) == -(-n // 256)
    free = wv.adjoint(M, lights, bits, _cu(x.gi), _cu(x.gv), w=_cu(x.w))
    with _grid(Cb):
        blocks = lib.hf_grid_blocks(n, 2)
        assert blocks == Cb and blocks < n / (256 * 3), (blocks, n)
        forced = wv.adjoint(M, lights, bits, _cu(x.gi), _cu(x.gv), w=_cu(x.w))
    assert torch.equal(free[0], forced[0]) and torch.equal(free[1], forced[1])
    ref = R.adjoint(M, lights, wv.np["o"], wv.np["d"], wv.np["t"], x.w, _np(bits).astype(np.uint32), K, SEED, grad_image=x.gi, grad_value=x.gv)
    _check(forced[0], ref.gw, "grad_weight"); _check(forced[1], ref.gt, "grad_t")
    for got in (free, forced):
        _check_params(got[2], ref, n, "forced grid")


def test_inverse_fog_example_descends(hf):
    import inverse_fog
    hist, start, end, target = inverse_fog.run(size=32, steps=12, verbose=False)
    print("loss", hist[0], "->", hist[-1], "sigma_t", start[0], "->", end[0], "target", target[0])
    assert np.isfinite(hist[-1]) and hist[-1] < hist[0], (hist[0], hist[-1])
    assert abs(end[0] - target[0]) < abs(start[0] - target[0])

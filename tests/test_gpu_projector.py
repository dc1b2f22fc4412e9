"""Projector lighting on the GPU (hf_projector_rays, hf_projector_lighting, _adjoint, _tangent) on row_helpers.base_scene:
sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0),
both face_normals modes, the two projectors of tests/projector_ref.py (`above`: the frustum's border crosses the terrain;
`side`: most traced samples are in shadow), a 16 x 8 texture under both wraps and no texture.
  (1) vis against the two-call sequence hf_projector_rays + hf_ray_test bit for bit, the masks and the rays against the
      restatement, the lit and occluded shares;
  (2) image, value, uv, every gradient (the 14 reduced numbers among them) and the tangents against the restatement fed
      with the GPU's visibility; the composition the parent offers (hf_sensor_project on a film of TW x TH, Bitmap.eval,
      torch arithmetic); the transposition gap on the device through backward and jvp;
  (3) the 14 reduced numbers over 301 rows; the chain projector_lighting -> loss -> backward -> dL/dheight;
  (4) n = 0, an all-miss wavefront, odd sizes with guard bands, every optional pointer NULL in turn, spp 3, HF_FORCE_GRID,
      bitwise repeatability, a captured graph;
  (5) a projector that faces away, a flat field, a 1 x 1 and a 5 x 3 texture;
  (6) examples/inverse_projector.py descends in both modes.

Tolerances (scripts/projector_f32_error.py computes them on the CPU, profiles/projector/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records and
visibility, over both projectors, both wraps and no texture, by at most the figures of F32 below (projector_ref.errors:
per-lane quantities as the largest difference over max(1, the largest value), uv absolute, grad_tex and the 14 reduced
numbers as the L2 norm of the difference over the L2 norm of the float64 result).  The GPU is allowed four times that:
another operation order.  Samples on which rounding may decide a mask (a deciding quantity within MARGIN) are left out of
the comparisons, at most UNSURE_CAP of the samples (the restatement alone leaves out at most 6.1e-5); lanes whose texel
coordinate is within BORDER of a border between two cells of the lookup are taken out of the visibility the derivative
kernels and the restatement are given."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import projector_ref as P
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, _rel, base_scene, guarded, intact, rows, sub, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
TW, TH = P.TEX
SPP = 4
F32 = {"image": 4.77e-7, "value": 9.97e-7, "uv": 4.51e-7, "dimage": 1.59e-6, "dvalue": 1.96e-6, "grad_sh_n": 1.02e-6,
       "grad_p": 3.19e-6, "grad_weight": 9.14e-7, "grad14": 3.08e-6, "grad_tex": 1.53e-6}
# the maxima of profiles/projector/f32_error.json, cut off after three digits
TOL = {k: 4 * v for k, v in F32.items()}
TEX = P.textures(TW, TH)["random"]
WRAPS = {"clamp": P.CLAMP, "repeat": P.REPEAT}
COMBOS = [(oi, fn, name) for oi in range(2) for fn in (True, False) for name in sorted(P.PROJECTORS)]
VARIANTS = (("clamp", True), ("repeat", True), ("repeat", False))          # (wrap, textured)


def _projector(hf, pr, tex=None, wrap="repeat", **kw):
    """the hf_amd.Projector of the restatement's pr; tex: a device tensor (None: uniform, with pr's resolution for the aspect)"""
    a = dict(to_world=pr.to_world, fov=pr.fov, scale=pr.scale)
    a.update(kw)
    return hf.Projector(a["to_world"], a["fov"], tex, scale=a["scale"], wrap=wrap, resolution=None if tex is not None else pr.res)


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), ORIGINS[oi], face_normals)
        sc.eligible, _ = P.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
        sc.runs = {}
        _SCENES[key] = sc
    return _SCENES[key]


def _run(hf, sc, name):
    """one projector on a scene: the GPU's visibility and the restatement's masks, once"""
    if name not in sc.runs:
        r = P.types.SimpleNamespace(pr=P.PROJECTORS[name]())
        r.proj = _projector(hf, r.pr)
        _, vis = hf.projector_lighting(sc.shape, sc.si, sc.ray, r.proj, albedo=P.ALBEDO, spp=SPP, return_visibility=True)
        r.vis = _np(vis).astype(bool)
        r.traced, r.unsure = P.traced(r.pr, sc.np["p"], sc.np["sh_n"], sc.np["d"], sc.np["t"])
        assert r.unsure.mean() <= UNSURE_CAP, r.unsure.mean()                # (asserted on the restatement before comparing)
        r.sure = ~r.unsure
        r.pix = r.sure.reshape(-1, SPP).all(1)
        r.m = P.mapping(r.pr, sc.np["p"])
        with np.errstate(invalid="ignore"):
            r.lanes = sc.hit & (r.m.ref[2] > 0)
        sc.runs[name] = r
    return sc.runs[name]


class _Wave:
    """the device rows of the samples [lo, hi) of a scene and the C calls on them"""

    def __init__(self, hf, sc, lo=0, hi=None):
        hi = sc.n if hi is None else hi
        cut = lambda v: v.detach()[..., lo:hi].contiguous()
        self.hf, self.shape, self.n = hf, sc.shape, hi - lo
        self.p, self.nr, self.sn, self.d, self.t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
        self.np = {k: _np(v) for k, v in (("p", self.p), ("n", self.nr), ("sh_n", self.sn), ("d", self.d), ("t", self.t))}
        self.lib, self.check = hf._capi.lib(), hf._capi.check
        self.ws = torch.empty(self.lib.hf_projector_workspace_floats(), device="cuda")

    def mid(self, pr, w, tex, wrap, res=None):
        S = self.hf._capi.hf_projector_t((C.c_double * 12)(*pr.to_world.reshape(-1).tolist()), pr.fov, pr.scale)
        res = pr.res if res is None else res
        return (None if w is None else w.data_ptr(), S, res[0], res[1], None if tex is None else tex.data_ptr(), wrap, P.ALBEDO)

    def head(self, spp):
        return (self.n, spp, rows(self.p), rows(self.sn), rows(self.d), self.t.data_ptr())

    def forward(self, spp, mid, image=None, value=None, vis=None, uv=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_projector_lighting(self.shape._h, self.n, spp, rows(self.p), rows(self.nr), rows(self.sn), rows(self.d),
                                                  self.t.data_ptr(), *mid, image, value, vis, uv, s))

    def adjoint(self, spp, mid, vis, gi, gv, gn=None, gp=None, gw=None, gt=None, g12=None, gf=None, gs=None, ws=True):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_projector_lighting_adjoint(*self.head(spp), *mid, vis, gi, gv, gn, gp, gw, gt, g12, gf, gs,
                                                          self.ws.data_ptr() if ws else None, s))

    def tangent(self, spp, mid, vis, dn=None, dp=None, dw=None, dtex=None, dtw=None, dfov=None, dscale=None, dimage=None, dvalue=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_projector_lighting_tangent(*self.head(spp), *mid, vis, dn, dp, dw, dtex, dtw, dfov, dscale, dimage,
                                                          dvalue, s))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _derivatives(wv, pr, x, tex, wrap, vis, spp, weighted=True):
    """the adjoint and the tangent through the C ABI under the inputs x and the given visibility: a namespace with dimage,
    dvalue, gn, gp, gw, gtex, g14 as numpy"""
    n = wv.n
    w = _cu(x.w) if weighted else None
    mid = wv.mid(pr, w, tex, wrap)
    v8 = _cu(vis.astype(np.uint8))
    z = lambda *s: torch.zeros(s, device="cuda")
    gn, gp, gw, g12, gf, gs = z(3, n), z(3, n), z(n), z(12), z(1), z(1)
    gt = z(TH, TW) if tex is not None else None
    gi, gv = _cu(x.gi), _cu(x.gv)
    wv.adjoint(spp, mid, v8.data_ptr(), gi.data_ptr(), gv.data_ptr(), rows(gn), rows(gp), gw.data_ptr() if weighted else None, _ptr(gt),
               g12.data_ptr(), gf.data_ptr(), gs.data_ptr())
    dimage, dvalue = z(n // spp), z(n)
    t = [_cu(np.asarray(a, np.float32)) for a in (x.dn, x.dp, x.dw, x.dtex, x.dtw, np.array([x.dfov]), np.array([x.dscale]))]
    wv.tangent(spp, mid, v8.data_ptr(), rows(t[0]), rows(t[1]), t[2].data_ptr() if weighted else None, t[3].data_ptr() if tex is not None else None,
               t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), dimage.data_ptr(), dvalue.data_ptr())
    torch.cuda.synchronize()
    g = P.types.SimpleNamespace(dimage=_np(dimage), dvalue=_np(dvalue), gn=_np(gn), gp=_np(gp), gtex=None if gt is None else _np(gt),
                                g14=np.concatenate([_np(g12), _np(gf), _np(gs)]))
    g.gw = _np(gw) if weighted else None
    return g


@pytest.mark.parametrize("oi,face_normals,name", COMBOS)
def test_visibility_equals_the_two_call_sequence_bit_for_bit_and_the_masks_the_restatement(hf, oracle, oi, face_normals, name):
    sc = _scene(hf, oracle, oi, face_normals)
    r = _run(hf, sc, name)
    ray = hf.projector_rays(sc.si, sc.ray, r.proj)
    tr = _np(ray.maxt >= 0)
    two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
    assert np.array_equal(r.vis, two), int((r.vis != two).sum())
    assert np.array_equal(tr[r.sure], r.traced[r.sure])
    assert not r.vis[~sc.eligible & r.sure].any()
    o, w, maxt, _ = P.rays(r.pr, sc.np["p"], sc.np["n"], sc.np["sh_n"], sc.np["d"], sc.np["t"])
    both = tr & r.traced
    assert np.abs(_np(ray.o) - o)[:, both].max() <= 1e-6 and np.abs(_np(ray.d) - w)[:, both].max() <= 2e-6
    assert np.abs(_np(ray.maxt) - maxt)[both].max() <= 1e-5 * maxt[both].max()
    assert not _np(ray.o)[:, ~tr].any() and not _np(ray.d)[:, ~tr].any() and (_np(ray.maxt)[~tr] == -1).all()
    lit = r.m.lit[sc.eligible].mean()
    occluded = 1.0 - r.vis.sum() / tr.sum()
    print(name, "unsure", r.unsure.mean(), "lit of eligible", lit, "traced of eligible", tr[sc.eligible].mean(), "occluded of traced", occluded,
          "smallest ref.z", r.m.ref[2][tr].min())
    if name == "above":
        assert 0.15 <= lit <= 0.95, lit
    else:
        assert 0.3 <= occluded <= 0.85, occluded
    # the texture and the wrap do not enter the visibility
    _, v2 = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, r.pr, _cu(TEX), "clamp"), spp=SPP, return_visibility=True)
    assert np.array_equal(_np(v2).astype(bool), r.vis)


def _composition(hf, sc, r, tex, wrap, w):
    """what the parent offers: hf_sensor_project on a film of TW x TH -> Bitmap.eval -> torch arithmetic (float64) with the
    same visibility.  Returns (value [n], uv [2, n]) as numpy"""
    pr = r.pr
    cam = hf.PerspectiveCamera(pr.to_world, pr.fov, film=(TW, TH), near_clip=1e-3, far_clip=1e4)
    pos, _, _ = cam.sample_direction(sc.si.p.detach())
    I = hf.Bitmap(tex, wrap=wrap).eval(pos).double() if tex is not None else 1.0
    A, c = (torch.as_tensor(a, device="cuda") for a in (pr.to_world[:, :3], pr.to_world[:, 3]))
    u = c[:, None] - sc.si.p.detach().double()
    z = (torch.linalg.inv(A) @ -u)[2]
    G = (sc.si.sh_frame.n.detach().double() * u).sum(0) / z ** 3
    value = w.double() * (P.ALBEDO * pr.scale) * I * G
    value = torch.where(_cu(r.vis), value, torch.zeros_like(value))
    return _np(value), _np(pos) / np.array([[TW], [TH]])


@pytest.mark.parametrize("oi,face_normals,name", COMBOS)
def test_values_uv_gradients_and_tangents_against_the_restatement(hf, oracle, oi, face_normals, name):
    sc = _scene(hf, oracle, oi, face_normals)
    r = _run(hf, sc, name)
    pr = r.pr
    x = P.inputs(sc.n, SPP, (TH, TW))
    wv = _Wave(hf, sc)
    steady = P.steady(pr, sc.np["p"], r.vis) & r.sure
    worst = {k: 0.0 for k in TOL}
    for wrap, textured in VARIANTS:
        tex = _cu(TEX) if textured else None
        img, val, vis, uv = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, pr, tex, wrap), albedo=P.ALBEDO, spp=SPP,
                                                  weight=_cu(x.w), return_value=True, return_visibility=True, return_uv=True)
        assert np.array_equal(_np(vis).astype(bool), r.vis)
        assert not _np(val)[~r.vis].any()                                           # exactly 0 where nothing is seen
        ref = P.evaluate(pr, wv.np, x, TEX if textured else None, WRAPS[wrap], steady, SPP)
        ref.image, ref.value, ref.uv = P.forward(pr, wv.np["p"], wv.np["sh_n"], x.w, TEX if textured else None, WRAPS[wrap], P.ALBEDO,
                                                 r.vis, SPP)
        # (without a texture nothing depends on the field of view once the masks are held: column 12 is exactly 0)
        assert ref.value.max() > 0.3 and np.abs(np.delete(ref.g14, () if textured else 12)).min() > 0
        got = _derivatives(wv, pr, x, tex, WRAPS[wrap], steady, SPP)
        assert textured or (ref.g14[12] == 0 and got.g14[12] == 0)
        got.image, got.value, got.uv = (_np(a).copy() for a in (img, val, uv))
        for ns in (got, ref):                                                       # (samples that rounding may decide)
            ns.value = np.where(r.sure, ns.value, 0.0)
            ns.image = np.where(r.pix, ns.image, 0.0)
        for k in ("gn", "gp", "gw", "dvalue"):
            assert not getattr(got, k)[..., ~steady].any()                          # exact zeros where vis = 0
        err = P.errors(got, ref, r.lanes & r.sure)
        assert not _np(uv)[:, sc.hit & ~r.lanes].any()                              # zeros behind the projector
        # the composition the parent offers, within the same margins
        cval, cuv = _composition(hf, sc, r, tex, wrap, _cu(x.w))
        err["value"] = max(err["value"], P.err_abs(np.where(r.sure, cval, 0.0), ref.value))
        err["uv"] = max(err["uv"], float(np.abs(cuv - ref.uv)[:, r.lanes & r.sure].max()))
        print(wrap, textured, {k: "%.3g" % v for k, v in err.items()})
        for k, v in err.items():
            worst[k] = max(worst[k], v)
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


def _leaf(hf, sc, sh_n=None, p=None):
    si = hf.SurfaceInteraction3f()
    si.n, si.t = sc.si.n.detach(), sc.si.t.detach()
    si.p = sc.si.p.detach().clone().requires_grad_(True) if p is None else p
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True) if sh_n is None else sh_n)
    return si


@pytest.mark.parametrize("name", sorted(P.PROJECTORS))
def test_transposition_on_the_device_through_backward_and_jvp_and_repeatability(hf, oracle, name):
    """<J u, v> = <u, J^T v> through the public function: forward_ad against backward, both sides float32 results added up in
    float64, each side within its tolerance of the exact bilinear form; and two runs give the same bits (all but grad_tex)"""
    sc = _scene(hf, oracle, 0, False)
    r = _run(hf, sc, name)
    pr = r.pr
    x = P.inputs(sc.n, SPP, (TH, TW))
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    runs = []
    for _ in range(2):
        si, wt, td = _leaf(hf, sc), _cu(x.w).requires_grad_(True), _cu(TEX).requires_grad_(True)
        tw, fov, scale = f64(pr.to_world).requires_grad_(True), f64(pr.fov).requires_grad_(True), f64(pr.scale).requires_grad_(True)
        img, val, vis = hf.projector_lighting(sc.shape, si, sc.ray, _projector(hf, pr, td, "repeat", to_world=tw, fov=fov, scale=scale),
                                              albedo=P.ALBEDO, spp=SPP, weight=wt, return_value=True, return_visibility=True)
        ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
        with fwAD.dual_level():
            sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
            dual = _projector(hf, pr, fwAD.make_dual(_cu(TEX), _cu(x.dtex)), "repeat",
                              to_world=fwAD.make_dual(f64(pr.to_world), f64(x.dtw).reshape(3, 4)),
                              fov=fwAD.make_dual(f64(pr.fov), f64(x.dfov)), scale=fwAD.make_dual(f64(pr.scale), f64(x.dscale)))
            ti, tv = hf.projector_lighting(sc.shape, sid, sc.ray, dual, albedo=P.ALBEDO, spp=SPP,
                                           weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), return_value=True)
            ti, tv = fwAD.unpack_dual(ti).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        assert tw.grad.shape == (3, 4) and fov.grad.shape == () and scale.grad.shape == ()
        runs.append((vis.clone(), img.detach().clone(), val.detach().clone(), si.sh_frame.n.grad.clone(), si.p.grad.clone(), wt.grad.clone(),
                     tw.grad.clone(), fov.grad.clone(), scale.grad.clone(), ti, tv, td.grad.clone()))
    for a, b in zip(runs[0][:-1], runs[1][:-1]):
        assert torch.equal(a, b)                                                    # everything but grad_tex: bitwise
    assert _rel(_np(runs[0][-1]), _np(runs[1][-1]).astype(np.float64)) <= 1e-5     # (float atomics: the order differs)
    _, _, _, gn, gp, gw, gtw, gfov, gsc, ti, tv, gtex = (_np(a) for a in runs[0])
    gap = transposition_gap(((ti, x.gi), (tv, x.gv)),
                            ((gn, x.dn), (gp, x.dp), (gw, x.dw), (gtex, x.dtex), (gtw.reshape(-1), x.dtw), (gfov, x.dfov), (gsc, x.dscale)))
    size = np.linalg.norm(tv) * np.linalg.norm(x.gv) + np.linalg.norm(ti) * np.linalg.norm(x.gi)
    print("transposition gap", gap, "size", size)
    assert size > 0 and gap <= (TOL["dvalue"] + TOL["grad_p"]) * size, (gap, size)


def _busiest(vis, n):
    """the start (a multiple of 64) of the window of n samples that holds the most visible ones"""
    c = np.concatenate([[0], np.cumsum(vis)])
    starts = np.arange(0, len(vis) - n + 1, 64)
    return int(starts[np.argmax(c[starts + n] - c[starts])])


@pytest.mark.parametrize("name", sorted(P.PROJECTORS))
def test_the_fourteen_reduced_numbers_over_301_rows(hf, oracle, name):
    """n = 301 (more than one block, odd), spp 1: to_world's 12, fov's and scale's against the float64 reverse sweep"""
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, name)
    lo = _busiest(r.vis, 301)
    wv = _Wave(hf, sc, lo, lo + 301)
    x = P.inputs(301, 1, (TH, TW), seed=8)
    vis = P.steady(r.pr, wv.np["p"], r.vis[lo:lo + 301]) & r.sure[lo:lo + 301]
    assert vis.sum() >= 20
    for wrap, textured in VARIANTS:
        got = _derivatives(wv, r.pr, x, _cu(TEX) if textured else None, WRAPS[wrap], vis, 1)
        ref = P.adjoint(r.pr, wv.np["p"], wv.np["sh_n"], x.w, TEX if textured else None, WRAPS[wrap], P.ALBEDO, vis, 1, x.gi, x.gv)
        err = P.err_l2(got.g14, ref.g14)
        print(name, wrap, textured, "grad14", err, ref.g14)
        assert np.abs(np.delete(ref.g14, () if textured else 12)).min() > 0 and err <= TOL["grad14"], err


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """projector_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n and grad_p (fed
    with the GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint,
    which tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: four times the float32 error of
    grad_p (the larger of the two gradients' errors) + the 1e-5 of the sky row's chain."""
    sc = _scene(hf, oracle, 0, face_normals)
    r = _run(hf, sc, "side")
    x = P.inputs(sc.n, SPP, (TH, TW))
    keep = (P.steady(r.pr, sc.np["p"], r.vis) | ~r.vis) & r.sure
    gi = np.where(keep.reshape(-1, SPP).all(1), x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.projector_lighting(shape, si, sc.ray, _projector(hf, r.pr, _cu(TEX), "repeat"), albedo=P.ALBEDO, spp=SPP,
                                     return_visibility=True)
    assert np.array_equal(_np(vis).astype(bool), r.vis)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = P.adjoint(r.pr, _np(si.p), _np(si.sh_frame.n), None, TEX, P.REPEAT, P.ALBEDO, r.vis, SPP, gi)
    rr = _np(sc.rays)
    if face_normals:
        t, u, v, prim = sc.field.ray_intersect_preliminary(rr)
        gh = sc.field.adjoint(rr, t, u, v, prim, {"sh_n": g.gn.astype(np.float32), "p": g.gp.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[1:4] = _cu(g.gp.astype(np.float32)); ybar[9:12] = _cu(g.gn.astype(np.float32))
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= TOL["grad_p"] + 1e-5, err


def test_empty_and_all_miss_wavefronts_and_refusals(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "above")
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, val0, vis0, uv0 = hf.projector_lighting(sc.shape, si0, ray0, r.proj, spp=SPP, return_value=True, return_visibility=True,
                                                  return_uv=True)
    assert img0.shape == (0,) and val0.shape == (0,) and vis0.shape == (0,) and uv0.shape == (2, 0)
    img0.sum().backward()
    assert len(hf.projector_rays(si0, ray0, r.proj)) == 0
    # a wavefront with no eligible sample: rays that leave the terrain behind, and hits seen from behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    for s, ry in ((sim, up), (sc.si, up)):
        imgm, vism = hf.projector_lighting(sc.shape, s, ry, r.proj, spp=SPP, return_visibility=True)
        assert not bool(imgm.any()) and not bool(vism.any())
    with pytest.raises(hf.HfError):
        hf.projector_lighting(sc.shape, sc.si, sc.ray, r.proj, spp=3)
    with pytest.raises(hf.HfError):
        hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, r.pr, fov=180.0), spp=SPP)


@pytest.mark.parametrize("spp", [1, 3])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, spp):
    """n = spp * 151 (two whole workgroup batches of 64 and a part of one; spp 3 is no power of two: the film's other
    paths), guard values around every output row, and every optional pointer NULL in turn"""
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "side")
    pr = r.pr
    n, G = spp * 151, 96
    lo = _busiest(r.vis, n)
    wv = _Wave(hf, sc, lo, lo + n)
    x = P.inputs(n, spp, (TH, TW), seed=9)
    w, tex = _cu(x.w), _cu(TEX)
    mid = wv.mid(pr, w, tex, P.REPEAT)
    sure = r.sure[lo:lo + n]

    def forward(skip=None, m=mid):
        image, ip = guarded(n // spp, G); value, vp = guarded(n, G); uv, up = guarded(n, G, 2)
        vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        wv.forward(spp, m, None if skip == "image" else ip[0], None if skip == "value" else vp[0],
                   None if skip == "vis" else vis.data_ptr() + G, None if skip == "uv" else up)
        return {"image": image, "value": value, "vis": vis, "uv": uv}
    full = forward()
    assert intact(full["image"], n // spp, G) and intact(full["value"], n, G) and intact(full["uv"], n, G)
    assert bool((full["vis"][:G] == 0x5A).all()) and bool((full["vis"][G + n:] == 0x5A).all())
    vis8 = full["vis"][G:G + n].contiguous()
    vis = _np(vis8).astype(bool)
    assert np.array_equal(vis, r.vis[lo:lo + n]) and vis.sum() >= 20                # the slice of the whole
    ri, rv, ruv = P.forward(pr, wv.np["p"], wv.np["sh_n"], x.w, TEX, P.REPEAT, P.ALBEDO, vis, spp)
    pix = sure.reshape(-1, spp).all(1)
    assert P.err_abs(np.where(pix, _np(full["image"][0, G:G + n // spp]), 0), np.where(pix, ri, 0)) <= TOL["image"]
    assert P.err_abs(np.where(sure, _np(full["value"][0, G:G + n]), 0), np.where(sure, rv, 0)) <= TOL["value"]
    lanes = r.lanes[lo:lo + n] & sure
    assert np.abs(_np(full["uv"][:, G:G + n]) - ruv)[:, lanes].max() <= TOL["uv"]
    for skip in ("image", "value", "vis", "uv"):
        part = forward(skip)
        for k in full:
            if k == skip:
                assert bool((part[k] == (0x5A if k == "vis" else GUARD)).all())     # untouched
            else:
                assert torch.equal(part[k], full[k])
    # without a weight and without a texture: the same film as with a weight of 1 and a texture of ones
    a = forward(m=wv.mid(pr, None, None, P.REPEAT))
    one_w, one_t = torch.ones(n, device="cuda"), torch.ones((TH, TW), device="cuda")
    b = forward(m=wv.mid(pr, one_w, one_t, P.REPEAT))
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["value"], b["value"]) and torch.equal(a["vis"], b["vis"])
    # the adjoint: all outputs, then each one NULL in turn -- the others are bitwise what they were, grad_tex to rounding
    gi, gv = _cu(x.gi), _cu(x.gv)

    def adjoint(skip=None, gi_=gi, gv_=gv):
        gn, gnp = guarded(n, G, 3); gp, gpp = guarded(n, G, 3); gw, gwp = guarded(n, G)
        z = lambda *s: torch.zeros(s, device="cuda")
        o = {"gn": gn, "gp": gp, "gw": gw, "gt": z(TH, TW), "g12": z(12), "gf": z(1), "gs": z(1)}
        ptr = lambda k, v: None if skip == k else v
        wv.adjoint(spp, mid, vis8.data_ptr(), _ptr(gi_), _ptr(gv_), ptr("gn", gnp), ptr("gp", gpp), ptr("gw", gwp[0]),
                   ptr("gt", o["gt"].data_ptr()), ptr("g12", o["g12"].data_ptr()), ptr("gf", o["gf"].data_ptr()), ptr("gs", o["gs"].data_ptr()))
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("gn", "gp", "gw"))
    assert float(fulla["g12"].abs().min()) > 0 and float(fulla["gf"].abs()) > 0 and float(fulla["gs"].abs()) > 0
    for skip in ("gn", "gp", "gw", "gt", "g12", "gf", "gs"):
        part = adjoint(skip)
        for k in part:
            if k == skip:
                assert bool((part[k] == GUARD).all()) if k in ("gn", "gp", "gw") else not bool(part[k].any())   # untouched
            elif k == "gt":
                assert _rel(_np(part["gt"]), _np(fulla["gt"]).astype(np.float64)) <= 1e-5   # (float atomics: the order differs)
            else:
                assert torch.equal(part[k], fulla[k]), (skip, k)
    # (no reduced gradient wanted: no workspace needed; grad_image or grad_value alone: their sum is the whole)
    gn, gnp = guarded(n, G, 3)
    wv.adjoint(spp, mid, vis8.data_ptr(), gi.data_ptr(), gv.data_ptr(), gnp, ws=False)
    assert torch.equal(gn, fulla["gn"])
    only_i, only_v = adjoint(gv_=None), adjoint(gi_=None)
    for k in ("gn", "g12", "gs"):
        cut = (lambda a: a[:, G:G + n]) if k == "gn" else (lambda a: a)
        s = cut(_np(only_i[k])).astype(np.float64) + cut(_np(only_v[k]))
        assert np.abs(s - cut(_np(fulla[k]))).max() <= 1e-5 * np.abs(cut(_np(fulla[k]))).max()
    # the tangent: every tangent NULL in turn, and their sum is the whole (the map is linear)
    t = {k: _cu(np.asarray(v, np.float32)) for k, v in (("dn", x.dn), ("dp", x.dp), ("dw", x.dw), ("dtex", x.dtex), ("dtw", x.dtw),
                                                        ("dfov", np.array([x.dfov])), ("dscale", np.array([x.dscale])))}

    def tangent(use, image=True, value=True):
        di, dip = guarded(n // spp, G); dv, dvp = guarded(n, G)
        q = lambda k: (rows(t[k]) if k in ("dn", "dp") else t[k].data_ptr()) if k in use else None
        wv.tangent(spp, mid, vis8.data_ptr(), q("dn"), q("dp"), q("dw"), q("dtex"), q("dtw"), q("dfov"), q("dscale"),
                   dip[0] if image else None, dvp[0] if value else None)
        assert (intact(di, n // spp, G) if image else bool((di == GUARD).all())) and (intact(dv, n, G) if value else bool((dv == GUARD).all()))
        return di, dv
    di, dv = tangent(tuple(t))
    assert torch.equal(tangent(tuple(t), value=False)[0], di) and torch.equal(tangent(tuple(t), image=False)[1], dv)
    parts = sum(_np(tangent((k,))[1][0, G:G + n]).astype(np.float64) for k in t)
    assert not bool(tangent(())[1][0, G:G + n].any())
    whole = _np(dv[0, G:G + n]).astype(np.float64)
    assert np.abs(whole - parts).max() <= 8 * TOL["dvalue"] * max(1.0, np.abs(whole).max())   # (eight results, each within its tolerance)
    assert np.abs(_np(di[0, G:G + n // spp]) - whole.reshape(-1, spp).mean(1)).max() <= 1e-6 * max(1.0, np.abs(whole).max())
    # the rays
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    S = mid[1]
    wv.check(wv.lib.hf_projector_rays(n, rows(wv.p), rows(wv.nr), rows(wv.sn), rows(wv.d), wv.t.data_ptr(), S, TW, TH, rop, rdp, rmp[0],
                                      torch.cuda.current_stream().cuda_stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    torch.cuda.synchronize()


class _env:
    """HF_FORCE_GRID = blocks for the launches inside; restored afterwards (tests/test_gpu_grid_stride.py's hook)"""

    def __init__(self, blocks):
        self.blocks = blocks

    def __enter__(self):
        self.old = os.environ.get("HF_FORCE_GRID")
        os.environ["HF_FORCE_GRID"] = str(self.blocks)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("HF_FORCE_GRID", None)
        else:
            os.environ["HF_FORCE_GRID"] = self.old


def test_a_forced_grid_loops_the_adjoint_and_leaves_the_other_kernels_alone(hf, oracle):
    """HF_FORCE_GRID = 3: the adjoint's grid-stride loop runs 22 times per lane on 16384 samples and its slab has 3 rows; the
    per-lane outputs are bitwise the same, the reduced numbers the same sums in another order.  The forward, the tangent
    and the rays kernels take one lane per sample: the hook does not reach them, and their outputs are bitwise the same"""
    sc = _scene(hf, oracle, 0, True)
    r = _run(hf, sc, "side")
    wv = _Wave(hf, sc)
    x = P.inputs(sc.n, SPP, (TH, TW))
    vis = P.steady(r.pr, sc.np["p"], r.vis)
    free = _derivatives(wv, r.pr, x, _cu(TEX), P.REPEAT, vis, SPP)
    ray = hf.projector_rays(sc.si, sc.ray, r.proj)
    with _env(3):
        assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 3
        forced = _derivatives(wv, r.pr, x, _cu(TEX), P.REPEAT, vis, SPP)
        _, v2 = hf.projector_lighting(sc.shape, sc.si, sc.ray, r.proj, albedo=P.ALBEDO, spp=SPP, return_visibility=True)
        ray2 = hf.projector_rays(sc.si, sc.ray, r.proj)
    for k in ("gn", "gp", "gw", "dimage", "dvalue"):
        assert np.array_equal(getattr(free, k), getattr(forced, k)), k
    assert P.err_l2(forced.g14, free.g14.astype(np.float64)) <= 1e-6 and np.abs(free.g14).min() > 0
    assert np.array_equal(_np(v2).astype(bool), r.vis) and torch.equal(ray.maxt, ray2.maxt) and torch.equal(ray.o, ray2.o)


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "side")
    wv = _Wave(hf, sc)
    tex = _cu(TEX)
    mid = wv.mid(r.pr, None, tex, P.REPEAT)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, device="cuda", dtype=dtype)
    img, val, vis, uv = z(sc.n // SPP), z(sc.n), z(sc.n, dtype=torch.uint8), z(2, sc.n)
    gn, gp, g12, gf, gs, dimg, dval = z(3, sc.n), z(3, sc.n), z(12), z(1), z(1), z(sc.n // SPP), z(sc.n)
    gi, ones, d12, one = torch.ones(sc.n // SPP, device="cuda"), torch.ones((3, sc.n), device="cuda"), torch.ones(12, device="cuda"), torch.ones(1, device="cuda")

    def launch():
        for a in (g12, gf, gs):
            a.zero_()                                                    # (accumulated into)
        wv.forward(SPP, mid, img.data_ptr(), val.data_ptr(), vis.data_ptr(), rows(uv))
        wv.adjoint(SPP, mid, vis.data_ptr(), gi.data_ptr(), None, rows(gn), rows(gp), None, None, g12.data_ptr(), gf.data_ptr(), gs.data_ptr())
        wv.tangent(SPP, mid, vis.data_ptr(), rows(ones), rows(ones), None, None, d12.data_ptr(), one.data_ptr(), one.data_ptr(),
                   dimg.data_ptr(), dval.data_ptr())
    outs = (img, val, vis, uv, gn, gp, g12, gf, gs, dimg, dval)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert np.array_equal(_np(vis).astype(bool), r.vis) and float(img.abs().sum()) > 0 and float(g12.abs().min()) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for v in outs:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def _flat(hf, k=24, z=0.5):
    """a flat field z = 0.5 seen straight down from a k x k grid of camera rays over [-0.6, 0.6]^2"""
    shape = hf.Heightfield(heightfield=torch.full((16, 16), 1.0, device="cuda"), max_height=z)
    xs = (torch.arange(k, device="cuda", dtype=torch.float32) + 0.5) / k * 1.2 - 0.6
    py, px = torch.meshgrid(xs, xs, indexing="ij")
    hit = torch.stack([px.reshape(-1), py.reshape(-1), torch.full((k * k,), z, device="cuda")])
    dd = torch.tensor((0.0, 0.0, -1.0), device="cuda")[:, None].expand(3, k * k).contiguous()
    ray = hf.Ray3f((hit - dd).contiguous(), dd)
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid().all()) and float((si.p - hit).abs().max()) <= 1e-6
    return shape, si, ray


def test_a_projector_that_faces_away_lights_nothing_and_a_flat_field_sees_every_traced_sample(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    away = P.projector(P.look_at((0.3, -0.2, 2.0), (0.3, -0.2, 4.0), (0, 1, 0)), 40.0, P.SCALE)     # `above`, looking up
    img, val, vis = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, away), spp=SPP, return_value=True, return_visibility=True)
    assert not bool(vis.any()) and not bool(img.any()) and not bool(val.any())      # exactly 0
    assert bool((hf.projector_rays(sc.si, sc.ray, _projector(hf, away)).maxt == -1).all())
    shape, si, ray = _flat(hf)
    for name in sorted(P.PROJECTORS):
        proj = _projector(hf, P.PROJECTORS[name]())
        _, vis = hf.projector_lighting(shape, si, ray, proj, spp=1, return_visibility=True)
        tr = hf.projector_rays(si, ray, proj).maxt >= 0
        assert torch.equal(vis.bool(), tr) and float(tr.float().mean()) > 0.1       # nothing occludes


@pytest.mark.parametrize("res", [(1, 1), (5, 3)])
def test_small_textures(hf, oracle, res):
    """a 1 x 1 texture (every lookup reads the one texel, under both wraps) and a 5 x 3 one (odd sizes, another aspect)"""
    sc = _scene(hf, oracle, 1, False)
    rng = np.random.default_rng(21)
    data = rng.uniform(0.2, 1.0, (res[1], res[0])).astype(np.float32)
    for name in sorted(P.PROJECTORS):
        pr = P.PROJECTORS[name](res=res)
        tr, unsure = P.traced(pr, sc.np["p"], sc.np["sh_n"], sc.np["d"], sc.np["t"])
        assert unsure.mean() <= UNSURE_CAP
        for wrap in WRAPS:
            td = _cu(data).requires_grad_(True)
            img, val, vis = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, pr, td, wrap), albedo=P.ALBEDO, spp=SPP,
                                                  return_value=True, return_visibility=True)
            v = _np(vis).astype(bool)
            assert not v[~tr & ~unsure].any() and v.sum() > 100
            _, rv, _ = P.forward(pr, sc.np["p"], sc.np["sh_n"], None, data, WRAPS[wrap], P.ALBEDO, v, SPP)
            assert P.err_abs(np.where(unsure, 0, _np(val)), np.where(unsure, 0, rv)) <= TOL["value"]
            val.sum().backward()
            g = P.adjoint(pr, sc.np["p"], sc.np["sh_n"], None, data, WRAPS[wrap], P.ALBEDO, v & ~unsure, SPP, grad_value=np.ones(sc.n))
            if res == (1, 1):
                # the one texel: value = I * (the untextured value), and its gradient the sum of the untextured values
                _, plain = hf.projector_lighting(sc.shape, sc.si, sc.ray, _projector(hf, pr, None), albedo=P.ALBEDO, spp=SPP, return_value=True)
                assert P.err_abs(_np(val), _np(plain).astype(np.float64) * float(data[0, 0])) <= TOL["value"]
            assert _rel(_np(td.grad), g.gtex) <= TOL["grad_tex"] + unsure.mean()


@pytest.mark.parametrize("pose", [False, True])
def test_inverse_projector_example_descends(hf, pose):
    import inverse_projector
    hist, err = inverse_projector.run(size=48, steps=31, pose=pose, verbose=False)
    assert np.isfinite(hist[-1]) and hist[30] < hist[0], (hist[0], hist[30])

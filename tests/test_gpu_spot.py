"""Spot lighting on the GPU (hf_spot_rays, hf_spot_lighting, _adjoint, _tangent) on row_helpers.base_scene: sine_heights(96),
max_height 0.5, the 64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0), both face_normals
modes, under the rig of 8 lights of tests/spot_ref.py (RIG: `above`, `side`, `wide`, `hard`, `point`, `graze`, `near`, `back`),
K = 1 (each light alone), K = 3 and K = 8.
  (1) bit k of vis against the two-call sequence hf_spot_rays(light k) + hf_ray_test bit for bit, the masks and the rays
      against the restatement, the shares of the rig;
  (2) the K = 8 launch against eight K = 1 launches (and a K = 3 launch) bit for bit: image rows, value rows, vis bits;
  (3) image, value, every gradient (the K x 15 reduced numbers among them) and the tangents against the restatement fed
      with the GPU's visibility; `point` alone against the parent's hf_amd.point_lighting given the same visibility; the
      transposition gap on the device through backward and jvp, the gradients reaching each SpotLight's own tensors;
  (4) the K x 15 reduced numbers over 301 rows; the chain spot_lighting -> loss -> backward -> dL/dheight;
  (5) n = 0, an all-miss wavefront, n = 1, 63, 65, 257 with guard bands, every optional pointer NULL in turn, spp 1, 3 and
      4, HF_FORCE_GRID, bitwise repeatability, a captured graph;
  (6) a light that faces away, a flat field, cutoff == beam at 30 and at 180;
  (7) examples/inverse_spot.py descends in both modes.

Tolerances (scripts/spot_f32_error.py computes them on the CPU, profiles/spot/f32_error.json).  The restatement
evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records and visibility,
for the whole rig, weighted and not, by at most the figures of F32 below (spot_ref.errors: per-lane quantities as the
largest difference over max(1, the largest value), the K x 15 reduced numbers as the L2 norm of the difference over the L2
norm of the float64 result).  The GPU is allowed four times that: another operation order.  Samples on which rounding may
decide a mask (a deciding quantity within MARGIN) are left out of the comparisons, at most UNSURE_CAP of the samples over
the union of the 8 lights (the restatement alone leaves out at most 2.5e-4); lanes within KINK of theta = beam have their
bit for that light cleared in the visibility the derivative kernels and the restatement are given (at most 3.1e-4)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import spot_ref as P
from row_helpers import GUARD, _cu, _np, base_scene, guarded, intact, rows, sub, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SPP = P.SPP
K8 = len(P.NAMES)
F32 = {"image": 1.54e-7, "value": 3.66e-7, "dimage": 1.81e-7, "dvalue": 3.17e-7, "grad_sh_n": 3.43e-7, "grad_p": 3.62e-7,
       "grad_weight": 1.68e-7, "grad15": 4.19e-7}
# the maxima of profiles/spot/f32_error.json, cut off after three digits
TOL = {k: 4 * v for k, v in F32.items()}
COMBOS = [(oi, fn) for oi in range(2) for fn in (True, False)]
TRIO = (1, 4, 6)        # side, point, near: the K = 3 rig


def _spot(hf, L, **kw):
    a = dict(to_world=L.to_world, intensity=L.intensity, cutoff_angle=L.cutoff, beam_width=L.beam)
    a.update(kw)
    return hf.SpotLight(a["to_world"], a["intensity"], a["cutoff_angle"], a["beam_width"])


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """a scene with the rig on it, once: the GPU's K = 8 launch, the restatement's masks and the asserted shares"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), P.ORIGINS[oi], face_normals)
        sc.eligible, _ = P.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
        sc.ref = P.rig()
        sc.lights = [_spot(hf, L) for L in sc.ref]
        sc.w = P.inputs(sc.n, SPP, K8).w
        img, val, vis = hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights, albedo=P.ALBEDO, spp=SPP, weight=_cu(sc.w),
                                         return_value=True, return_visibility=True)
        sc.img, sc.val, sc.byte = _np(img).copy(), _np(val).copy(), _np(vis).copy()
        sc.vis = P.unpack(sc.byte, K8)
        tu = [P.traced(L, sc.np["p"], sc.np["sh_n"], sc.np["d"], sc.np["t"]) for L in sc.ref]
        sc.traced, sc.unsure = np.stack([a for a, _ in tu]), np.stack([b for _, b in tu])
        sc.sure = ~sc.unsure.any(0)
        sc.pix = sc.sure.reshape(-1, SPP).all(1)
        shares = {}
        for k, (name, L) in enumerate(zip(P.NAMES, sc.ref)):
            m = P.mapping(L, sc.np["p"])
            tr = sc.traced[k]
            shares[name] = {"in_cone_of_eligible": float(m.cone[sc.eligible].mean()), "zone_of_traced": float(m.zone[tr].mean()),
                            "occluded_of_traced": float(1.0 - sc.vis[k][tr].mean())}
        print("unsure union", sc.unsure.any(0).mean(), {k: {a: round(b, 3) for a, b in v.items()} for k, v in shares.items()})
        P.assert_shares(shares, float(sc.unsure.any(0).mean()))               # (asserted on the restatement before comparing)
        sc.steady = np.stack([P.steady(L, sc.np["p"], sc.vis[k]) for k, L in enumerate(sc.ref)]) & sc.sure[None]
        _SCENES[key] = sc
    return _SCENES[key]


def _structs(hf, lights):
    S = (hf._capi.hf_spot_light_t * len(lights))()
    for k, L in enumerate(lights):
        S[k] = hf._capi.hf_spot_light_t((C.c_double * 12)(*L.to_world.reshape(-1).tolist()), L.intensity, L.cutoff, L.beam)
    return S


class _Wave:
    """the device rows of the samples [lo, hi) of a scene and the C calls on them"""

    def __init__(self, hf, sc, lo=0, hi=None):
        hi = sc.n if hi is None else hi
        cut = lambda v: v.detach()[..., lo:hi].contiguous()
        self.hf, self.shape, self.n = hf, sc.shape, hi - lo
        self.p, self.nr, self.sn, self.d, self.t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
        self.np = {k: _np(v) for k, v in (("p", self.p), ("n", self.nr), ("sh_n", self.sn), ("d", self.d), ("t", self.t))}
        self.lib, self.check = hf._capi.lib(), hf._capi.check
        self.ws = torch.empty(self.lib.hf_spot_workspace_floats(K8), device="cuda")

    def mid(self, lights, w):
        return (None if w is None else w.data_ptr(), len(lights), _structs(self.hf, lights), P.ALBEDO)

    def head(self, spp):
        return (self.n, spp, rows(self.p), rows(self.sn), rows(self.d), self.t.data_ptr())

    def forward(self, spp, mid, image=None, value=None, vis=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_spot_lighting(self.shape._h, self.n, spp, rows(self.p), rows(self.nr), rows(self.sn), rows(self.d),
                                             self.t.data_ptr(), *mid, image, value, vis, s))

    def adjoint(self, spp, mid, vis, gi, gv, gn=None, gp=None, gw=None, gl=None, ws=True):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_spot_lighting_adjoint(*self.head(spp), *mid, vis, gi, gv, gn, gp, gw, gl,
                                                     self.ws.data_ptr() if ws else None, s))

    def tangent(self, spp, mid, vis, dn=None, dp=None, dw=None, dl=None, dimage=None, dvalue=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_spot_lighting_tangent(*self.head(spp), *mid, vis, dn, dp, dw, dl, dimage, dvalue, s))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _sel(x, ks, K=K8):
    """the inputs x of the whole rig cut down to the lights ks"""
    y = P.types.SimpleNamespace(**vars(x))
    y.gi, y.gv, y.dl = x.gi[list(ks)], x.gv[list(ks)], x.dl[list(ks)]
    return y


def _derivatives(wv, lights, x, vis, spp, weighted=True):
    """the adjoint and the tangent through the C ABI under the inputs x and the given [K, n] visibility: a namespace with
    dimage, dvalue, gn, gp, gw, g15 as numpy"""
    n, K = wv.n, len(lights)
    w = _cu(x.w) if weighted else None
    mid = wv.mid(lights, w)
    v8 = _cu(P.pack(vis))
    z = lambda *s: torch.zeros(s, device="cuda")
    gn, gp, gw, gl = z(3, n), z(3, n), z(n), z(K, P.PARAMS)
    gi, gv = _cu(x.gi), _cu(x.gv)
    wv.adjoint(spp, mid, v8.data_ptr(), gi.data_ptr(), gv.data_ptr(), rows(gn), rows(gp), gw.data_ptr() if weighted else None, gl.data_ptr())
    dimage, dvalue = z(K, n // spp), z(K, n)
    t = [_cu(np.asarray(a, np.float32)) for a in (x.dn, x.dp, x.dw, x.dl)]
    wv.tangent(spp, mid, v8.data_ptr(), rows(t[0]), rows(t[1]), t[2].data_ptr() if weighted else None, t[3].data_ptr(),
               dimage.data_ptr(), dvalue.data_ptr())
    torch.cuda.synchronize()
    g = P.types.SimpleNamespace(dimage=_np(dimage), dvalue=_np(dvalue), gn=_np(gn), gp=_np(gp), g15=_np(gl))
    g.gw = _np(gw) if weighted else None
    return g


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_visibility_bits_equal_the_two_call_sequence_bit_for_bit_and_the_masks_the_restatement(hf, oracle, oi, face_normals):
    sc = _scene(hf, oracle, oi, face_normals)
    assert not sc.byte[~sc.eligible & sc.sure].any()                              # a sample that is not eligible: a zero byte
    for k, (name, L) in enumerate(zip(P.NAMES, sc.ref)):
        ray = hf.spot_rays(sc.si, sc.ray, sc.lights[k])
        tr = _np(ray.maxt >= 0)
        two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
        assert np.array_equal(sc.vis[k], two), (name, int((sc.vis[k] != two).sum()))
        sure = ~sc.unsure[k]
        assert np.array_equal(tr[sure], sc.traced[k][sure]), name
        o, w, maxt, _ = P.rays(L, sc.np["p"], sc.np["n"], sc.np["sh_n"], sc.np["d"], sc.np["t"])
        both = tr & sc.traced[k]
        assert np.abs(_np(ray.o) - o)[:, both].max() <= 1e-6 and np.abs(_np(ray.d) - w)[:, both].max() <= 2e-6, name
        assert np.abs(_np(ray.maxt) - maxt)[both].max() <= 1e-5 * maxt[both].max()
        assert not _np(ray.o)[:, ~tr].any() and not _np(ray.d)[:, ~tr].any() and (_np(ray.maxt)[~tr] == -1).all()
        assert not sc.val[k][~sc.vis[k]].any()                                   # exactly 0 where the bit is clear


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_one_launch_of_eight_equals_eight_launches_of_one_and_a_launch_of_three_bit_for_bit(hf, oracle, oi, face_normals):
    """a light's arithmetic does not depend on its neighbours"""
    sc = _scene(hf, oracle, oi, face_normals)
    w = _cu(sc.w)
    for k in range(K8):
        img, val, vis = hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights[k], albedo=P.ALBEDO, spp=SPP, weight=w, return_value=True,
                                         return_visibility=True)
        assert img.shape == (1, sc.n // SPP) and val.shape == (1, sc.n)
        assert np.array_equal(_np(img)[0], sc.img[k]) and np.array_equal(_np(val)[0], sc.val[k]), P.NAMES[k]
        assert np.array_equal(_np(vis), (sc.byte >> k) & 1), P.NAMES[k]
    img, val, vis = hf.spot_lighting(sc.shape, sc.si, sc.ray, [sc.lights[k] for k in TRIO], albedo=P.ALBEDO, spp=SPP, weight=w,
                                     return_value=True, return_visibility=True)
    assert np.array_equal(_np(img), sc.img[list(TRIO)]) and np.array_equal(_np(val), sc.val[list(TRIO)])
    assert np.array_equal(P.unpack(_np(vis), 3), sc.vis[list(TRIO)]) and not (_np(vis) >> 3).any()


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, oi, face_normals):
    sc = _scene(hf, oracle, oi, face_normals)
    wv = _Wave(hf, sc)
    x = P.inputs(sc.n, SPP, K8)
    assert np.array_equal(x.w, sc.w)
    worst = {k: 0.0 for k in TOL}
    for ks, weighted in ((tuple(range(K8)), True), (TRIO, False)) + tuple(((k,), True) for k in range(K8)):
        lights, xs, steady = [sc.ref[k] for k in ks], _sel(x, ks), sc.steady[list(ks)]
        ref = P.evaluate(lights, wv.np, xs, steady, SPP, weighted=weighted)
        ref.image, ref.value = P.forward(lights, wv.np["p"], wv.np["sh_n"], x.w if weighted else None, P.ALBEDO, sc.vis[list(ks)], SPP)
        got = _derivatives(wv, lights, xs, steady, SPP, weighted)
        if weighted:
            got.image, got.value = sc.img[list(ks)].copy(), sc.val[list(ks)].copy()
        else:
            img, val = wv.hf.spot_lighting(sc.shape, sc.si, sc.ray, [sc.lights[k] for k in ks], albedo=P.ALBEDO, spp=SPP, return_value=True)
            got.image, got.value = _np(img).copy(), _np(val).copy()
        for ns in (got, ref):                                                       # (samples that rounding may decide)
            ns.value = np.where(sc.sure[None], ns.value, 0.0)
            ns.image = np.where(sc.pix[None], ns.image, 0.0)
        dark = ~steady.any(0)
        for k in ("gn", "gp", "gw"):
            assert getattr(got, k) is None or not getattr(got, k)[..., dark].any()  # exact zeros where vis = 0
        assert not got.dvalue[~steady].any()
        assert ref.value.max() > 0.1 and np.abs(ref.g15[:, [3, 7, 11, 12]]).min() > 0
        for j, k in enumerate(ks):                                                  # a hard edge: exact zeros for both angles
            if P.NAMES[k] in ("hard", "point"):
                assert not got.g15[j, 13:].any() and not ref.g15[j, 13:].any()
            elif P.NAMES[k] != "wide":                                              # (`wide`'s zone misses the terrain from one origin)
                assert np.abs(ref.g15[j]).min() > 0
        err = P.errors(got, ref)
        print([P.NAMES[k] for k in ks], weighted, {k: "%.3g" % v for k, v in err.items()})
        for k, v in err.items():
            worst[k] = max(worst[k], v)
    # `point` alone against the parent's point_lighting given the same visibility, within the image tolerance
    k = P.NAMES.index("point")
    L = sc.ref[k]
    pl = hf.point_lighting(sc.si, sc.ray, torch.tensor([[*L.to_world[:, 3], L.intensity]]), albedo=P.ALBEDO, spp=SPP,
                           vis=_cu(sc.vis[k:k + 1].astype(np.uint8)))
    one = _np(hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights[k], albedo=P.ALBEDO, spp=SPP))
    cross = P.err_abs(np.where(sc.pix, _np(pl)[0], 0.0), np.where(sc.pix, one[0], 0.0).astype(np.float64))
    print("point against point_lighting", cross)
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    assert cross <= TOL["image"], cross
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


def _leaf(hf, sc, sh_n=None, p=None):
    si = hf.SurfaceInteraction3f()
    si.n, si.t = sc.si.n.detach(), sc.si.t.detach()
    si.p = sc.si.p.detach().clone().requires_grad_(True) if p is None else p
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True) if sh_n is None else sh_n)
    return si


def test_transposition_on_the_device_through_backward_and_jvp_repeatability_and_each_lights_own_gradients(hf, oracle):
    """<J u, v> = <u, J^T v> through the public function: forward_ad against backward, both sides float32 results added up in
    float64, each side within its tolerance of the exact bilinear form; two runs give the same bits; every SpotLight's own
    tensors get their own gradients"""
    sc = _scene(hf, oracle, 0, False)
    x = P.inputs(sc.n, SPP, K8)
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    runs = []
    for _ in range(2):
        si, wt = _leaf(hf, sc), _cu(x.w).requires_grad_(True)
        par = [[f64(v).requires_grad_(True) for v in (L.to_world, L.intensity, L.cutoff, L.beam)] for L in sc.ref]
        lights = [hf.SpotLight(*q) for q in par]
        img, val, vis = hf.spot_lighting(sc.shape, si, sc.ray, lights, albedo=P.ALBEDO, spp=SPP, weight=wt, return_value=True,
                                         return_visibility=True)
        ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
        with fwAD.dual_level():
            sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
            dual = [hf.SpotLight(fwAD.make_dual(f64(L.to_world), f64(x.dl[k, :12]).reshape(3, 4)),
                                 *(fwAD.make_dual(f64(v), f64(x.dl[k, 12 + j])) for j, v in enumerate((L.intensity, L.cutoff, L.beam))))
                    for k, L in enumerate(sc.ref)]
            ti, tv = hf.spot_lighting(sc.shape, sid, sc.ray, dual, albedo=P.ALBEDO, spp=SPP, weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)),
                                      return_value=True)
            ti, tv = fwAD.unpack_dual(ti).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        assert all(q[0].grad.shape == (3, 4) and q[1].grad.shape == () for q in par)
        g15 = torch.stack([torch.cat([q[0].grad.reshape(-1), torch.stack([q[1].grad, q[2].grad, q[3].grad])]) for q in par])
        runs.append((vis.clone(), img.detach().clone(), val.detach().clone(), si.sh_frame.n.grad.clone(), si.p.grad.clone(), wt.grad.clone(),
                     g15, ti, tv))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                                    # everything: bitwise
    byte, _, _, gn, gp, gw, g15, ti, tv = (_np(a) for a in runs[0])
    assert np.array_equal(byte, sc.byte)
    for k, name in enumerate(P.NAMES):                                              # each light's own numbers, not its neighbour's
        assert np.abs(g15[k, [3, 7, 11, 12]]).min() > 0, name
        assert not g15[k, 13:].any() if name in ("hard", "point") else (name == "wide" or np.abs(g15[k, 13:]).min() > 0), name
    gap = transposition_gap(((ti, x.gi), (tv, x.gv)), ((gn, x.dn), (gp, x.dp), (gw, x.dw), (g15, x.dl)))
    size = np.linalg.norm(tv) * np.linalg.norm(x.gv) + np.linalg.norm(ti) * np.linalg.norm(x.gi)
    print("transposition gap", gap, "size", size)
    assert size > 0 and gap <= (TOL["dvalue"] + TOL["grad_p"]) * size, (gap, size)


def _busiest(vis, n):
    """the start (a multiple of 64) of the window of n samples that holds the most visible ones"""
    c = np.concatenate([[0], np.cumsum(vis)])
    starts = np.arange(0, len(vis) - n + 1, 64)
    return int(starts[np.argmax(c[starts + n] - c[starts])])


def test_the_reduced_numbers_over_301_rows(hf, oracle):
    """n = 301 (more than one block, odd), spp 1: the K x 15 numbers against the float64 reverse sweep"""
    sc = _scene(hf, oracle, 1, True)
    lo = _busiest(sc.steady.sum(0), 301)
    wv = _Wave(hf, sc, lo, lo + 301)
    x = P.inputs(301, 1, K8, seed=8)
    vis = sc.steady[:, lo:lo + 301]
    assert (vis.sum(1) >= 20).all(), vis.sum(1)
    got = _derivatives(wv, sc.ref, x, vis, 1)
    ref = P.adjoint(sc.ref, wv.np["p"], wv.np["sh_n"], x.w, P.ALBEDO, vis, 1, x.gi, x.gv)
    err = P.err_l2(got.g15, ref.g15)
    print("grad15 over 301 rows", err, [P.err_l2(got.g15[k], ref.g15[k]) for k in range(K8)])
    assert err <= TOL["grad15"], err
    for k in range(K8):                                                             # (each row against its own norm)
        assert P.err_l2(got.g15[k], ref.g15[k]) <= TOL["grad15"], (P.NAMES[k], got.g15[k], ref.g15[k])


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """spot_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n and grad_p (fed with
    the GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: four times the float32 error of grad_p
    (the larger of the two gradients' errors) + the 1e-5 of the sky row's chain."""
    sc = _scene(hf, oracle, 0, face_normals)
    x = P.inputs(sc.n, SPP, K8)
    keep = ((sc.steady | ~sc.vis).all(0)) & sc.sure
    gi = np.where(keep.reshape(-1, SPP).all(1)[None], x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.spot_lighting(shape, si, sc.ray, sc.lights, albedo=P.ALBEDO, spp=SPP, return_visibility=True)
    assert np.array_equal(_np(vis), sc.byte)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = P.adjoint(sc.ref, _np(si.p), _np(si.sh_frame.n), None, P.ALBEDO, sc.vis, SPP, gi)
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
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, val0, vis0 = hf.spot_lighting(sc.shape, si0, ray0, sc.lights, spp=SPP, return_value=True, return_visibility=True)
    assert img0.shape == (K8, 0) and val0.shape == (K8, 0) and vis0.shape == (0,)
    img0.sum().backward()
    assert len(hf.spot_rays(si0, ray0, sc.lights[0])) == 0
    # a wavefront with no eligible sample: rays that leave the terrain behind, and hits seen from behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    for s, ry in ((sim, up), (sc.si, up)):
        imgm, vism = hf.spot_lighting(sc.shape, s, ry, sc.lights, spp=SPP, return_visibility=True)
        assert not bool(imgm.any()) and not bool(vism.any())
    with pytest.raises(hf.HfError):
        hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights, spp=3)
    with pytest.raises(ValueError):
        hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights + sc.lights[:1], spp=SPP)
    bad = hf.SpotLight(sc.ref[0].to_world, 1.0, 30.0, 20.0)
    bad.cutoff_angle = 190.0
    with pytest.raises(hf.HfError):
        hf.spot_lighting(sc.shape, sc.si, sc.ray, bad, spp=SPP)


@pytest.mark.parametrize("n,spp", [(1, 1), (63, 1), (65, 1), (257, 1), (3 * 151, 3), (4 * 65, 4)])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, n, spp):
    """n = 1, 63, 65, 257 (a part of a batch of 64, one more than a batch, more than a block), spp 3 (no power of two: the
    film's other paths, whose atomics add a pixel's samples in an order that may differ from launch to launch: its image is
    compared to rounding, everything else bit for bit) and 4, guard values around every output row of every light, and every
    optional pointer NULL in turn"""
    sc = _scene(hf, oracle, 1, True)
    G = 96
    lo = _busiest(sc.vis.sum(0), max(n, 64))
    wv = _Wave(hf, sc, lo, lo + n)
    x = P.inputs(n, spp, K8, seed=9)
    w = _cu(x.w)
    mid = wv.mid(sc.ref, w)
    sure = sc.sure[lo:lo + n]
    npix = n // spp
    tree = spp & (spp - 1) == 0         # the film's shuffle tree: one store per pixel; any other spp: float atomics

    def planes(count, m):
        """a [K8, G + m + G] guarded buffer whose K rows stand m apart: the pointer to row 0's element G only if the rows are
        contiguous -- so one buffer of K * m elements with one guard band on either side"""
        buf = torch.full((K8 * m + 2 * G,), GUARD, device="cuda")
        return buf, buf.data_ptr() + 4 * G

    def forward(skip=None, m=mid):
        image, ip = planes(K8, npix); value, vp = planes(K8, n)
        vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        wv.forward(spp, m, None if skip == "image" else ip, None if skip == "value" else vp, None if skip == "vis" else vis.data_ptr() + G)
        return {"image": image, "value": value, "vis": vis}

    def whole(buf, m):
        return bool((buf[:G] == GUARD).all()) and bool((buf[G + K8 * m:] == GUARD).all()) and bool((buf[G:G + K8 * m] != GUARD).all())
    full = forward()
    assert whole(full["image"], npix) and whole(full["value"], n)
    assert bool((full["vis"][:G] == 0x5A).all()) and bool((full["vis"][G + n:] == 0x5A).all())
    vis8 = full["vis"][G:G + n].contiguous()
    vis = P.unpack(_np(vis8), K8)
    assert np.array_equal(vis, sc.vis[:, lo:lo + n]) and (n < 64 or vis.sum() >= 20)  # the slice of the whole
    ri, rv = P.forward(sc.ref, wv.np["p"], wv.np["sh_n"], x.w, P.ALBEDO, vis, spp)
    pix = sure.reshape(-1, spp).all(1)
    assert P.err_abs(np.where(pix, _np(full["image"][G:G + K8 * npix]).reshape(K8, npix), 0), np.where(pix, ri, 0)) <= TOL["image"]
    assert P.err_abs(np.where(sure, _np(full["value"][G:G + K8 * n]).reshape(K8, n), 0), np.where(sure, rv, 0)) <= TOL["value"]
    for skip in ("image", "value", "vis"):
        part = forward(skip)
        for k in full:
            if k == skip:
                assert bool((part[k] == (0x5A if k == "vis" else GUARD)).all())     # untouched
            elif k == "image" and not tree:
                assert torch.allclose(part[k], full[k], rtol=1e-6, atol=1e-7)       # (float atomics: the order differs)
            else:
                assert torch.equal(part[k], full[k]), (skip, k)
    # without a weight: the same film as with a weight of 1
    one_w = torch.ones(n, device="cuda")
    a, b = forward(m=wv.mid(sc.ref, None)), forward(m=wv.mid(sc.ref, one_w))
    assert all(torch.equal(a[k], b[k]) or (k == "image" and not tree and torch.allclose(a[k], b[k], rtol=1e-6, atol=1e-7)) for k in a)
    # the adjoint: all outputs, then each one NULL in turn -- the others are bitwise what they were
    gi, gv = _cu(x.gi), _cu(x.gv)

    def adjoint(skip=None, gi_=gi, gv_=gv, ws=True):
        gn, gnp = guarded(n, G, 3); gp, gpp = guarded(n, G, 3); gw, gwp = guarded(n, G)
        o = {"gn": gn, "gp": gp, "gw": gw, "gl": torch.zeros((K8, P.PARAMS), device="cuda")}
        ptr = lambda k, v: None if skip == k else v
        wv.adjoint(spp, mid, vis8.data_ptr(), _ptr(gi_), _ptr(gv_), ptr("gn", gnp), ptr("gp", gpp), ptr("gw", gwp[0]),
                   ptr("gl", o["gl"].data_ptr()), ws=ws)
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("gn", "gp", "gw"))
    for skip in ("gn", "gp", "gw", "gl"):
        part = adjoint(skip, ws=skip != "gl")                                      # (no grad_lights: no workspace needed)
        for k in part:
            if k == skip:
                assert bool((part[k] == GUARD).all()) if k != "gl" else not bool(part[k].any())   # untouched
            else:
                assert torch.equal(part[k], fulla[k]), (skip, k)
    assert torch.equal(adjoint()["gl"], fulla["gl"])                                # bitwise repeatable
    if vis.any():
        only_i, only_v = adjoint(gv_=None), adjoint(gi_=None)
        for k in ("gn", "gl"):
            cut = (lambda a: a[:, G:G + n]) if k == "gn" else (lambda a: a)
            s = cut(_np(only_i[k])).astype(np.float64) + cut(_np(only_v[k]))
            assert np.abs(s - cut(_np(fulla[k]))).max() <= 1e-5 * np.abs(cut(_np(fulla[k]))).max()
    # the tangent: every tangent NULL in turn, and their sum is the whole (the map is linear)
    t = {k: _cu(np.asarray(v, np.float32)) for k, v in (("dn", x.dn), ("dp", x.dp), ("dw", x.dw), ("dl", x.dl))}

    def tangent(use, image=True, value=True):
        di, dip = planes(K8, npix); dv, dvp = planes(K8, n)
        q = lambda k: (rows(t[k]) if k in ("dn", "dp") else t[k].data_ptr()) if k in use else None
        wv.tangent(spp, mid, vis8.data_ptr(), q("dn"), q("dp"), q("dw"), q("dl"), dip if image else None, dvp if value else None)
        assert (whole(di, npix) if image else bool((di == GUARD).all())) and (whole(dv, n) if value else bool((dv == GUARD).all()))
        return di, dv
    di, dv = tangent(tuple(t))
    assert torch.equal(tangent(tuple(t), value=False)[0], di) and torch.equal(tangent(tuple(t), image=False)[1], dv)
    cutv = lambda a: _np(a[G:G + K8 * n]).reshape(K8, n).astype(np.float64)
    parts = sum(cutv(tangent((k,))[1]) for k in t)
    assert not bool(tangent(())[1][G:G + K8 * n].any())
    wholev = cutv(dv)
    assert np.abs(wholev - parts).max() <= 4 * TOL["dvalue"] * max(1.0, np.abs(wholev).max())   # (four results, each within its tolerance)
    assert np.abs(_np(di[G:G + K8 * npix]).reshape(K8, npix) - wholev.reshape(K8, -1, spp).mean(2)).max() <= 1e-6 * max(1.0, np.abs(wholev).max())
    # the rays
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    wv.check(wv.lib.hf_spot_rays(n, rows(wv.p), rows(wv.nr), rows(wv.sn), rows(wv.d), wv.t.data_ptr(), _structs(hf, sc.ref[1:2]), rop, rdp,
                                 rmp[0], torch.cuda.current_stream().cuda_stream))
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
    """HF_FORCE_GRID = 3: both grid-stride loops of the adjoint run 22 times per lane on 16384 samples and every light's slab
    has 3 rows; the per-lane outputs are bitwise the same, the reduced numbers the same sums in another order.  The forward,
    the tangent and the rays kernels take one lane per sample: the hook does not reach them"""
    sc = _scene(hf, oracle, 0, True)
    wv = _Wave(hf, sc)
    x = P.inputs(sc.n, SPP, K8)
    free = _derivatives(wv, sc.ref, x, sc.steady, SPP)
    ray = hf.spot_rays(sc.si, sc.ray, sc.lights[1])
    with _env(3):
        assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 3
        forced = _derivatives(wv, sc.ref, x, sc.steady, SPP)
        _, v2 = hf.spot_lighting(sc.shape, sc.si, sc.ray, sc.lights, albedo=P.ALBEDO, spp=SPP, return_visibility=True)
        ray2 = hf.spot_rays(sc.si, sc.ray, sc.lights[1])
    for k in ("gn", "gp", "gw", "dimage", "dvalue"):
        assert np.array_equal(getattr(free, k), getattr(forced, k)), k
    assert P.err_l2(forced.g15, free.g15.astype(np.float64)) <= 1e-6
    assert np.array_equal(_np(v2), sc.byte) and torch.equal(ray.maxt, ray2.maxt) and torch.equal(ray.o, ray2.o)


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    """one captured graph of a single-stream forward + adjoint (+ tangent), replayed"""
    sc = _scene(hf, oracle, 1, True)
    wv = _Wave(hf, sc)
    mid = wv.mid(sc.ref, None)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, device="cuda", dtype=dtype)
    img, val, vis = z(K8, sc.n // SPP), z(K8, sc.n), z(sc.n, dtype=torch.uint8)
    gn, gp, gl, dimg, dval = z(3, sc.n), z(3, sc.n), z(K8, P.PARAMS), z(K8, sc.n // SPP), z(K8, sc.n)
    gi, ones, dl = torch.ones((K8, sc.n // SPP), device="cuda"), torch.ones((3, sc.n), device="cuda"), torch.ones((K8, P.PARAMS), device="cuda")

    def launch():
        gl.zero_()                                                       # (accumulated into)
        wv.forward(SPP, mid, img.data_ptr(), val.data_ptr(), vis.data_ptr())
        wv.adjoint(SPP, mid, vis.data_ptr(), gi.data_ptr(), None, rows(gn), rows(gp), None, gl.data_ptr())
        wv.tangent(SPP, mid, vis.data_ptr(), rows(ones), rows(ones), None, dl.data_ptr(), dimg.data_ptr(), dval.data_ptr())
    outs = (img, val, vis, gn, gp, gl, dimg, dval)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert np.array_equal(_np(vis), sc.byte) and float(img.abs().sum()) > 0 and float(gl[:, 12].abs().min()) > 0
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


def test_a_light_that_faces_away_a_flat_field_and_hard_edges_at_30_and_180(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    away = hf.SpotLight.look_at((0.3, -0.2, 2.0), (0.3, -0.2, 4.0), (0, 1, 0), intensity=3.0, cutoff_angle=20.0, beam_width=15.0)   # `above`, looking up
    img, val, vis = hf.spot_lighting(sc.shape, sc.si, sc.ray, [away, sc.lights[0]], spp=SPP, return_value=True, return_visibility=True)
    assert not bool((vis & 1).any()) and not bool(img[0].any()) and not bool(val[0].any())      # exactly 0
    assert np.array_equal(_np(vis) >> 1, (sc.byte >> 0) & 1)                         # ... and its neighbour is untouched by it
    assert bool((hf.spot_rays(sc.si, sc.ray, away).maxt == -1).all())
    shape, si, ray = _flat(hf)
    rig = [_spot(hf, L) for L in sc.ref]
    _, vis = hf.spot_lighting(shape, si, ray, rig, spp=1, return_visibility=True)
    for k, name in enumerate(P.NAMES):
        tr = hf.spot_rays(si, ray, rig[k]).maxt >= 0
        assert torch.equal(((vis >> k) & 1).bool(), tr), name                         # nothing occludes
    assert float(((vis >> P.NAMES.index("point")) & 1).float().mean()) == 1.0
    # cutoff == beam at 30 and at 180: values of the full beam, exact zeros for both angle gradients, no NaN
    for cut in (30.0, 180.0):
        par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (2.0, cut, cut)]
        L = hf.SpotLight(torch.tensor(sc.ref[3].to_world), *par)
        s = _leaf(hf, sc)
        img, val, vis = hf.spot_lighting(sc.shape, s, sc.ray, L, albedo=P.ALBEDO, spp=SPP, return_value=True, return_visibility=True)
        assert bool(vis.any()) and bool(torch.isfinite(val).all())
        val.sum().backward()
        assert float(par[1].grad) == 0.0 and float(par[2].grad) == 0.0 and float(par[0].grad) > 0
        assert bool(torch.isfinite(s.p.grad).all()) and bool(torch.isfinite(s.sh_frame.n.grad).all())
        ref = P.forward([P.light(sc.ref[3].to_world, 2.0, cut, cut)], sc.np["p"], sc.np["sh_n"], None, P.ALBEDO, _np(vis)[None].astype(bool), SPP)[1]
        assert P.err_abs(_np(val), ref) <= TOL["value"]
        if cut == 180.0:                                                             # every sample that faces the light is traced
            u = sc.ref[3].to_world[:, 3:4] - sc.np["p"].astype(np.float64)
            facing = sc.eligible & ((sc.np["sh_n"] * u).sum(0) > P.MARGIN)
            assert (_np(hf.spot_rays(sc.si, sc.ray, L).maxt) >= 0)[facing].all()


@pytest.mark.parametrize("pose", [False, True])
def test_inverse_spot_example_descends(hf, pose):
    import inverse_spot
    hist, err = inverse_spot.run(size=48, steps=31, pose=pose, verbose=False)
    assert np.isfinite(hist[-1]) and hist[30] < hist[0], (hist[0], hist[30])

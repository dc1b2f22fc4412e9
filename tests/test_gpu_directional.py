"""Directional lighting on the GPU (hf_directional_rays, hf_directional_lighting, _adjoint, _tangent) on
row_helpers.base_scene: sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and
from (0.6, 0.35, 2.0), both face_normals modes, under the rig of 8 lights of tests/directional_ref.py (RIG: `zenith`, `high`,
`low_x`, `low_y`, `graze`, `diag`, `below`, `unnorm`; to_light deliberately not unit), K = 1 (each light alone), K = 3 and
K = 8.
  (1) bit k of vis against the two-call sequence hf_directional_rays(light k) + hf_ray_test bit for bit in both coherence
      modes and against the oracle's ray_test on those rays, the ray direction bitwise float32(l), the origin and the masks
      against the restatement, the shares of the rig on the GPU's visibility;
  (2) the K = 8 launch against eight K = 1 launches (and a K = 3 launch) bit for bit: image rows, value rows, vis bits;
  (3) image, value, every gradient (the K x 4 reduced numbers among them) and the tangents against the restatement fed
      with the GPU's visibility, weighted and not; the images against the existing hf_amd.direct_lighting handed the same
      visibility; the transposition gap on the device through backward and jvp, the gradients reaching each
      DirectionalLight's own tensors;
  (4) the K x 4 reduced numbers over 301 rows and over many block rows (HF_FORCE_GRID); the chain directional_lighting ->
      loss -> backward -> dL/dheight;
  (5) n = 0, an all-miss wavefront, n = 1, 63, 65, 257 with guard bands, every optional pointer NULL in turn, spp 1, 3 and
      4, bitwise repeatability, a captured graph;
  (6) `below` alone on a flat field, a flat field under `zenith`, irradiance = 0;
  (7) examples/inverse_sun.py descends in both modes.

Tolerances (scripts/directional_f32_error.py computes them on the CPU, profiles/directional/f32_error.json).
The restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records
and visibility, for the whole rig, weighted and not, by at most the figures of F32 below (directional_ref.errors: per-lane
quantities as the largest difference over max(1, the largest value), the K x 4 reduced numbers as the L2 norm of the
difference over the L2 norm of the float64 result).  The GPU is allowed four times that: another operation order.  Samples
on which rounding may decide a mask (a deciding quantity within MARGIN) are left out of the mask and value comparisons, at
most UNSURE_CAP of the samples over the union of the 8 lights (the restatement alone leaves out at most 4.3e-4)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import directional_ref as D
from row_helpers import GUARD, _cu, _np, base_scene, guarded, intact, leaf_si, rows, sub, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SPP = D.SPP
K8 = len(D.NAMES)
# the maxima of profiles/directional/f32_error.json, cut off after three digits
F32 = {"image": 1.75e-7, "value": 1.86e-7, "dimage": 1.65e-7, "dvalue": 1.59e-7, "grad_sh_n": 1.13e-7, "grad_weight": 1.36e-7,
       "grad4": 2.37e-7}
TOL = {k: 4 * v for k, v in F32.items()}
DIRECT = 2e-5           # hf_direct_lighting's documented bound, of the largest pixel
CHAIN = 4 * 3.62e-7 + 1e-5   # the relative L2 tests/test_gpu_spot.py allows its chain to the heights
COMBOS = [(oi, fn) for oi in range(2) for fn in (True, False)]
TRIO = tuple(D.NAMES.index(k) for k in ("low_x", "diag", "unnorm"))        # the K = 3 rig


def _light(hf, L):
    return hf.DirectionalLight(L.to_light, L.irradiance)


_SCENES = {}


def _shares(sc, vis):
    return {name: D.shares(sc.eligible, sc.traced[k], vis[k]) for k, name in enumerate(D.NAMES)}


def _scene(hf, oracle, oi, face_normals):
    """a scene with the rig on it, once: the GPU's K = 8 launch, the restatement's masks and the asserted shares"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), D.ORIGINS[oi], face_normals)
        sc.eligible, _ = D.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
        sc.ref = D.rig()
        sc.lights = [_light(hf, L) for L in sc.ref]
        sc.w = D.inputs(sc.n, SPP, K8).w
        img, val, vis = hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights, albedo=D.ALBEDO, spp=SPP, weight=_cu(sc.w),
                                                return_value=True, return_visibility=True)
        sc.img, sc.val, sc.byte = _np(img).copy(), _np(val).copy(), _np(vis).copy()
        sc.vis = D.unpack(sc.byte, K8)
        tu = [D.traced(L, sc.np["sh_n"], sc.np["d"], sc.np["t"]) for L in sc.ref]
        sc.traced, sc.unsure = np.stack([a for a, _ in tu]), np.stack([b for _, b in tu])
        sc.sure = ~sc.unsure.any(0)
        sc.pix = sc.sure.reshape(-1, SPP).all(1)
        sh = _shares(sc, sc.vis & sc.traced)
        print("unsure union", sc.unsure.any(0).mean(), {k: {a: round(b, 3) for a, b in v.items()} for k, v in sh.items()})
        D.assert_shares(sh, float(sc.unsure.any(0).mean()))               # (asserted before anything is compared)
        sc.held = sc.vis & sc.sure[None]          # the visibility the derivative kernels and the restatement are given
        _SCENES[key] = sc
    return _SCENES[key]


def _structs(hf, lights):
    S = (hf._capi.hf_directional_light_t * len(lights))()
    for k, L in enumerate(lights):
        S[k] = hf._capi.hf_directional_light_t((C.c_double * 3)(*L.to_light.tolist()), L.irradiance)
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
        self.ws = torch.empty(self.lib.hf_directional_workspace_floats(K8), device="cuda")

    def mid(self, lights, w):
        return (None if w is None else w.data_ptr(), len(lights), _structs(self.hf, lights), D.ALBEDO)

    def head(self, spp):
        return (self.n, spp, rows(self.sn), rows(self.d), self.t.data_ptr())

    def forward(self, spp, mid, image=None, value=None, vis=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_directional_lighting(self.shape._h, self.n, spp, rows(self.p), rows(self.nr), rows(self.sn),
                                                    rows(self.d), self.t.data_ptr(), *mid, image, value, vis, s))

    def adjoint(self, spp, mid, vis, gi, gv, gn=None, gw=None, gl=None, ws=True):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_directional_lighting_adjoint(*self.head(spp), *mid, vis, gi, gv, gn, gw, gl,
                                                            self.ws.data_ptr() if ws else None, s))

    def tangent(self, spp, mid, vis, dn=None, dw=None, dl=None, dimage=None, dvalue=None):
        s = torch.cuda.current_stream().cuda_stream
        self.check(self.lib.hf_directional_lighting_tangent(*self.head(spp), *mid, vis, dn, dw, dl, dimage, dvalue, s))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _sel(x, ks):
    """the inputs x of the whole rig cut down to the lights ks"""
    y = D.types.SimpleNamespace(**vars(x))
    y.gi, y.gv, y.dl = x.gi[list(ks)], x.gv[list(ks)], x.dl[list(ks)]
    return y


def _derivatives(wv, lights, x, vis, spp, weighted=True):
    """the adjoint and the tangent through the C ABI under the inputs x and the given [K, n] visibility: a namespace with
    dimage, dvalue, gn, gw, g4 as numpy"""
    n, K = wv.n, len(lights)
    w = _cu(x.w) if weighted else None
    mid = wv.mid(lights, w)
    v8 = _cu(D.pack(vis))
    z = lambda *s: torch.zeros(s, device="cuda")
    gn, gw, gl = z(3, n), z(n), z(K, D.PARAMS)
    gi, gv = _cu(x.gi), _cu(x.gv)
    wv.adjoint(spp, mid, v8.data_ptr(), gi.data_ptr(), gv.data_ptr(), rows(gn), gw.data_ptr() if weighted else None, gl.data_ptr())
    dimage, dvalue = z(K, n // spp), z(K, n)
    t = [_cu(np.asarray(a, np.float32)) for a in (x.dn, x.dw, x.dl)]
    wv.tangent(spp, mid, v8.data_ptr(), rows(t[0]), t[1].data_ptr() if weighted else None, t[2].data_ptr(), dimage.data_ptr(),
               dvalue.data_ptr())
    torch.cuda.synchronize()
    g = D.types.SimpleNamespace(dimage=_np(dimage), dvalue=_np(dvalue), gn=_np(gn), g4=_np(gl))
    g.gw = _np(gw) if weighted else None
    return g


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_visibility_bits_equal_the_two_call_sequence_bit_for_bit_and_the_masks_the_restatement(hf, oracle, oi, face_normals):
    sc = _scene(hf, oracle, oi, face_normals)
    assert not sc.byte[~sc.eligible & sc.sure].any()                              # a sample that is not eligible: a zero byte
    for k, (name, L) in enumerate(zip(D.NAMES, sc.ref)):
        ray = hf.directional_rays(sc.si, sc.ray, sc.lights[k])
        tr = _np(ray.maxt >= 0)
        for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
            old = sc.shape.ray_coherence()
            sc.shape.set_ray_coherence(mode)
            try:
                two = _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))
                # (the fused launch under this mode: the same byte, and the mode is left as it was)
                _, byte = hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights[k], spp=SPP, return_visibility=True)
                assert sc.shape.ray_coherence() == mode and np.array_equal(_np(byte), (sc.byte >> k) & 1), (name, mode)
            finally:
                sc.shape.set_ray_coherence(old)
            assert np.array_equal(sc.vis[k], two), (name, mode, int((sc.vis[k] != two).sum()))
        # ... and the oracle's ray_test on those rays
        r7 = np.concatenate([_np(ray.o), _np(ray.d), _np(ray.maxt)[None]]).astype(np.float32)
        occ = np.zeros(sc.n, bool)
        occ[tr] = sc.field.ray_test(r7[:, tr]).astype(bool)
        assert np.array_equal(sc.vis[k], tr & ~occ), (name, int((sc.vis[k] != (tr & ~occ)).sum()))
        sure = ~sc.unsure[k]
        assert np.array_equal(tr[sure], sc.traced[k][sure]), name
        o, w, maxt, _ = D.rays(L, sc.np["p"], sc.np["n"], sc.np["sh_n"], sc.np["d"], sc.np["t"])
        both = tr & sc.traced[k]
        lf = D.unit(L)[0].astype(np.float32)
        assert np.array_equal(_np(ray.d)[:, tr], np.repeat(lf[:, None], int(tr.sum()), 1)), name   # bitwise float32(l)
        assert np.abs(_np(ray.o) - o)[:, both].max() <= 1e-6, name                 # the sky row's bound
        assert np.isinf(_np(ray.maxt)[tr]).all()
        assert not _np(ray.o)[:, ~tr].any() and not _np(ray.d)[:, ~tr].any() and (_np(ray.maxt)[~tr] == -1).all()
        assert not sc.val[k][~sc.vis[k]].any()                                   # exactly 0 where the bit is clear


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_one_launch_of_eight_equals_eight_launches_of_one_and_a_launch_of_three_bit_for_bit(hf, oracle, oi, face_normals):
    """a light's arithmetic does not depend on its neighbours"""
    sc = _scene(hf, oracle, oi, face_normals)
    w = _cu(sc.w)
    kw = dict(albedo=D.ALBEDO, spp=SPP, weight=w, return_value=True, return_visibility=True)
    for k in range(K8):
        img, val, vis = hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights[k], **kw)
        assert img.shape == (1, sc.n // SPP) and val.shape == (1, sc.n)
        assert np.array_equal(_np(img)[0], sc.img[k]) and np.array_equal(_np(val)[0], sc.val[k]), D.NAMES[k]
        assert np.array_equal(_np(vis), (sc.byte >> k) & 1), D.NAMES[k]
    img, val, vis = hf.directional_lighting(sc.shape, sc.si, sc.ray, [sc.lights[k] for k in TRIO], **kw)
    assert np.array_equal(_np(img), sc.img[list(TRIO)]) and np.array_equal(_np(val), sc.val[list(TRIO)])
    assert np.array_equal(D.unpack(_np(vis), 3), sc.vis[list(TRIO)]) and not (_np(vis) >> 3).any()
    # the [K, 4] tensor that direct_lighting takes is the same rig
    tab = torch.tensor(np.stack([D.row4(L) for L in sc.ref]), dtype=torch.float64)
    img, val, vis = hf.directional_lighting(sc.shape, sc.si, sc.ray, tab, **kw)
    assert np.array_equal(_np(img), sc.img) and np.array_equal(_np(val), sc.val) and np.array_equal(_np(vis), sc.byte)


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, oi, face_normals):
    sc = _scene(hf, oracle, oi, face_normals)
    wv = _Wave(hf, sc)
    x = D.inputs(sc.n, SPP, K8)
    assert np.array_equal(x.w, sc.w)
    worst = {k: 0.0 for k in TOL}
    for ks, weighted in ((tuple(range(K8)), True), (tuple(range(K8)), False), (TRIO, False)) + tuple(((k,), True) for k in range(K8)):
        lights, xs, held = [sc.ref[k] for k in ks], _sel(x, ks), sc.held[list(ks)]
        ref = D.evaluate(lights, wv.np, xs, held, SPP, weighted=weighted)
        ref.image, ref.value = D.forward(lights, wv.np["sh_n"], x.w if weighted else None, D.ALBEDO, sc.vis[list(ks)], SPP)
        got = _derivatives(wv, lights, xs, held, SPP, weighted)
        if weighted:
            got.image, got.value = sc.img[list(ks)].copy(), sc.val[list(ks)].copy()
        else:
            img, val = hf.directional_lighting(sc.shape, sc.si, sc.ray, [sc.lights[k] for k in ks], albedo=D.ALBEDO, spp=SPP,
                                               return_value=True)
            got.image, got.value = _np(img).copy(), _np(val).copy()
        for ns in (got, ref):                                                       # (samples that rounding may decide)
            ns.value = np.where(sc.sure[None], ns.value, 0.0)
            ns.image = np.where(sc.pix[None], ns.image, 0.0)
        dark = ~held.any(0)
        for k in ("gn", "gw"):
            assert getattr(got, k) is None or not getattr(got, k)[..., dark].any()  # exact zeros where vis = 0
        assert not got.dvalue[~held].any()
        # (`below` alone lights only the few steep slopes that face it: its irradiance is the smallest of the rig)
        assert ref.value.max() > (0.01 if ks == (D.NAMES.index("below"),) else 0.1)
        assert np.abs(ref.g4[:, 3]).min() > 0 and (np.abs(ref.g4[:, :3]).max(1) > 0).all()
        err = D.errors(got, ref)
        print([D.NAMES[k] for k in ks], weighted, {k: "%.3g" % v for k, v in err.items()})
        for k, v in err.items():
            worst[k] = max(worst[k], v)
    # every light's image against the existing direct_lighting handed the same visibility (unit directions, as it asks)
    tab = torch.tensor(np.stack([np.append(D.unit(L)[0], L.irradiance) for L in sc.ref]), dtype=torch.float32)
    old = _np(hf.direct_lighting(sc.si, sc.ray, tab, albedo=D.ALBEDO, spp=SPP, vis=_cu(sc.vis.astype(np.uint8)), weight=_cu(sc.w)))
    for k, name in enumerate(D.NAMES):
        cross = np.abs(np.where(sc.pix, old[k].astype(np.float64) - sc.img[k], 0.0)).max()
        print(name, "against direct_lighting", cross, "largest pixel", sc.img[k].max())
        assert cross <= DIRECT * max(sc.img[k].max(), old[k].max()), (name, cross)
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


def test_transposition_on_the_device_through_backward_and_jvp_repeatability_and_each_lights_own_gradients(hf, oracle):
    """<J u, v> = <u, J^T v> through the public function: forward_ad against backward, both sides float32 results added up in
    float64, each side within its tolerance of the exact bilinear form; two runs give the same bits; every
    DirectionalLight's own tensors get their own gradients"""
    sc = _scene(hf, oracle, 0, False)
    x = D.inputs(sc.n, SPP, K8)
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    runs = []
    for _ in range(2):
        si, wt = leaf_si(hf, sc), _cu(x.w).requires_grad_(True)
        par = [[f64(v).requires_grad_(True) for v in (L.to_light, L.irradiance)] for L in sc.ref]
        lights = [hf.DirectionalLight(*q) for q in par]
        img, val, vis = hf.directional_lighting(sc.shape, si, sc.ray, lights, albedo=D.ALBEDO, spp=SPP, weight=wt, return_value=True,
                                                return_visibility=True)
        ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
        with fwAD.dual_level():
            sid = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)))
            dual = [hf.DirectionalLight(fwAD.make_dual(f64(L.to_light), f64(x.dl[k, :3])),
                                        fwAD.make_dual(f64(L.irradiance), f64(x.dl[k, 3]))) for k, L in enumerate(sc.ref)]
            ti, tv = hf.directional_lighting(sc.shape, sid, sc.ray, dual, albedo=D.ALBEDO, spp=SPP,
                                             weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), return_value=True)
            ti, tv = fwAD.unpack_dual(ti).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        assert all(q[0].grad.shape == (3,) and q[1].grad.shape == () for q in par)
        g4 = torch.stack([torch.cat([q[0].grad, q[1].grad.reshape(1)]) for q in par])
        runs.append((vis.clone(), img.detach().clone(), val.detach().clone(), si.sh_frame.n.grad.clone(), wt.grad.clone(), g4, ti, tv))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                                    # everything: bitwise
    byte, _, _, gn, gw, g4, ti, tv = (_np(a) for a in runs[0])
    assert np.array_equal(byte, sc.byte)
    for k, (name, L) in enumerate(zip(D.NAMES, sc.ref)):                            # each light's own numbers, not its neighbour's
        assert g4[k, 3] != 0 and np.abs(g4[k, :3]).max() > 0, name
        l = D.unit(L)[0]
        assert abs(g4[k, :3] @ l) <= 4 * TOL["grad4"] * np.linalg.norm(g4[k, :3]), name   # orthogonal to l
    assert len({float(v) for v in g4[:, 3]}) == K8
    gap = transposition_gap(((ti, x.gi), (tv, x.gv)), ((gn, x.dn), (gw, x.dw), (g4, x.dl)))
    size = np.linalg.norm(tv) * np.linalg.norm(x.gv) + np.linalg.norm(ti) * np.linalg.norm(x.gi)
    print("transposition gap", gap, "size", size)
    assert size > 0 and gap <= (TOL["dvalue"] + TOL["grad_sh_n"]) * size, (gap, size)


def _busiest(vis, n):
    """the start (a multiple of 64) of the window of n samples that holds the most visible ones"""
    c = np.concatenate([[0], np.cumsum(vis)])
    starts = np.arange(0, len(vis) - n + 1, 64)
    return int(starts[np.argmax(c[starts + n] - c[starts])])


def test_the_reduced_numbers_over_301_rows(hf, oracle):
    """n = 301 (more than one block, odd), spp 1: the K x 4 numbers against the float64 reverse sweep"""
    sc = _scene(hf, oracle, 1, True)
    lo = _busiest(sc.held.sum(0), 301)
    wv = _Wave(hf, sc, lo, lo + 301)
    x = D.inputs(301, 1, K8, seed=8)
    vis = sc.held[:, lo:lo + 301]
    print("visible of 301 per light", vis.sum(1))
    assert ((vis.sum(1) >= 20).sum() >= 5) and vis[D.NAMES.index("graze")].any(), vis.sum(1)
    got = _derivatives(wv, sc.ref, x, vis, 1)
    ref = D.adjoint(sc.ref, wv.np["sh_n"], x.w, D.ALBEDO, vis, 1, x.gi, x.gv)
    err = D.err_l2(got.g4, ref.g4)
    print("grad4 over 301 rows", err, [D.err_l2(got.g4[k], ref.g4[k]) for k in range(K8) if vis[k].any()])
    assert err <= TOL["grad4"], err
    for k in range(K8):                                                             # (each row against its own norm)
        if vis[k].any():
            assert D.err_l2(got.g4[k], ref.g4[k]) <= TOL["grad4"], (D.NAMES[k], got.g4[k], ref.g4[k])
        else:
            assert not got.g4[k].any() and not ref.g4[k].any()


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """directional_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n (fed with
    the GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: the spot row's for its chain."""
    sc = _scene(hf, oracle, 0, face_normals)
    x = D.inputs(sc.n, SPP, K8)
    gi = np.where(sc.pix[None], x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.directional_lighting(shape, si, sc.ray, sc.lights, albedo=D.ALBEDO, spp=SPP, return_visibility=True)
    assert np.array_equal(_np(vis), sc.byte)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = D.adjoint(sc.ref, _np(si.sh_frame.n), None, D.ALBEDO, sc.vis, SPP, gi)
    rr = _np(sc.rays)
    if face_normals:
        t, u, v, prim = sc.field.ray_intersect_preliminary(rr)
        gh = sc.field.adjoint(rr, t, u, v, prim, {"sh_n": g.gn.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[9:12] = _cu(g.gn.astype(np.float32))
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= CHAIN, err


def test_empty_and_all_miss_wavefronts_and_refusals(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, val0, vis0 = hf.directional_lighting(sc.shape, si0, ray0, sc.lights, spp=SPP, return_value=True, return_visibility=True)
    assert img0.shape == (K8, 0) and val0.shape == (K8, 0) and vis0.shape == (0,)
    img0.sum().backward()
    assert len(hf.directional_rays(si0, ray0, sc.lights[0])) == 0
    # a wavefront with no eligible sample: rays that leave the terrain behind, and hits seen from behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    for s, ry in ((sim, up), (sc.si, up)):
        imgm, vism = hf.directional_lighting(sc.shape, s, ry, sc.lights, spp=SPP, return_visibility=True)
        assert not bool(imgm.any()) and not bool(vism.any())
        assert bool((hf.directional_rays(s, ry, sc.lights[0]).maxt == -1).all())
    with pytest.raises(hf.HfError):
        hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights, spp=3)
    with pytest.raises(ValueError):
        hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights + sc.lights[:1], spp=SPP)
    bad = hf.DirectionalLight((0.0, 0.0, 1.0), 1.0)
    bad.irradiance = float("nan")
    with pytest.raises(hf.HfError):
        hf.directional_lighting(sc.shape, sc.si, sc.ray, bad, spp=SPP)


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
    x = D.inputs(n, spp, K8, seed=9)
    w = _cu(x.w)
    mid = wv.mid(sc.ref, w)
    sure = sc.sure[lo:lo + n]
    npix = n // spp
    tree = spp & (spp - 1) == 0         # the film's shuffle tree: one store per pixel; any other spp: float atomics

    def planes(m):
        """one buffer of K8 * m elements, the K rows m apart, with one guard band on either side"""
        buf = torch.full((K8 * m + 2 * G,), GUARD, device="cuda")
        return buf, buf.data_ptr() + 4 * G

    def forward(skip=None, m=mid):
        image, ip = planes(npix); value, vp = planes(n)
        vis = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        wv.forward(spp, m, None if skip == "image" else ip, None if skip == "value" else vp, None if skip == "vis" else vis.data_ptr() + G)
        return {"image": image, "value": value, "vis": vis}

    def whole(buf, m):
        return bool((buf[:G] == GUARD).all()) and bool((buf[G + K8 * m:] == GUARD).all()) and bool((buf[G:G + K8 * m] != GUARD).all())
    full = forward()
    assert whole(full["image"], npix) and whole(full["value"], n)
    assert bool((full["vis"][:G] == 0x5A).all()) and bool((full["vis"][G + n:] == 0x5A).all())
    vis8 = full["vis"][G:G + n].contiguous()
    vis = D.unpack(_np(vis8), K8)
    assert np.array_equal(vis, sc.vis[:, lo:lo + n]) and (n < 64 or vis.sum() >= 20)  # the slice of the whole
    ri, rv = D.forward(sc.ref, wv.np["sh_n"], x.w, D.ALBEDO, vis, spp)
    pix = sure.reshape(-1, spp).all(1)
    assert D.err_abs(np.where(pix, _np(full["image"][G:G + K8 * npix]).reshape(K8, npix), 0), np.where(pix, ri, 0)) <= TOL["image"]
    assert D.err_abs(np.where(sure, _np(full["value"][G:G + K8 * n]).reshape(K8, n), 0), np.where(sure, rv, 0)) <= TOL["value"]
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
        gn, gnp = guarded(n, G, 3); gw, gwp = guarded(n, G)
        o = {"gn": gn, "gw": gw, "gl": torch.zeros((K8, D.PARAMS), device="cuda")}
        ptr = lambda k, v: None if skip == k else v
        wv.adjoint(spp, mid, vis8.data_ptr(), _ptr(gi_), _ptr(gv_), ptr("gn", gnp), ptr("gw", gwp[0]), ptr("gl", o["gl"].data_ptr()), ws=ws)
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("gn", "gw"))
    for skip in ("gn", "gw", "gl"):
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
    t = {k: _cu(np.asarray(v, np.float32)) for k, v in (("dn", x.dn), ("dw", x.dw), ("dl", x.dl))}

    def tangent(use, image=True, value=True):
        di, dip = planes(npix); dv, dvp = planes(n)
        q = lambda k: (rows(t[k]) if k == "dn" else t[k].data_ptr()) if k in use else None
        wv.tangent(spp, mid, vis8.data_ptr(), q("dn"), q("dw"), q("dl"), dip if image else None, dvp if value else None)
        assert (whole(di, npix) if image else bool((di == GUARD).all())) and (whole(dv, n) if value else bool((dv == GUARD).all()))
        return di, dv
    di, dv = tangent(tuple(t))
    assert torch.equal(tangent(tuple(t), value=False)[0], di) and torch.equal(tangent(tuple(t), image=False)[1], dv)
    assert torch.equal(tangent(tuple(t))[0], di) and torch.equal(tangent(tuple(t))[1], dv)     # bitwise repeatable, any spp
    cutv = lambda a: _np(a[G:G + K8 * n]).reshape(K8, n).astype(np.float64)
    parts = sum(cutv(tangent((k,))[1]) for k in t)
    assert not bool(tangent(())[1][G:G + K8 * n].any())
    wholev = cutv(dv)
    assert np.abs(wholev - parts).max() <= 3 * TOL["dvalue"] * max(1.0, np.abs(wholev).max())   # (three results, each within its tolerance)
    assert np.abs(_np(di[G:G + K8 * npix]).reshape(K8, npix) - wholev.reshape(K8, -1, spp).mean(2)).max() <= 1e-6 * max(1.0, np.abs(wholev).max())
    # the rays
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    wv.check(wv.lib.hf_directional_rays(n, rows(wv.p), rows(wv.nr), rows(wv.sn), rows(wv.d), wv.t.data_ptr(), _structs(hf, sc.ref[2:3]),
                                        rop, rdp, rmp[0], torch.cuda.current_stream().cuda_stream))
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
    has 3 rows; unforced, the same launch has 64 block rows per light.  The per-lane outputs are bitwise the same, the
    reduced numbers the same sums in another order and both within the tolerance of the float64 reverse sweep.  The
    forward, the tangent and the rays kernels take one lane per sample: the hook does not reach them"""
    sc = _scene(hf, oracle, 0, True)
    wv = _Wave(hf, sc)
    x = D.inputs(sc.n, SPP, K8)
    assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 64
    free = _derivatives(wv, sc.ref, x, sc.held, SPP)
    ray = hf.directional_rays(sc.si, sc.ray, sc.lights[2])
    with _env(3):
        assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 3
        forced = _derivatives(wv, sc.ref, x, sc.held, SPP)
        _, v2 = hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights, albedo=D.ALBEDO, spp=SPP, return_visibility=True)
        ray2 = hf.directional_rays(sc.si, sc.ray, sc.lights[2])
    for k in ("gn", "gw", "dimage", "dvalue"):
        assert np.array_equal(getattr(free, k), getattr(forced, k)), k
    ref = D.adjoint(sc.ref, wv.np["sh_n"], x.w, D.ALBEDO, sc.held, SPP, x.gi, x.gv)
    for got in (free, forced):
        for k in range(K8):
            assert D.err_l2(got.g4[k], ref.g4[k]) <= TOL["grad4"], (D.NAMES[k], got.g4[k], ref.g4[k])
    assert np.array_equal(_np(v2), sc.byte) and torch.equal(ray.maxt, ray2.maxt) and torch.equal(ray.o, ray2.o)


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    """one captured graph of a single-stream forward + adjoint + tangent, replayed: the capture succeeds only if no call
    allocates or synchronises the host"""
    sc = _scene(hf, oracle, 1, True)
    wv = _Wave(hf, sc)
    mid = wv.mid(sc.ref, None)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, device="cuda", dtype=dtype)
    img, val, vis = z(K8, sc.n // SPP), z(K8, sc.n), z(sc.n, dtype=torch.uint8)
    gn, gl, dimg, dval = z(3, sc.n), z(K8, D.PARAMS), z(K8, sc.n // SPP), z(K8, sc.n)
    gi, ones, dl = torch.ones((K8, sc.n // SPP), device="cuda"), torch.ones((3, sc.n), device="cuda"), torch.ones((K8, D.PARAMS), device="cuda")

    def launch():
        gl.zero_()                                                       # (accumulated into)
        wv.forward(SPP, mid, img.data_ptr(), val.data_ptr(), vis.data_ptr())
        wv.adjoint(SPP, mid, vis.data_ptr(), gi.data_ptr(), None, rows(gn), None, gl.data_ptr())
        wv.tangent(SPP, mid, vis.data_ptr(), rows(ones), None, dl.data_ptr(), dimg.data_ptr(), dval.data_ptr())
    outs = (img, val, vis, gn, gl, dimg, dval)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert np.array_equal(_np(vis), sc.byte) and float(img.abs().sum()) > 0 and float(gl[:, 3].abs().min()) > 0
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


def test_below_alone_a_flat_field_under_the_zenith_and_a_dark_light(hf, oracle):
    shape, si, ray = _flat(hf)
    n = len(ray)
    ref = D.rig()
    # `below` alone on a flat field: no sample faces it, no bit is set, every gradient is an exact zero
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (ref[6].to_light, ref[6].irradiance)]
    s = hf.SurfaceInteraction3f()
    s.p, s.n, s.t = si.p.detach(), si.n.detach(), si.t.detach()
    s.sh_frame = hf.Frame3f(None, None, si.sh_frame.n.detach().clone().requires_grad_(True))
    wt = torch.ones(n, device="cuda", requires_grad=True)
    img, val, vis = hf.directional_lighting(shape, s, ray, hf.DirectionalLight(*par), albedo=D.ALBEDO, weight=wt, return_value=True,
                                            return_visibility=True)
    assert not bool(vis.any()) and not bool(img.any()) and not bool(val.any())
    (img.sum() + val.sum()).backward()
    assert not bool(s.sh_frame.n.grad.any()) and not bool(wt.grad.any()) and not bool(par[0].grad.any()) and float(par[1].grad) == 0.0
    assert bool((hf.directional_rays(s, ray, hf.DirectionalLight(ref[6].to_light)).maxt == -1).all())
    # a flat field under `zenith`: every sample is lit, value = albedo / pi E
    img, val, vis = hf.directional_lighting(shape, si, ray, _light(hf, ref[0]), albedo=D.ALBEDO, return_value=True, return_visibility=True)
    assert bool((vis == 1).all())
    known = D.ALBEDO / np.pi * ref[0].irradiance
    assert np.abs(_np(val).astype(np.float64) - known).max() <= TOL["value"] * max(1.0, known)
    assert np.abs(_np(img).astype(np.float64) - known).max() <= TOL["image"] * max(1.0, known)
    # the whole rig on the flat field: nothing occludes, bit k is set exactly where the sample is traced
    rig = [_light(hf, L) for L in ref]
    _, vis = hf.directional_lighting(shape, si, ray, rig, return_visibility=True)
    for k, name in enumerate(D.NAMES):
        tr = hf.directional_rays(si, ray, rig[k]).maxt >= 0
        assert torch.equal(((vis >> k) & 1).bool(), tr) and bool(tr.all()) == (name != "below"), name
    # irradiance = 0: a zero image, finite gradients (the irradiance's own is the image per unit irradiance)
    sc = _scene(hf, oracle, 1, True)
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (ref[2].to_light, 0.0)]
    s = leaf_si(hf, sc)
    img, val, vis = hf.directional_lighting(sc.shape, s, sc.ray, hf.DirectionalLight(*par), albedo=D.ALBEDO, spp=SPP, return_value=True,
                                            return_visibility=True)
    assert np.array_equal(_np(vis), (sc.byte >> 2) & 1) and not bool(img.any()) and not bool(val.any())
    val.sum().backward()
    assert not bool(s.sh_frame.n.grad.any()) and not bool(par[0].grad.any()) and bool(torch.isfinite(par[1].grad))
    want = (D.ALBEDO / np.pi * (np.asarray(sc.np["sh_n"], np.float64) * D.unit(ref[2])[0][:, None]).sum(0))[sc.vis[2]].sum()
    assert abs(float(par[1].grad) - want) <= TOL["grad4"] * abs(want) and want > 0


@pytest.mark.parametrize("heights", [False, True])
def test_inverse_sun_example_descends(hf, heights):
    import inverse_sun
    hist, err0, err = inverse_sun.run(size=48, steps=31, heights=heights, verbose=False)
    print("heights" if heights else "rig", "loss", hist[0], "->", hist[30], "parameter error", err0, "->", err)
    assert np.isfinite(hist[-1]) and hist[30] < hist[0], (hist[0], hist[30])
    assert err < err0, (err0, err)

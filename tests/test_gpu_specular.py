"""Specular highlights on the GPU (hf_specular_lighting, _adjoint, _tangent); under to_world, flip_normals and odd grids: tests/test_gpu_row_scenes.py.  Here row_helpers.base_scene: sine_heights(96),
max_height 0.5, the 64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0), both face_normals
modes, under the rig of 8 lights of tests/directional_ref.py.  The visibility byte is the GPU's own
hf_directional_lighting's; the roughness is a per-sample row spread over [0.05, 0.6] ("row") and, in one case per scene,
a constant 0.02 ("sharp"); eta = 1.5.
  (1) the shares of the rig on the GPU's byte, asserted before anything is compared;
  (2) image, value, grad_sh_n, grad_weight, grad_alpha, the K x 4 reduced numbers, dimage and dvalue against the
      restatement (tests/specular_ref.py) fed the same byte, weighted and not, for K = 8, a K = 3 subset and each light
      alone; the K = 8 launch against eight K = 1 launches bit for bit;
  (3) the transposition gap on the device through backward and jvp with each light's parameters and a scalar alpha as
      the user's own tensors, bitwise repeatability, a captured graph;
  (4) the K x 4 numbers over 301 rows and under HF_FORCE_GRID (64 and 3 block rows per light);
  (5) n = 0, a byte of zeros, n = 1, 63, 65, 257, spp 3 and 4 with guard bands and every optional pointer NULL in turn;
  (6) the flat-field known answers; dL/dheight through ray_intersect -> directional_lighting (vis) -> specular_lighting;
  (7) examples/inverse_highlight.py descends in both modes.

Tolerances (scripts/specular_f32_error.py computes them on the CPU, profiles/specular/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records and
visibility, by at most the figures of F32 below (specular_ref.errors: per-lane quantities as the largest difference over
max(1, the largest value), the K x 4 reduced numbers as relative L2).  The GPU is allowed four times that.  The kernels
form D and the products in double, which the float32 restatement does not (float32 cancels in s^2 / a^2 + c_h^2): the
device's measured worst case over the four scenes (this file's print; MI355X) is far inside -- image 2.4e-7, value
2.1e-7, dimage 2.8e-7, dvalue 2.5e-7, grad_sh_n 2.4e-7, grad_alpha 2.2e-7, grad_weight 2.1e-7, the K x 4 numbers 5.4e-7
on "row"; at most 1.7e-7 on "sharp".  Every mask comes from the byte and from cosines both sides form in double from
the same float32 rows: NO sample is left out of any comparison."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import directional_ref as D
import specular_ref as R
from row_helpers import GUARD, _cu, _np, base_scene, guarded, intact, leaf_si, rows, sub, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SPP = D.SPP
K8 = len(D.NAMES)
ETA = R.ETA
# the maxima of profiles/specular/f32_error.json per roughness row, cut off after three digits
F32 = {"row": {"image": 4.92e-5, "value": 5.13e-5, "dimage": 5.14e-5, "dvalue": 5.36e-5, "grad_sh_n": 7.53e-5,
               "grad_alpha": 1.04e-4, "grad_weight": 5.02e-5, "grad4": 6.93e-5},
       "sharp": {"image": 4.40e-4, "value": 5.18e-4, "dimage": 7.28e-4, "dvalue": 7.29e-4, "grad_sh_n": 6.61e-4,
                 "grad_alpha": 8.83e-4, "grad_weight": 4.40e-4, "grad4": 1.01e-3}}
TOL = {kind: {k: 4 * v for k, v in f.items()} for kind, f in F32.items()}
CHAIN = 4 * 3.62e-7 + 1e-5   # the relative L2 tests/test_gpu_directional.py allows its chain to the heights
COMBOS = [(oi, fn) for oi in range(2) for fn in (True, False)]
TRIO = tuple(D.NAMES.index(k) for k in ("low_x", "diag", "unnorm"))        # the K = 3 rig


def _light(hf, L):
    return hf.DirectionalLight(L.to_light, L.irradiance)


def _structs(hf, lights):
    S = (hf._capi.hf_directional_light_t * len(lights))()
    for k, L in enumerate(lights):
        S[k] = hf._capi.hf_directional_light_t((C.c_double * 3)(*L.to_light.tolist()), L.irradiance)
    return S


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """a scene with the rig on it, once: the GPU's directional byte, the asserted shares, and the K = 8 specular launch
    with the "row" roughness and a weight"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), D.ORIGINS[oi], face_normals)
        sc.ref = D.rig()
        sc.lights = [_light(hf, L) for L in sc.ref]
        _, vis = hf.directional_lighting(sc.shape, sc.si, sc.ray, sc.lights, spp=SPP, return_visibility=True)
        sc.vis8 = vis
        sc.byte = _np(vis).copy()
        sc.vis = D.unpack(sc.byte, K8)
        # the shares of the rig on this byte, asserted before anything is compared: a comparison of zeros cannot pass
        el, _ = D.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
        tu = [D.traced(L, sc.np["sh_n"], sc.np["d"], sc.np["t"]) for L in sc.ref]
        tr, unsure = np.stack([a for a, _ in tu]), np.stack([b for _, b in tu])
        sh = {name: D.shares(el, tr[k], sc.vis[k] & tr[k]) for k, name in enumerate(D.NAMES)}
        print("unsure union", unsure.any(0).mean(), {k: {a: round(b, 3) for a, b in v.items()} for k, v in sh.items()})
        D.assert_shares(sh, float(unsure.any(0).mean()))
        x = R.inputs(sc.n, SPP, K8)
        sc.w = x.w
        sc.alpha = {kind: R.alpha_row(kind, sc.n) for kind in ("row", "sharp")}
        img, val = hf.specular_lighting(sc.si, sc.ray, sc.lights, vis, _cu(sc.alpha["row"]), eta=ETA, spp=SPP, weight=_cu(sc.w),
                                        return_value=True)
        sc.img, sc.val = _np(img).copy(), _np(val).copy()
        lit = (sc.val > 0).mean(1)
        print("share of samples with a highlight per light", lit.round(3))
        assert (lit[[D.NAMES.index(k) for k in ("zenith", "high", "unnorm")]] > 0.3).all() and (lit > 0).all(), lit
        _SCENES[key] = sc
    return _SCENES[key]


class _Wave:
    """the device rows of the samples [lo, hi) of a scene and the C calls on them"""

    def __init__(self, hf, sc, lo=0, hi=None, kind="row"):
        hi = sc.n if hi is None else hi
        cut = lambda v: v.detach()[..., lo:hi].contiguous()
        self.hf, self.n = hf, hi - lo
        self.sn, self.d = cut(sc.si.sh_frame.n), cut(sc.ray.d)
        self.al = _cu(sc.alpha[kind][lo:hi])
        self.np = {"sh_n": _np(self.sn), "d": _np(self.d), "alpha": _np(self.al)}
        self.lib, self.check = hf._capi.lib(), hf._capi.check
        self.ws = torch.empty(self.lib.hf_specular_workspace_floats(K8), device="cuda")

    def head(self, spp, lights, w, vis, eta=ETA):
        return (self.n, spp, rows(self.sn), rows(self.d), None if w is None else w.data_ptr(), self.al.data_ptr(), eta,
                len(lights), _structs(self.hf, lights), vis)

    def forward(self, head, image=None, value=None):
        self.check(self.lib.hf_specular_lighting(*head, image, value, torch.cuda.current_stream().cuda_stream))

    def adjoint(self, head, gi, gv, gn=None, gw=None, ga=None, gl=None, ws=True):
        self.check(self.lib.hf_specular_lighting_adjoint(*head, gi, gv, gn, gw, ga, gl, self.ws.data_ptr() if ws else None,
                                                         torch.cuda.current_stream().cuda_stream))

    def tangent(self, head, dn=None, dw=None, da=None, dl=None, dimage=None, dvalue=None):
        self.check(self.lib.hf_specular_lighting_tangent(*head, dn, dw, da, dl, dimage, dvalue,
                                                         torch.cuda.current_stream().cuda_stream))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _sel(x, ks):
    """the inputs x of the whole rig cut down to the lights ks"""
    y = types.SimpleNamespace(**vars(x))
    y.gi, y.gv, y.dl = x.gi[list(ks)], x.gv[list(ks)], x.dl[list(ks)]
    return y


def _all(wv, lights, x, vis, spp, weighted=True):
    """forward, adjoint and tangent through the C ABI under the inputs x and the given [K, n] visibility: the namespace
    specular_ref.errors takes, as numpy"""
    n, K = wv.n, len(lights)
    w = _cu(x.w) if weighted else None
    v8 = _cu(D.pack(vis))
    head = wv.head(spp, lights, w, v8.data_ptr())
    z = lambda *s: torch.zeros(s, device="cuda")
    image, value = z(K, n // spp), z(K, n)
    wv.forward(head, image.data_ptr(), value.data_ptr())
    gn, gw, ga, gl = z(3, n), z(n), z(n), z(K, D.PARAMS)
    gi, gv = _cu(x.gi), _cu(x.gv)
    wv.adjoint(head, gi.data_ptr(), gv.data_ptr(), rows(gn), gw.data_ptr() if weighted else None, ga.data_ptr(), gl.data_ptr())
    dimage, dvalue = z(K, n // spp), z(K, n)
    t = [_cu(np.asarray(a, np.float32)) for a in (x.dn, x.dw, x.da, x.dl)]
    wv.tangent(head, rows(t[0]), t[1].data_ptr() if weighted else None, t[2].data_ptr(), t[3].data_ptr(), dimage.data_ptr(),
               dvalue.data_ptr())
    torch.cuda.synchronize()
    g = types.SimpleNamespace(image=_np(image), value=_np(value), dimage=_np(dimage), dvalue=_np(dvalue), gn=_np(gn),
                              ga=_np(ga), g4=_np(gl))
    g.gw = _np(gw) if weighted else None
    return g


def _reference(wv, lights, x, vis, spp, weighted=True):
    return R.evaluate(lights, wv.np["sh_n"], wv.np["d"], x, wv.np["alpha"], ETA, vis, spp, weighted=weighted)


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, oi, face_normals):
    sc = _scene(hf, oracle, oi, face_normals)
    x = R.inputs(sc.n, SPP, K8)
    assert np.array_equal(x.w, sc.w)
    rigs = (tuple(range(K8)), TRIO) + tuple((k,) for k in range(K8))       # K = 8, K = 3, each light alone
    for kind, cases in (("row", tuple((ks, weighted) for ks in rigs for weighted in (True, False))),
                        ("sharp", ((tuple(range(K8)), True),))):
        wv = _Wave(hf, sc, kind=kind)
        worst = {k: 0.0 for k in TOL[kind]}
        for ks, weighted in cases:
            lights, xs, vis = [sc.ref[k] for k in ks], _sel(x, ks), sc.vis[list(ks)]
            ref = _reference(wv, lights, xs, vis, SPP, weighted)
            got = _all(wv, lights, xs, vis, SPP, weighted)
            if kind == "row" and weighted:      # (the public function's launch gave the same bits)
                assert np.array_equal(got.image, sc.img[list(ks)]) and np.array_equal(got.value, sc.val[list(ks)])
            # every sample takes part: the masks of both sides are the byte and the double cosines
            assert got.value.shape == ref.value.shape == (len(ks), sc.n) and np.array_equal(got.value > 0, ref.value > 0)
            assert not got.value[~vis].any() and not got.dvalue[~vis].any()
            dark = ~vis.any(0)
            for k in ("gn", "gw", "ga"):
                assert getattr(got, k) is None or not getattr(got, k)[..., dark].any()  # exact zeros where vis = 0
            # (`below` alone lights only the few steep slopes that face it, far from their highlight)
            assert ref.value.max() > (1e-3 if ks == (D.NAMES.index("below"),) else 0.05), (ks, ref.value.max())
            assert np.abs(ref.g4[:, 3]).min() > 0 and (np.abs(ref.g4[:, :3]).max(1) > 0).all() and np.abs(ref.ga).max() > 0
            err = R.errors(got, ref)
            print(kind, [D.NAMES[k] for k in ks], weighted, {k: "%.3g" % v for k, v in err.items()})
            for k, v in err.items():
                worst[k] = max(worst[k], v)
        print("worst", kind, {k: "%.3g / %.3g" % (worst[k], TOL[kind][k]) for k in TOL[kind]})
        for k in TOL[kind]:
            assert worst[k] <= TOL[kind][k], (kind, k, worst[k], TOL[kind][k])


@pytest.mark.parametrize("oi,face_normals", COMBOS)
def test_one_launch_of_eight_equals_eight_launches_of_one_and_a_launch_of_three_bit_for_bit(hf, oracle, oi, face_normals):
    """a light's arithmetic does not depend on its neighbours; light k alone reads bit 0 of the byte it is given"""
    sc = _scene(hf, oracle, oi, face_normals)
    kw = dict(eta=ETA, spp=SPP, weight=_cu(sc.w), return_value=True)
    al = _cu(sc.alpha["row"])
    for k in range(K8):
        img, val = hf.specular_lighting(sc.si, sc.ray, sc.lights[k], (sc.vis8 >> k) & 1, al, **kw)
        assert img.shape == (1, sc.n // SPP) and val.shape == (1, sc.n)
        assert np.array_equal(_np(img)[0], sc.img[k]) and np.array_equal(_np(val)[0], sc.val[k]), D.NAMES[k]
    three = _cu(D.pack(sc.vis[list(TRIO)]))
    img, val = hf.specular_lighting(sc.si, sc.ray, [sc.lights[k] for k in TRIO], three, al, **kw)
    assert np.array_equal(_np(img), sc.img[list(TRIO)]) and np.array_equal(_np(val), sc.val[list(TRIO)])
    # the [K, 4] tensor that directional_lighting takes is the same rig
    tab = torch.tensor(np.stack([D.row4(L) for L in sc.ref]), dtype=torch.float64)
    img, val = hf.specular_lighting(sc.si, sc.ray, tab, sc.vis8, al, **kw)
    assert np.array_equal(_np(img), sc.img) and np.array_equal(_np(val), sc.val)


def test_transposition_on_the_device_through_backward_and_jvp_repeatability_and_the_users_own_tensors(hf, oracle):
    """<J u, v> = <u, J^T v> through the public function: forward_ad against backward, each light's parameters and a scalar
    alpha the user's own tensors; two runs give the same bits"""
    sc = _scene(hf, oracle, 0, False)
    x = R.inputs(sc.n, SPP, K8)
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    A0, dA = 0.25, 0.7
    runs = []
    for _ in range(2):
        si, wt = leaf_si(hf, sc), _cu(x.w).requires_grad_(True)
        alpha = torch.tensor(A0, requires_grad=True)
        par = [[f64(v).requires_grad_(True) for v in (L.to_light, L.irradiance)] for L in sc.ref]
        lights = [hf.DirectionalLight(*q) for q in par]
        img, val = hf.specular_lighting(si, sc.ray, lights, sc.vis8, alpha, eta=ETA, spp=SPP, weight=wt, return_value=True)
        ((img * _cu(x.gi)).sum() + (val * _cu(x.gv)).sum()).backward()
        with fwAD.dual_level():
            sid = leaf_si(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)))
            dual = [hf.DirectionalLight(fwAD.make_dual(f64(L.to_light), f64(x.dl[k, :3])),
                                        fwAD.make_dual(f64(L.irradiance), f64(x.dl[k, 3]))) for k, L in enumerate(sc.ref)]
            ti, tv = hf.specular_lighting(sid, sc.ray, dual, sc.vis8, fwAD.make_dual(torch.tensor(A0), torch.tensor(dA)), eta=ETA,
                                          spp=SPP, weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), return_value=True)
            ti, tv = fwAD.unpack_dual(ti).tangent.clone(), fwAD.unpack_dual(tv).tangent.clone()
        assert all(q[0].grad.shape == (3,) and q[1].grad.shape == () for q in par) and alpha.grad.shape == ()
        g4 = torch.stack([torch.cat([q[0].grad, q[1].grad.reshape(1)]) for q in par])
        runs.append((img.detach().clone(), val.detach().clone(), si.sh_frame.n.grad.clone(), wt.grad.clone(), alpha.grad.clone(),
                     g4, ti, tv))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                                    # everything: bitwise
    _, _, gn, gw, ga, g4, ti, tv = (_np(a) for a in runs[0])
    for k, (name, L) in enumerate(zip(D.NAMES, sc.ref)):                            # each light's own numbers
        assert g4[k, 3] != 0 and np.abs(g4[k, :3]).max() > 0, name
        l = D.unit(L)[0]
        assert abs(g4[k, :3] @ l) <= 4 * TOL["row"]["grad4"] * np.linalg.norm(g4[k, :3]), name   # orthogonal to l
    assert len({float(v) for v in g4[:, 3]}) == K8 and float(ga) != 0
    gap = transposition_gap(((ti, x.gi), (tv, x.gv)), ((gn, x.dn), (gw, x.dw), (ga, dA), (g4, x.dl)))
    # The bound comes from the device's own rounding, not from the float32 restatement's tolerances (which the
    # cancellation in D inflates a thousandfold).  Every per-sample tangent is one float32 rounding of a double expression
    # whose float32 factors F, G1(c_i), G1(c_o) and their derivatives carry a few ulp each: 8 ulp of 2^-24 per element, so
    # the left side is within 8 eps * mass of the exact bilinear form, mass = sum |tangent| |upstream|.  The adjoint side
    # rounds the same products regrouped by input (sh_n, weight, alpha, the lights), whose absolute sums may exceed the
    # mass through cancellation between the four groups: the project's factor 4 for another operation order.  A sign, a
    # factor or a dropped term in any derivative is of the order of the mass itself.
    mass = (np.abs(tv.astype(np.float64) * x.gv).sum() + np.abs(ti.astype(np.float64) * x.gi).sum())
    bound = (8 + 4 * 8) * 2.0 ** -24 * mass
    print("transposition gap", gap, "mass", mass, "bound", bound)
    assert mass > 0 and gap <= bound, (gap, mass, bound)


def _busiest(vis, n):
    """the start (a multiple of 64) of the window of n samples that holds the most visible ones"""
    c = np.concatenate([[0], np.cumsum(vis)])
    starts = np.arange(0, len(vis) - n + 1, 64)
    return int(starts[np.argmax(c[starts + n] - c[starts])])


def test_the_reduced_numbers_over_301_rows(hf, oracle):
    """n = 301 (more than one block, odd), spp 1: the K x 4 numbers against the float64 reverse sweep"""
    sc = _scene(hf, oracle, 1, True)
    lo = _busiest(sc.vis.sum(0), 301)
    wv = _Wave(hf, sc, lo, lo + 301)
    x = R.inputs(301, 1, K8, seed=8)
    vis = sc.vis[:, lo:lo + 301]
    print("visible of 301 per light", vis.sum(1))
    assert (vis.sum(1) >= 20).sum() >= 5, vis.sum(1)
    got = _all(wv, sc.ref, x, vis, 1)
    ref = _reference(wv, sc.ref, x, vis, 1)
    err = R.err_l2(got.g4, ref.g4)
    print("grad4 over 301 rows", err)
    assert err <= TOL["row"]["grad4"], err
    for k in range(K8):                                                             # (each row against its own norm)
        if np.abs(ref.g4[k]).max() > 0:
            assert R.err_l2(got.g4[k], ref.g4[k]) <= TOL["row"]["grad4"], (D.NAMES[k], got.g4[k], ref.g4[k])
        else:
            assert not got.g4[k].any()


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
    """HF_FORCE_GRID = 3: both grid-stride loops of the adjoint run 22 times per lane on 16384 samples and every light's
    slab has 3 rows; unforced, the same launch has 64 block rows per light.  The per-lane outputs are bitwise the same,
    the reduced numbers the same sums in another order and both within the tolerance of the float64 reverse sweep.  The
    forward and the tangent take one lane per sample: the hook does not reach them"""
    sc = _scene(hf, oracle, 0, True)
    wv = _Wave(hf, sc)
    x = R.inputs(sc.n, SPP, K8)
    assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 64
    free = _all(wv, sc.ref, x, sc.vis, SPP)
    with _env(3):
        assert hf._capi.lib().hf_grid_blocks(sc.n, 2) == 3
        forced = _all(wv, sc.ref, x, sc.vis, SPP)
    for k in ("image", "value", "gn", "gw", "ga", "dimage", "dvalue"):
        assert np.array_equal(getattr(free, k), getattr(forced, k)), k
    ref = _reference(wv, sc.ref, x, sc.vis, SPP)
    for got in (free, forced):
        for k in range(K8):
            assert R.err_l2(got.g4[k], ref.g4[k]) <= TOL["row"]["grad4"], (D.NAMES[k], got.g4[k], ref.g4[k])


def test_an_empty_wavefront_and_a_byte_of_zeros(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, val0 = hf.specular_lighting(si0, ray0, sc.lights, sc.vis8[:0], 0.3, spp=SPP, return_value=True)
    assert img0.shape == (K8, 0) and val0.shape == (K8, 0)
    img0.sum().backward()
    # a byte of zeros: exact zero outputs and gradients, the lights' and the scalar alpha's among them
    si, wt = leaf_si(hf, sc), torch.ones(sc.n, device="cuda", requires_grad=True)
    alpha = torch.tensor(0.3, requires_grad=True)
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (sc.ref[1].to_light, sc.ref[1].irradiance)]
    img, val = hf.specular_lighting(si, sc.ray, hf.DirectionalLight(*par), torch.zeros_like(sc.vis8), alpha, spp=SPP, weight=wt,
                                    return_value=True)
    assert not bool(img.any()) and not bool(val.any())
    (img.sum() + val.sum()).backward()
    assert not bool(si.sh_frame.n.grad.any()) and not bool(wt.grad.any()) and float(alpha.grad) == 0.0
    assert not bool(par[0].grad.any()) and float(par[1].grad) == 0.0
    # a foreign byte of ones: a lane whose cosines are not positive gets an exact zero, NaN-free
    img, val = hf.specular_lighting(sc.si, sc.ray, sc.lights, torch.full_like(sc.vis8, 255), _cu(sc.alpha["row"]), spp=SPP,
                                    return_value=True)
    ref = R.forward(sc.ref, sc.np["sh_n"], sc.np["d"], None, sc.alpha["row"], ETA, np.ones((K8, sc.n), bool), SPP)[1]
    assert bool(torch.isfinite(val).all()) and np.array_equal(_np(val) > 0, ref > 0) and (ref == 0).any() and (ref > 0).any()
    with pytest.raises(hf.HfError):       # (a rig the library refuses)
        bad = hf.DirectionalLight((0.0, 0.0, 1.0), 1.0)
        bad.irradiance = float("nan")
        hf.specular_lighting(sc.si, sc.ray, bad, sc.vis8, 0.3, spp=SPP)


@pytest.mark.parametrize("n,spp", [(1, 1), (63, 1), (65, 1), (257, 1), (3 * 151, 3), (4 * 65, 4)])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, n, spp):
    """n = 1, 63, 65, 257 (a part of a batch of 64, one more than a batch, more than a block), spp 3 (no power of two: the
    film's other paths, whose atomics add a pixel's samples in an order that may differ from launch to launch: its image
    is compared to rounding, everything else bit for bit) and 4, guard values around every output row of every light, and
    every optional pointer NULL in turn"""
    sc = _scene(hf, oracle, 1, True)
    G = 96
    lo = _busiest(sc.vis.sum(0), max(n, 64))
    wv = _Wave(hf, sc, lo, lo + n)
    x = R.inputs(n, spp, K8, seed=9)
    w = _cu(x.w)
    vis = sc.vis[:, lo:lo + n]
    vis8 = _cu(D.pack(vis))
    head = wv.head(spp, sc.ref, w, vis8.data_ptr())
    npix = n // spp
    tree = spp & (spp - 1) == 0         # the film's shuffle tree: one store per pixel; any other spp: float atomics
    tol = TOL["row"]

    def planes(m):
        """one buffer of K8 * m elements, the K rows m apart, with one guard band on either side"""
        buf = torch.full((K8 * m + 2 * G,), GUARD, device="cuda")
        return buf, buf.data_ptr() + 4 * G

    def forward(skip=None, h=head):
        image, ip = planes(npix); value, vp = planes(n)
        wv.forward(h, None if skip == "image" else ip, None if skip == "value" else vp)
        return {"image": image, "value": value}

    def whole(buf, m):
        return bool((buf[:G] == GUARD).all()) and bool((buf[G + K8 * m:] == GUARD).all()) and bool((buf[G:G + K8 * m] != GUARD).all())
    full = forward()
    assert whole(full["image"], npix) and whole(full["value"], n)
    assert n < 64 or vis.sum() >= 20
    ri, rv = R.forward(sc.ref, wv.np["sh_n"], wv.np["d"], x.w, wv.np["alpha"], ETA, vis, spp)
    assert R.err_abs(_np(full["image"][G:G + K8 * npix]).reshape(K8, npix), ri) <= tol["image"]
    assert R.err_abs(_np(full["value"][G:G + K8 * n]).reshape(K8, n), rv) <= tol["value"]
    for skip in ("image", "value"):
        part = forward(skip)
        for k in full:
            if k == skip:
                assert bool((part[k] == GUARD).all())                               # untouched
            elif k == "image" and not tree:
                assert torch.allclose(part[k], full[k], rtol=1e-6, atol=1e-7)       # (float atomics: the order differs)
            else:
                assert torch.equal(part[k], full[k]), (skip, k)
    # without a weight: the same film as with a weight of 1
    one_w = torch.ones(n, device="cuda")
    a, b = forward(h=wv.head(spp, sc.ref, None, vis8.data_ptr())), forward(h=wv.head(spp, sc.ref, one_w, vis8.data_ptr()))
    assert all(torch.equal(a[k], b[k]) or (k == "image" and not tree and torch.allclose(a[k], b[k], rtol=1e-6, atol=1e-7)) for k in a)
    # the adjoint: all outputs, then each one NULL in turn -- the others are bitwise what they were
    gi, gv = _cu(x.gi), _cu(x.gv)

    def adjoint(skip=None, gi_=gi, gv_=gv, ws=True):
        gn, gnp = guarded(n, G, 3); gw, gwp = guarded(n, G); ga, gap = guarded(n, G)
        o = {"gn": gn, "gw": gw, "ga": ga, "gl": torch.zeros((K8, D.PARAMS), device="cuda")}
        ptr = lambda k, v: None if skip == k else v
        wv.adjoint(head, _ptr(gi_), _ptr(gv_), ptr("gn", gnp), ptr("gw", gwp[0]), ptr("ga", gap[0]), ptr("gl", o["gl"].data_ptr()), ws=ws)
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("gn", "gw", "ga"))
    for skip in ("gn", "gw", "ga", "gl"):
        part = adjoint(skip, ws=skip != "gl")                                      # (no grad_lights: no workspace needed)
        for k in part:
            if k == skip:
                assert bool((part[k] == GUARD).all()) if k != "gl" else not bool(part[k].any())   # untouched
            else:
                assert torch.equal(part[k], fulla[k]), (skip, k)
    assert torch.equal(adjoint()["gl"], fulla["gl"])                                # bitwise repeatable
    ref = R.adjoint(sc.ref, wv.np["sh_n"], wv.np["d"], x.w, wv.np["alpha"], ETA, vis, spp, x.gi, x.gv)
    assert R.err_abs(_np(fulla["gn"])[:, G:G + n], ref.gn) <= tol["grad_sh_n"]
    assert R.err_abs(_np(fulla["ga"])[0, G:G + n], ref.ga) <= tol["grad_alpha"]
    assert R.err_abs(_np(fulla["gw"])[0, G:G + n], ref.gw) <= tol["grad_weight"]
    if np.abs(ref.g4).max() > 0:
        assert R.err_l2(_np(fulla["gl"]), ref.g4) <= tol["grad4"]
    # either upstream NULL in turn (grad_value alone, grad_image alone): each half against the restatement given that
    # half, and the two halves add up to the whole (the adjoint is linear in its upstream)
    halves = []
    for gi_, gv_, xi, xv in ((gi, None, x.gi, None), (None, gv, None, x.gv)):
        half = adjoint(gi_=gi_, gv_=gv_)
        assert all(intact(half[k], n, G) for k in ("gn", "gw", "ga"))
        rh = R.adjoint(sc.ref, wv.np["sh_n"], wv.np["d"], x.w, wv.np["alpha"], ETA, vis, spp, xi, xv)
        assert R.err_abs(_np(half["gn"])[:, G:G + n], rh.gn) <= tol["grad_sh_n"]
        assert R.err_abs(_np(half["ga"])[0, G:G + n], rh.ga) <= tol["grad_alpha"]
        assert R.err_abs(_np(half["gw"])[0, G:G + n], rh.gw) <= tol["grad_weight"]
        if np.abs(rh.g4).max() > 0:
            assert R.err_l2(_np(half["gl"]), rh.g4) <= tol["grad4"]
        halves.append(half)
    none = adjoint(gi_=None, gv_=None)                                           # no upstream at all: exact zeros
    assert all(not bool(none[k][..., G:G + n].any()) for k in ("gn", "gw", "ga")) and not bool(none["gl"].any())
    if vis.any():
        for k in ("gn", "gw", "ga", "gl"):
            cut = (lambda a: a) if k == "gl" else (lambda a: a[:, G:G + n])
            s2 = cut(_np(halves[0][k])).astype(np.float64) + cut(_np(halves[1][k]))
            assert np.abs(s2 - cut(_np(fulla[k]))).max() <= 1e-5 * np.abs(cut(_np(fulla[k]))).max(), k
    # the tangent: every tangent NULL in turn, and their sum is the whole (the map is linear)
    t = {k: _cu(np.asarray(v, np.float32)) for k, v in (("dn", x.dn), ("dw", x.dw), ("da", x.da), ("dl", x.dl))}

    def tangent(use, image=True, value=True):
        di, dip = planes(npix); dv, dvp = planes(n)
        q = lambda k: (rows(t[k]) if k == "dn" else t[k].data_ptr()) if k in use else None
        wv.tangent(head, q("dn"), q("dw"), q("da"), q("dl"), dip if image else None, dvp if value else None)
        assert (whole(di, npix) if image else bool((di == GUARD).all())) and (whole(dv, n) if value else bool((dv == GUARD).all()))
        return di, dv
    di, dv = tangent(tuple(t))
    assert torch.equal(tangent(tuple(t), value=False)[0], di) and torch.equal(tangent(tuple(t), image=False)[1], dv)
    assert torch.equal(tangent(tuple(t))[0], di) and torch.equal(tangent(tuple(t))[1], dv)     # bitwise repeatable, any spp
    cutv = lambda a: _np(a[G:G + K8 * n]).reshape(K8, n).astype(np.float64)
    parts = sum(cutv(tangent((k,))[1]) for k in t)
    assert not bool(tangent(())[1][G:G + K8 * n].any())
    wholev = cutv(dv)
    assert np.abs(wholev - parts).max() <= 4 * tol["dvalue"] * max(1.0, np.abs(wholev).max())   # (four results, each within its tolerance)
    assert np.abs(_np(di[G:G + K8 * npix]).reshape(K8, npix) - wholev.reshape(K8, -1, spp).mean(2)).max() <= 1e-6 * max(1.0, np.abs(wholev).max())
    rdi, rdv = R.tangent(sc.ref, wv.np["sh_n"], wv.np["d"], x.w, wv.np["alpha"], ETA, vis, spp, x.dn, x.dw, x.da, x.dl)
    assert R.err_abs(wholev, rdv) <= tol["dvalue"] and R.err_abs(_np(di[G:G + K8 * npix]).reshape(K8, npix), rdi) <= tol["dimage"]
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    """one captured graph of a single-stream forward + adjoint + tangent (no parallel branches), replayed: the capture
    succeeds only if no call allocates or synchronises the host"""
    sc = _scene(hf, oracle, 1, True)
    wv = _Wave(hf, sc)
    head = wv.head(SPP, sc.ref, None, sc.vis8.data_ptr())
    z = lambda *s: torch.zeros(s, device="cuda")
    img, val = z(K8, sc.n // SPP), z(K8, sc.n)
    gn, ga, gl, dimg, dval = z(3, sc.n), z(sc.n), z(K8, D.PARAMS), z(K8, sc.n // SPP), z(K8, sc.n)
    gi, ones, dl = torch.ones((K8, sc.n // SPP), device="cuda"), torch.ones((3, sc.n), device="cuda"), torch.ones((K8, D.PARAMS), device="cuda")

    def launch():
        gl.zero_()                                                       # (accumulated into)
        wv.forward(head, img.data_ptr(), val.data_ptr())
        wv.adjoint(head, gi.data_ptr(), None, rows(gn), None, ga.data_ptr(), gl.data_ptr())
        wv.tangent(head, rows(ones), None, ga.data_ptr(), dl.data_ptr(), dimg.data_ptr(), dval.data_ptr())
    outs = (img, val, gn, ga, gl, dimg, dval)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert float(img.abs().sum()) > 0 and float(gl[:, 3].abs().min()) > 0 and float(dval.abs().sum()) > 0
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
    assert bool(si.is_valid().all())
    return shape, si, ray


@pytest.mark.parametrize("eta", (1.5, 0.0))
def test_a_flat_field_seen_and_lit_from_the_zenith_has_the_known_value(hf, eta):
    """value = w E F(1, eta) / (4 pi a^2) with F(1, eta) = ((eta - 1) / (eta + 1))^2, and w E / (4 pi a^2) for the mirror"""
    shape, si, ray = _flat(hf)
    n = len(ray)
    zen = D.rig(("zenith",))[0]
    sun = _light(hf, zen)
    _, vis = hf.directional_lighting(shape, si, ray, sun, return_visibility=True)
    assert bool((vis == 1).all())
    w = np.linspace(0.5, 1.5, n).astype(np.float32)
    for a in (0.1, 0.3, 0.6):
        img, val = hf.specular_lighting(si, ray, sun, vis, a, eta=eta, weight=_cu(w), return_value=True)
        F = ((eta - 1) / (eta + 1)) ** 2 if eta else 1.0
        known = w.astype(np.float64) * zen.irradiance * F / (4 * np.pi * np.float64(np.float32(a)) ** 2)
        err = np.abs(_np(val)[0] - known).max() / max(1.0, known.max())
        print("eta", eta, "a", a, "known answer", err, "largest", known.max())
        assert err <= TOL["row"]["value"] and torch.equal(img, val)


def test_grazing_cosines_below_float32s_range_keep_every_derivative_finite(hf):
    """hand-placed lanes seen at c_i = 1e-20, 1e-15, 3e-14 and 1e-3 under the zenith light (c_o = 1), a foreign byte: the
    float32 G1(c_i) or its derivatives leave float32's range on the first lanes (hf.h: their d ln G1 counts as 0); the
    value is finite and tends to 0, and every gradient and tangent is finite"""
    ci = np.array([1e-20, 1e-15, 3e-14, 1e-3], np.float32)
    n = len(ci)
    sn = torch.tensor([[0.0] * n, [0.0] * n, [1.0] * n], device="cuda", requires_grad=True)
    d = _cu(-np.stack([np.sqrt(1 - ci.astype(np.float64) ** 2).astype(np.float32), np.zeros(n, np.float32), ci]))
    si = types.SimpleNamespace(sh_frame=types.SimpleNamespace(n=sn))
    ray = types.SimpleNamespace(d=d)
    alpha = torch.full((n,), 0.3, device="cuda", requires_grad=True)
    wt = torch.ones(n, device="cuda", requires_grad=True)
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in ((0.0, 0.0, 1.0), 3.0)]
    vis = torch.ones(n, dtype=torch.uint8, device="cuda")
    img, val = hf.specular_lighting(si, ray, hf.DirectionalLight(*par), vis, alpha, eta=ETA, weight=wt, return_value=True)
    val.sum().backward()
    got = [_np(v) for v in (val, sn.grad, alpha.grad, wt.grad, par[0].grad, par[1].grad)]
    print("grazing lanes", got[0], got[2])
    assert all(np.isfinite(g).all() for g in got)
    assert (got[0] >= 0).all() and got[0][0, 3] > 0 and got[0][0, 0] <= got[0][0, 3]
    with fwAD.dual_level():
        sid = types.SimpleNamespace(sh_frame=types.SimpleNamespace(n=fwAD.make_dual(sn.detach(), torch.ones_like(sn))))
        tv = hf.specular_lighting(sid, ray, hf.DirectionalLight((0.0, 0.0, 1.0), 3.0), vis,
                                  fwAD.make_dual(alpha.detach(), torch.ones(n, device="cuda")), eta=ETA, return_value=True)[1]
        assert bool(torch.isfinite(fwAD.unpack_dual(tv).tangent).all())


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """ray_intersect -> directional_lighting (vis) -> specular_lighting -> loss -> backward() -> shape.heightfield.grad
    against the restatement's grad_sh_n (fed with the GPU's records and byte), carried to the heights by the oracle's
    adjoint (flat shading) or by hf_adjoint (smooth shading).  Bound: the directional row's for its chain."""
    sc = _scene(hf, oracle, 0, face_normals)
    x = R.inputs(sc.n, SPP, K8)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    _, vis = hf.directional_lighting(shape, si, sc.ray, sc.lights, spp=SPP, return_visibility=True)
    assert np.array_equal(_np(vis), sc.byte)
    img = hf.specular_lighting(si, sc.ray, sc.lights, vis, _cu(sc.alpha["row"]), eta=ETA, spp=SPP)
    (img * _cu(x.gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    g = R.adjoint(sc.ref, _np(si.sh_frame.n), sc.np["d"], None, sc.alpha["row"], ETA, sc.vis, SPP, x.gi)
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


@pytest.mark.parametrize("heights", [False, True])
def test_inverse_highlight_example_descends(hf, heights):
    import inverse_highlight
    hist, err0, err, herr0, herr = inverse_highlight.run(size=48, steps=31, heights=heights, verbose=False)
    print("heights" if heights else "roughness", "loss", hist[0], "->", hist[30], "roughness error", err0, "->", err,
          "centred height error", herr0, "->", herr)
    assert np.isfinite(hist[-1]) and hist[30] < hist[0], (hist[0], hist[30])
    assert err < err0, (err0, err)
    if heights:
        assert herr < herr0, (herr0, herr)

"""The bump map on the GPU (hf_bumpmap_eval, _tangent, _adjoint; hf_amd.BumpMap) on the scenes of tests/row_scenes.py
(CASES, the view `steep`: 25 x 23 x 4 wavefronts under to_world, flip_normals and a view from below, flat and smooth
shading), with the textures of bumpmap_ref.TEXTURES (37 x 29 and 16 x 8, bumpmap_ref.texture) under both wraps and both
scales of bumpmap_ref.SCALES.
  (1) N, dN, grad_uv, grad_sh_n, grad_dp_du, grad_dp_dv per component and grad_tex as a relative L2 against the float64
      restatement within the table, the mask bitwise;
  (2) the lookup: with (Lx, Ly) taken from hf_bitmap_eval's out_grad at the same pos, the fused N equals the float64 frame
      algebra within one float32 ulp at 1 (2^-23 absolute);
  (3) the transposition on the device through backward and jvp with all five inputs attached; forward, tangent and the
      per-sample gradients bitwise repeatable, grad_tex to rounding;
  (4) the merged scatter on a wavefront where runs occur and on one where every lane has a cell of its own;
  (5) the known answers of tests/test_bumpmap_ref.py: the ramp, and the flipped geometric normal;
  (6) the flat map: perturb returns sh_frame.n within 2^-22, and directional_lighting of the perturbed interaction the
      unperturbed image within that row's tolerance;
  (7) the chain ray_intersect -> BumpMap.normal -> directional_lighting -> sum -> dL/dheight, flat and smooth shading;
  (8) the hand-placed pass-through lanes of tests/test_bumpmap_ref.py: exact copies, identity gradient, no texel touched;
  (9) n = 1, 63, 65, 257 and 3 * 151 with guard bands, every optional pointer NULL in turn; textures 1 x 1, 1 x 5, 2 x 2
      and 37 x 29 with uv stretched to [-1, 2]^2 under both wraps;
  (10) a captured graph of forward, tangent and adjoint replays to the same bits, grad_tex to rounding;
  (11) examples/inverse_bumpmap.py descends.
None of the three kernels is grid-stride (one lane per sample, a grid of ceil(n / 256) blocks): there is no loop to take
beyond its first iteration.

Tolerances (scripts/bumpmap_f32_error.py computes them on the CPU, profiles/bumpmap/f32_error.json): the
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records, by at
most the figures of bumpmap_ref.F32, kept per texture and scale (per component as the largest difference over max(1, the
largest value); grad_tex as a relative L2).  The GPU is allowed four times that (bumpmap_ref.TOL).  Samples whose position
in the cell is within bumpmap_ref.MARGIN of a cell edge -- the slopes jump there -- are left out of every comparison and
get zero tangents and a zero upstream gradient, at most row_helpers.UNSURE_CAP of the hits; asserted, with the other
conditions on the inputs (every hit perturbed, none near the pass-through threshold, |<n_geo, c / |c|>| >= 0.2, sigma = -1
on `mirror_flip`), on the GPU's own records before anything is compared."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import bumpmap_ref as R
import directional_ref as D
import row_scenes as RS
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, guarded, intact, rows
from test_bumpmap_ref import _axis_lanes, pass_through_lanes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ULP = 2.0 ** -23
WRAP_NAMES = ("clamp", "repeat")
COMBOS = [(TW, TH, w, s) for TW, TH in R.TEXTURES for w in WRAP_NAMES for s in R.SCALES]
_SCENES = {}


def _scene(hf, oracle, name, face_normals):
    """a scene of row_scenes on the device, once, with the records the map reads as numpy and the asserted conditions"""
    key = (name, face_normals)
    if key not in _SCENES:
        sc = RS.device_scene(hf, oracle, name, "steep", face_normals)
        sc.rec = {"uv": _np(sc.si.uv), "sh_n": _np(sc.si.sh_frame.n), "n": _np(sc.si.n), "dp_du": _np(sc.si.dp_du),
                  "dp_dv": _np(sc.si.dp_dv), "hit": sc.hit}
        sc.active = _cu(sc.hit.astype(np.uint8))
        sc.keep, negative = {}, 0
        for TW, TH, wname, scale in COMBOS:
            _, _, s = R.forward(R.texture(TW, TH), *R.record_args(sc.rec), sc.hit, R.WRAPS[wname], scale)
            sh = R.shares(s, sc.hit)
            print(name, face_normals, (TW, TH), wname, scale, sh)
            R.conditions(sh, UNSURE_CAP)                    # (asserted before anything is compared)
            negative += sh["sigma_negative"]
            sc.keep[(TW, TH, wname, scale)] = ~R.near_edge(s)
        assert negative > 0 or name != "mirror_flip"
        _SCENES[key] = sc
    return _SCENES[key]


class _Wave:
    """device rows of a wavefront, a texture, a wrap and a scale, and the three C calls on them"""

    def __init__(self, hf, uv, sh_n, n_geo, dp_du, dp_dv, active, tex, wname, scale):
        f = lambda x: (x if isinstance(x, torch.Tensor) else _cu(np.asarray(x, np.float32))).detach().contiguous()
        self.uv, self.sn, self.ng, self.du, self.dv, self.tex = f(uv), f(sh_n), f(n_geo), f(dp_du), f(dp_dv), f(tex)
        self.active = None if active is None else (active if isinstance(active, torch.Tensor) else _cu(np.asarray(active, np.uint8)))
        self.n, self.wrap, self.scale = self.uv.shape[1], R.WRAPS[wname], float(scale)
        self.lib, self.check = hf._capi.lib(), hf._capi.check

    def head(self, active=True):
        act = self.active.data_ptr() if (active and self.active is not None) else None
        return (self.n, rows(self.uv), rows(self.sn), rows(self.ng), rows(self.du), rows(self.dv), act, self.tex.shape[1],
                self.tex.shape[0], self.tex.data_ptr(), self.wrap, self.scale)

    def forward(self, out, mask=None, active=True):
        self.check(self.lib.hf_bumpmap_eval(*self.head(active), out, mask, torch.cuda.current_stream().cuda_stream))

    def tangent(self, out, dtex=None, duv=None, dn=None, dpu=None, dpv=None):
        q = lambda x: None if x is None else rows(x)
        self.check(self.lib.hf_bumpmap_eval_tangent(*self.head(), None if dtex is None else dtex.data_ptr(), q(duv), q(dn), q(dpu),
                                                    q(dpv), out, torch.cuda.current_stream().cuda_stream))

    def adjoint(self, gout, gtex=None, guv=None, gn=None, gpu=None, gpv=None):
        self.check(self.lib.hf_bumpmap_eval_adjoint(*self.head(), rows(gout), None if gtex is None else gtex.data_ptr(), guv, gn, gpu,
                                                    gpv, torch.cuda.current_stream().cuda_stream))

    def evaluate(self, x, keep):
        """forward, tangent and adjoint under the inputs x: the dict of bumpmap_ref.evaluate, as numpy"""
        z = lambda *s: torch.zeros(s, device="cuda")
        N, dN, mask = z(3, self.n), z(3, self.n), torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        gtex, guv, gn, gpu, gpv = torch.zeros_like(self.tex), z(2, self.n), z(3, self.n), z(3, self.n), z(3, self.n)
        t = [_cu(np.ascontiguousarray(a, np.float32)) for a in (x.dtex, x.duv * keep, x.db * keep, x.ddu * keep, x.ddv * keep,
                                                                 x.gout * keep)]
        if self.n:
            self.forward(rows(N), mask.data_ptr())
            self.tangent(rows(dN), *t[:5])
            self.adjoint(t[5], gtex, rows(guv), rows(gn), rows(gpu), rows(gpv))
        torch.cuda.synchronize()
        return {"N": _np(N), "mask": _np(mask).astype(bool), "dN": _np(dN), "grad_uv": _np(guv), "grad_sh_n": _np(gn),
                "grad_dp_du": _np(gpu), "grad_dp_dv": _np(gpv), "grad_tex": _np(gtex)}


def _scene_wave(hf, sc, TW, TH, wname, scale, lo=0, hi=None, seed=0):
    hi = sc.n if hi is None else hi
    cut = lambda v: v.detach()[..., lo:hi].contiguous()
    return _Wave(hf, cut(sc.si.uv), cut(sc.si.sh_frame.n), cut(sc.si.n), cut(sc.si.dp_du), cut(sc.si.dp_dv), cut(sc.active),
                 R.texture(TW, TH, seed), wname, scale)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, name, face_normals):
    sc = _scene(hf, oracle, name, face_normals)
    for TW, TH, wname, scale in COMBOS:
        tex = R.texture(TW, TH)
        x = R.inputs(sc.n, tex.shape)
        tol = R.TOL[R.table_key(TW, TH, scale)]
        keep = sc.keep[(TW, TH, wname, scale)]
        got = _scene_wave(hf, sc, TW, TH, wname, scale).evaluate(x, keep)
        ref = R.evaluate(tex, *R.record_args(sc.rec), sc.hit, R.WRAPS[wname], scale, x, keep)
        assert np.array_equal(got["mask"], ref["mask"]) and got["mask"][sc.hit].all() and not got["mask"][~sc.hit].any()
        miss = ~sc.hit
        for k in ("grad_uv", "grad_dp_du", "grad_dp_dv"):
            assert not got[k][:, miss].any(), k                                                  # exact zeros
        assert np.array_equal(got["N"][:, miss].view(np.uint32), sc.rec["sh_n"][:, miss].view(np.uint32))   # a copy
        assert np.array_equal(got["grad_sh_n"][:, miss], (x.gout * keep)[:, miss])
        assert np.array_equal(got["dN"][:, miss], (x.db * keep)[:, miss])
        for k in R.KEYS[1:]:
            assert np.abs(ref[k]).max() > 1e-3, k
        cosine = (ref["N"] * sc.rec["sh_n"]).sum(0)[sc.hit]
        # (the map does something: a tilt of 2.5 degrees is 1e4 times any tolerance here; the weakest combination, 16 x 8 at
        # scale 1 on a flat-shaded scene, tilts by 5.5 degrees in the median)
        assert np.median(cosine) < 0.999
        err = R.errors(got, ref, keep)
        print(name, face_normals, (TW, TH), wname, scale, "left out", int((~keep & sc.hit).sum()),
              {k: "%.3g / %.3g" % (v, tol[k]) for k, v in err.items()})
        for k, v in err.items():
            assert v <= tol[k], (k, v, tol[k], (TW, TH, wname, scale))


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_fused_normal_is_the_frame_algebra_on_the_bitmaps_slopes_within_one_ulp(hf, oracle, name, face_normals):
    sc = _scene(hf, oracle, name, face_normals)
    lib, check = hf._capi.lib(), hf._capi.check
    for TW, TH, wname, scale in COMBOS:
        tex = _cu(R.texture(TW, TH))
        N, mask = hf.BumpMap(tex, scale=scale, wrap=wname).normal(sc.si, active=sc.active, return_mask=True)
        # pos as the kernel forms it: one float32 product per coordinate
        pos = torch.stack([sc.si.uv[0].detach() * float(TW), sc.si.uv[1].detach() * float(TH)]).contiguous()
        L, slopes = torch.zeros(sc.n, device="cuda"), torch.zeros((2, sc.n), device="cuda")
        check(lib.hf_bitmap_eval(sc.n, rows(pos), sc.active.data_ptr(), TW, TH, tex.data_ptr(), R.WRAPS[wname], L.data_ptr(),
                                 rows(slopes), torch.cuda.current_stream().cuda_stream))
        Lx, Ly = _np(slopes)
        s = R.frame(Lx, Ly, np.isfinite(sc.rec["uv"]).all(0), sc.rec["sh_n"], sc.rec["n"], sc.rec["dp_du"], sc.rec["dp_dv"], TW, TH,
                    np.float32(scale), sc.hit)
        assert np.array_equal(_np(mask).astype(bool), s.pert) and s.pert[sc.hit].all() and not s.pert[~sc.hit].any()
        err = np.abs(_np(N).astype(np.float64) - s.N).max()
        print(name, face_normals, (TW, TH), wname, scale, "largest |N - restatement|", err, "in ulps at 1:", err / ULP)
        assert err <= ULP, err
        assert np.abs(Lx).max() > 0 and np.abs(Ly).max() > 0


def _leaf_si(hf, sc, uv, sh_n, dp_du, dp_dv):
    si = hf.SurfaceInteraction3f()
    si.uv, si.dp_du, si.dp_dv, si.sh_frame = uv, dp_du, dp_dv, hf.Frame3f(None, None, sh_n)
    si.p, si.n, si.t = sc.si.p.detach(), sc.si.n.detach(), sc.si.t.detach()
    return si


def test_transposition_on_the_device_through_backward_and_jvp_and_repeatability(hf, oracle):
    """<J u, v> = <u, J^T v> through the public class with the texels, uv, sh_n, dp_du and dp_dv attached: forward_ad against
    backward, both sides float32 results added up in float64.  Each side is within its tolerance of the exact bilinear form,
    so by Cauchy-Schwarz the gap is at most the sum over the quantities of (tolerance x the quantity's scale x the root of
    its size x the L2 norm of what it is paired with); grad_tex, held as a relative L2, enters with its own norm.  Lanes
    near a cell edge get zero tangents and gradients, as everywhere"""
    sc = _scene(hf, oracle, "affine", False)
    TW, TH = R.TEXTURES[0]
    scale = R.SCALES[1]
    tol = R.TOL[R.table_key(TW, TH, scale)]
    tex = R.texture(TW, TH)
    x = R.inputs(sc.n, tex.shape)
    keep = sc.keep[(TW, TH, "repeat", scale)]
    gout, tang = x.gout * keep, (x.dtex, x.duv * keep, x.db * keep, x.ddu * keep, x.ddv * keep)
    leaves = lambda: [v.detach().clone().requires_grad_(True) for v in (_cu(tex), sc.si.uv, sc.si.sh_frame.n, sc.si.dp_du, sc.si.dp_dv)]
    runs = []
    for _ in range(2):
        data, uv, sn, du, dv = leaves()
        bm = hf.BumpMap(data, scale=scale, wrap="repeat")
        N, mask = bm.normal(_leaf_si(hf, sc, uv, sn, du, dv), active=sc.active, return_mask=True)
        (N * _cu(gout)).sum().backward()
        with fwAD.dual_level():
            dual = [fwAD.make_dual(v.detach(), _cu(t)) for v, t in zip((data, uv, sn, du, dv), tang)]
            out = hf.BumpMap(dual[0], scale=scale, wrap="repeat").normal(_leaf_si(hf, sc, *dual[1:]), active=sc.active)
            dN = fwAD.unpack_dual(out).tangent.clone()
        runs.append((N.detach().clone(), mask.clone(), dN, uv.grad.clone(), sn.grad.clone(), du.grad.clone(), dv.grad.clone(),
                     data.grad.clone()))
    for a, b in zip(runs[0][:7], runs[1][:7]):
        assert torch.equal(a, b)                                                  # bitwise
    N, mask, dN, guv, gn, gpu, gpv, gtex = (_np(a) for a in runs[0])
    again = R.err_l2(_np(runs[1][7]), gtex.astype(np.float64))
    print("grad_tex run to run, relative L2", again)
    assert again <= tol["grad_tex"]                                                # float atomics: the order is free
    pairs = ((gtex, tang[0]), (guv, tang[1]), (gn, tang[2]), (gpu, tang[3]), (gpv, tang[4]))
    gap = abs((dN.astype(np.float64) * gout).sum() - sum((g.astype(np.float64) * t).sum() for g, t in pairs))
    norm = np.linalg.norm
    scale_of = lambda a: max(1.0, float(np.abs(a).max()))
    bound = tol["dN"] * scale_of(dN) * np.sqrt(dN.size) * norm(gout) + tol["grad_tex"] * norm(gtex) * norm(x.dtex)
    for k, (g, t) in zip(("grad_uv", "grad_sh_n", "grad_dp_du", "grad_dp_dv"), pairs[1:]):
        bound += tol[k] * scale_of(g) * np.sqrt(g.size) * norm(t)
    print("transposition gap", gap, "bound", bound, "<J u, v>", (dN.astype(np.float64) * gout).sum())
    assert norm(dN) > 0 and all(norm(g) > 0 for g, _ in pairs) and gap <= bound, (gap, bound)


def _run_share(state, pert):
    """the share of perturbed lanes whose cell is their predecessor's in the wave: the lanes a run absorbs"""
    j = state.e.idx
    same = (j[0, 1:] == j[0, :-1]) & (j[3, 1:] == j[3, :-1]) & pert[1:] & pert[:-1] & (np.arange(1, len(pert)) % 64 != 0)
    return float(same.sum() / max(pert.sum(), 1))


def test_the_merged_scatter_with_runs_and_without(hf, oracle):
    """the scene's wavefront as it is -- 4 samples per pixel, pixels smaller than the 16 x 8 texels: most lanes share their
    predecessor's cell -- and the same samples dealt out so that no two neighbouring lanes share one: grad_tex of both
    within the table's figure of the float64 adjoint, which is the same sum in either order"""
    sc = _scene(hf, oracle, "affine", True)
    TW, TH = R.TEXTURES[1]
    scale, wname = R.SCALES[0], "repeat"
    tol = R.TOL[R.table_key(TW, TH, scale)]["grad_tex"]
    tex = R.texture(TW, TH)
    keep = sc.keep[(TW, TH, wname, scale)]
    gout = R.inputs(sc.n, tex.shape).gout * keep
    a = (*R.record_args(sc.rec), sc.hit, R.WRAPS[wname], scale)
    _, pert, s = R.forward(tex, *a)
    ref = R.adjoint(tex, *a, gout).gtex
    # a stride that is coprime to n and half the film long: neighbouring lanes are 11 rows of pixels apart
    stride = 1151
    assert np.gcd(stride, sc.n) == 1
    perm = (np.arange(sc.n) * stride) % sc.n
    shares = []
    for order in (np.arange(sc.n), perm):
        rec = {k: np.ascontiguousarray(v[..., order]) for k, v in sc.rec.items()}
        _, p2, s2 = R.forward(tex, *R.record_args(rec), rec["hit"], R.WRAPS[wname], scale)
        shares.append(_run_share(s2, p2))
        wv = _Wave(hf, *R.record_args(rec), rec["hit"].astype(np.uint8), tex, wname, scale)
        gtex = torch.zeros_like(wv.tex)
        wv.adjoint(_cu(np.ascontiguousarray(gout[:, order])), gtex)
        torch.cuda.synchronize()
        err = R.err_l2(_np(gtex), ref)
        print("share of lanes in their predecessor's cell", shares[-1], "grad_tex relative L2", err, "/", tol)
        assert err <= tol, (shares[-1], err)
    assert shares[0] > 0.5 and shares[1] == 0.0, shares


@pytest.mark.parametrize("axis", ["u", "v"])
def test_a_ramp_and_a_flipped_geometric_normal_on_the_device(hf, axis):
    """tests/test_bumpmap_ref.py's known answer: N = (-scale k, 0, Sx) / sqrt(scale^2 k^2 + Sx^2) for a ramp in u (in v
    likewise).  The float32 texels k (i + 0.5) / T are each rounded by at most 2^-24 k, their difference by 2^-23 k, so
    g = scale T L is off by at most scale T k 2^-23 (the weights of a linear ramp add up to 1 and add a few 2^-24 of L:
    a factor 1.1), N by that over |c| = sqrt(g^2 + S^2), plus its own rounding 2^-24.  n_geo = (0, 0, -1): -N, bit for bit"""
    TW, TH, k, scale, Sx, Sy = 9, 6, 0.8, 1.75, 1.5, 0.6
    y, x = np.meshgrid((np.arange(TH) + 0.5) / TH, (np.arange(TW) + 0.5) / TW, indexing="ij")
    tex = (k * (x if axis == "u" else y)).astype(np.float32)
    uv, b, ng, u, v = _axis_lanes(333, Sx, Sy)
    S, T = (Sx, TW) if axis == "u" else (Sy, TH)
    want = np.zeros(3)
    want[0 if axis == "u" else 1], want[2] = -scale * k, S
    want /= np.hypot(scale * k, S)
    bound = 1.1 * scale * T * k * ULP / np.hypot(scale * k, S) + 2.0 ** -24
    out = {}
    for side in (1.0, -1.0):
        wv = _Wave(hf, uv, b, side * ng, u, v, None, tex, "clamp", scale)
        N, mask = torch.zeros((3, wv.n), device="cuda"), torch.zeros(wv.n, dtype=torch.uint8, device="cuda")
        wv.forward(rows(N), mask.data_ptr())
        torch.cuda.synchronize()
        assert bool(mask.all())
        out[side] = _np(N)
    err = np.abs(out[1.0] - want[:, None]).max()
    print(axis, "largest |N - known answer|", err, "bound", bound)
    assert err <= bound
    assert np.array_equal(out[-1.0].view(np.uint32), (-out[1.0]).view(np.uint32))


def _rig(hf, sc):
    _, lights = RS.rig("directional", sc)
    return lights, [hf.DirectionalLight(L.to_light, L.irradiance) for L in lights]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_flat_map_gives_the_base_normal_to_rounding(hf, oracle, name, face_normals):
    """g = 0: N is parallel to sh_n but formed anew from the projected tangents (the header says so): within 2^-22 per
    component, and directional_lighting of the perturbed interaction within that row's tolerance of the unperturbed image
    on the pixels none of whose samples has <sh_n, l> or <sh_n, -d> within directional_ref.MARGIN of zero.

    MEASURED (MI355X): the largest |N - sh_n| is 1.19e-7 = 0.5 x 2^-22 on all four scenes -- N is sh_n / |sh_n| within 3.0e-8,
    and ||sh_n| - 1| reaches 1.3e-7 -- and the image differs by 1.2e-7 of the allowed 5.8e-7.  [affine-False], smooth shading,
    is the case that the projection's division by <b, b> is there for: with the reference's k = 1 a normal of length
    1 + eps / 2 leaves the projected tangents a component -eps <b, dp_du> along b, c leaves b's direction by about eps tan(theta)
    -- b is not orthogonal to the face's tangents under smooth shading -- and the case measured 2.68e-7 = 1.125 x 2^-22.
    The figures are printed before the assert."""
    sc = _scene(hf, oracle, name, face_normals)
    ref_lights, lights = _rig(hf, sc)
    base = hf.directional_lighting(sc.shape, sc.si, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP)
    unsure = np.zeros(sc.n, bool)
    for L in ref_lights:
        unsure |= D.traced(L, sc.np["sh_n"], sc.np["d"], sc.np["t"])[1]
    assert unsure.mean() <= UNSURE_CAP
    pix = ~unsure.reshape(-1, RS.SPP).any(1)
    hit = sc.active.bool()
    for wname in WRAP_NAMES:
        for TW, TH in ((37, 29), (1, 1)):
            bm = hf.BumpMap.flat(TW, TH, device="cuda", scale=2.5, wrap=wname)
            si = bm.perturb(sc.si, active=sc.active)
            assert si is not sc.si and si.p is sc.si.p
            _, mask = bm.normal(sc.si, active=sc.active, return_mask=True)
            assert bool(mask[hit].all())                                          # (perturbed lanes, not copies)
            diff = float((si.sh_frame.n - sc.si.sh_frame.n)[:, hit].abs().max())
            b64 = sc.rec["sh_n"][:, sc.hit].astype(np.float64)
            unit = b64 / np.linalg.norm(b64, axis=0)
            print(name, face_normals, (TW, TH), wname, "largest |N - sh_n|", diff, "in 2^-22:", diff / 2.0 ** -22,
                  "largest ||sh_n| - 1|", np.abs(np.linalg.norm(b64, axis=0) - 1).max(), "largest |N - sh_n / |sh_n||",
                  np.abs(_np(si.sh_frame.n)[:, sc.hit] - unit).max())
            assert diff <= 2.0 ** -22
            assert torch.equal(si.sh_frame.n[:, ~hit], sc.si.sh_frame.n[:, ~hit])
            lit = hf.directional_lighting(sc.shape, si, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP)
            err = R.err_abs(_np(lit)[:, pix], _np(base)[:, pix].astype(np.float64))
            print("image", err, "/", RS.TOL["directional"]["image"])
            assert err <= RS.TOL["directional"]["image"]
    assert float(base.abs().sum()) > 0


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_chain_to_the_heights(hf, oracle, name, face_normals):
    """ray_intersect -> BumpMap.normal -> directional_lighting -> loss -> backward() -> shape.heightfield.grad against the
    restatements' gradients (directional_ref.adjoint for dL/dN, bumpmap_ref.adjoint for dL/d(uv, sh_n, dp_du, dp_dv), fed with
    the GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Measure and bound:
    tests/test_gpu_directional.py::test_chain_to_the_heights' (row_scenes.CHAIN)."""
    sc = _scene(hf, oracle, name, face_normals)
    ref_lights, lights = _rig(hf, sc)
    K = len(lights)
    TW, TH = R.TEXTURES[0]
    scale = R.SCALES[0]
    tex = R.texture(TW, TH)
    x = D.inputs(sc.n, RS.SPP, K)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    bm = hf.BumpMap(_cu(tex), scale=scale, wrap="repeat")
    lit = bm.perturb(si, active=sc.active)
    N = _np(lit.sh_frame.n)
    img, vis = hf.directional_lighting(shape, lit, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP, return_visibility=True)
    vis = D.unpack(_np(vis), K)
    # samples on which rounding may decide a mask of the lighting row, or the cell of the lookup, are left out of the loss
    edge = ~sc.keep[(TW, TH, "repeat", scale)] & sc.hit
    unsure = np.zeros(sc.n, bool)
    for L in ref_lights:
        unsure |= D.traced(L, N, sc.np["d"], sc.np["t"])[1]
    assert unsure.mean() <= UNSURE_CAP and edge.mean() <= UNSURE_CAP, (unsure.mean(), edge.mean())
    unsure |= edge
    gi = np.where(~unsure.reshape(-1, RS.SPP).any(1)[None], x.gi, 0).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    gN = D.adjoint(ref_lights, N, None, D.ALBEDO, vis, RS.SPP, gi).gn
    rec = {"uv": _np(si.uv), "sh_n": _np(si.sh_frame.n), "n": _np(si.n), "dp_du": _np(si.dp_du), "dp_dv": _np(si.dp_dv)}
    g = R.adjoint(tex, *R.record_args(rec), sc.hit, R.REPEAT, scale, gN)
    up = {"uv": g.guv.astype(np.float32), "sh_n": g.gn.astype(np.float32), "dp_du": g.gpu.astype(np.float32),
          "dp_dv": g.gpv.astype(np.float32)}
    if face_normals:
        t, u, v, prim = sc.pi_oracle
        gh = sc.field.adjoint(sc.rays, t, u, v, prim, up, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[7:9], ybar[9:12], ybar[12:15], ybar[15:18] = _cu(up["uv"]), _cu(up["sh_n"]), _cu(up["dp_du"]), _cu(up["dp_dv"])
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    parts = {k: float(np.linalg.norm(v)) for k, v in up.items()}
    print(name, "face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh), "upstream norms", parts)
    assert np.linalg.norm(gh) > 0 and all(v > 0 for v in parts.values()) and err <= RS.CHAIN, err


@pytest.mark.parametrize("wname", WRAP_NAMES)
def test_pass_through_lanes_on_the_device(hf, wname):
    """the hand-placed lanes of tests/test_bumpmap_ref.py: exact copies, the identity gradient, and no texel touched"""
    tex, uv, b, ng, u, v, active, names = pass_through_lanes()
    n = len(names)
    wv = _Wave(hf, uv, b, ng, u, v, active, tex, wname, 1.0)
    x = R.inputs(n, tex.shape)
    every = np.ones(n, bool)
    got = wv.evaluate(x, every)
    assert got["mask"].tolist() == [True] + [False] * (n - 1), dict(zip(names, got["mask"]))
    assert np.array_equal(got["N"][:, 1:].view(np.uint32), b[:, 1:].view(np.uint32))         # bit for bit, the NaN lane too
    assert not np.array_equal(got["N"][:, 0], b[:, 0])
    assert np.array_equal(got["dN"][:, 1:], x.db[:, 1:]) and np.array_equal(got["grad_sh_n"][:, 1:], x.gout[:, 1:])
    assert not got["grad_uv"][:, 1:].any() and not got["grad_dp_du"][:, 1:].any() and not got["grad_dp_dv"][:, 1:].any()
    a = (tex, uv, b, ng, u, v, active, R.WRAPS[wname], 1.0, x, every)
    r64, r32 = R.evaluate(*a), R.evaluate(*a, dtype=np.float32)
    # (these inputs are not the table's: four times the float32 restatement's own error, and at least half an ulp at 1)
    assert np.abs(got["N"][:, 0] - r64["N"][:, 0]).max() <= max(4 * np.abs(r32["N"][:, 0] - r64["N"][:, 0]).max(), ULP)
    # the pass-through lanes alone: no texel is touched
    rest = _Wave(hf, uv[:, 1:], b[:, 1:], ng[:, 1:], u[:, 1:], v[:, 1:], active[1:], tex, wname, 1.0)
    gtex = torch.zeros_like(rest.tex)
    gn, gnp = guarded(n - 1, 8, 3)
    rest.adjoint(_cu(x.gout[:, 1:]), gtex, None, gnp, None, None)
    torch.cuda.synchronize()
    assert not bool(gtex.any()) and intact(gn, n - 1, 8)


SIZES = [1, 63, 65, 257, 3 * 151]


@pytest.mark.parametrize("n", SIZES)
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, n):
    """a window of n samples of the `affine` scene with guard values around every output row, every optional pointer NULL
    in turn; a lane's arithmetic does not depend on its neighbours, so every per-lane output is bitwise the slice of the
    whole wavefront's"""
    sc = _scene(hf, oracle, "affine", True)
    TW, TH = R.TEXTURES[0]
    scale = R.SCALES[1]
    tol = R.TOL[R.table_key(TW, TH, scale)]["grad_tex"]
    G, lo = 96, 512
    keep_all = sc.keep[(TW, TH, "repeat", scale)]
    x_all = R.inputs(sc.n, (TH, TW))
    full = _scene_wave(hf, sc, TW, TH, "repeat", scale).evaluate(x_all, keep_all)
    wv = _scene_wave(hf, sc, TW, TH, "repeat", scale, lo, lo + n)
    x = R.types.SimpleNamespace(**{k: (v if k == "dtex" else v[:, lo:lo + n]) for k, v in vars(x_all).items()})
    keep = keep_all[lo:lo + n]
    dev = {k: _cu(np.ascontiguousarray(v, np.float32)) for k, v in (("dtex", x.dtex), ("duv", x.duv * keep), ("db", x.db * keep),
                                                                    ("ddu", x.ddu * keep), ("ddv", x.ddv * keep), ("gout", x.gout * keep))}
    sl = lambda k: full[k][..., lo:lo + n]
    cut = lambda buf: _np(buf[:, G:G + n])
    hit = sc.hit[lo:lo + n]

    def forward(mask=True, active=True):
        out, op = guarded(n, G, 3)
        m = torch.full((n + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        wv.forward(op, m.data_ptr() + G if mask else None, active)
        assert intact(out, n, G) and bool((m[:G] == 0x5A).all()) and bool((m[G + n:] == 0x5A).all())
        return out, m
    out, m = forward()
    assert np.array_equal(cut(out), sl("N")) and np.array_equal(_np(m[G:G + n]).astype(bool), sl("mask"))
    out2, m2 = forward(mask=False)
    assert torch.equal(out2, out) and bool((m2 == 0x5A).all())                                   # untouched
    out3, m3 = forward(active=False)                          # active NULL: every lane, the misses among them
    assert np.array_equal(cut(out3)[:, hit], sl("N")[:, hit]) and np.array_equal(_np(m3[G:G + n]).astype(bool)[hit], sl("mask")[hit])

    def tangent(use):
        o, op = guarded(n, G, 3)
        q = lambda k: dev[k] if k in use else None
        wv.tangent(op, q("dtex"), q("duv"), q("db"), q("ddu"), q("ddv"))
        assert intact(o, n, G)
        return o
    names = ("dtex", "duv", "db", "ddu", "ddv")
    dN = tangent(names)
    assert np.array_equal(cut(dN), sl("dN")) and torch.equal(tangent(names), dN)                 # bitwise repeatable
    assert not bool(tangent(())[:, G:G + n].any())
    parts = [cut(tangent((k,))).astype(np.float64) for k in names]
    # every part and the whole are float32 roundings of exact sums: six half ulps of the largest term, generously 2^-21
    assert np.abs(sum(parts) - cut(dN)).max() <= 2.0 ** -21 * max(1.0, max(np.abs(p).max() for p in parts))

    def adjoint(skip=None):
        o = {"gtex": torch.zeros_like(wv.tex)}
        ptr = {}
        for k, r in (("guv", 2), ("gn", 3), ("gpu", 3), ("gpv", 3)):
            o[k], ptr[k] = guarded(n, G, r)
        a = lambda k: None if skip == k else (o[k] if k == "gtex" else ptr[k])
        wv.adjoint(dev["gout"], a("gtex"), a("guv"), a("gn"), a("gpu"), a("gpv"))
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("guv", "gn", "gpu", "gpv"))
    for k, name in (("guv", "grad_uv"), ("gn", "grad_sh_n"), ("gpu", "grad_dp_du"), ("gpv", "grad_dp_dv")):
        assert np.array_equal(cut(fulla[k]), sl(name)), k
    assert torch.equal(adjoint()["guv"], fulla["guv"]) and torch.equal(adjoint()["gn"], fulla["gn"])   # bitwise repeatable
    gt = _np(fulla["gtex"]).astype(np.float64)
    for skip in ("gtex", "guv", "gn", "gpu", "gpv"):
        part = adjoint(skip)
        for k in part:
            if k == skip:
                assert not bool(part[k].any()) if k == "gtex" else bool((part[k] == GUARD).all())   # untouched
            elif k == "gtex":
                assert not (hit & keep).any() or R.err_l2(_np(part[k]), gt) <= tol                  # (float atomics)
            else:
                assert torch.equal(part[k], fulla[k]), (skip, k)
    # the texels' gradient of the window against the reverse sweep on the window's records
    if (hit & keep).sum() >= 32:
        w = slice(lo, lo + n)
        ref = R.adjoint(R.texture(TW, TH), sc.rec["uv"][:, w], sc.rec["sh_n"][:, w], sc.rec["n"][:, w], sc.rec["dp_du"][:, w],
                        sc.rec["dp_dv"][:, w], hit, R.REPEAT, scale, x.gout * keep)
        assert R.err_l2(gt, ref.gtex) <= tol
    torch.cuda.synchronize()


def _table_row(TW, TH, scale):
    """the table's row a texture is held to: its own, or -- the figures grow with TW and TH -- the smaller texture's"""
    return R.F32[R.table_key(*((37, 29) if (TW, TH) == (37, 29) else (16, 8)), scale)]


@pytest.mark.parametrize("TW,TH", [(1, 1), (1, 5), (2, 2), (37, 29)])
@pytest.mark.parametrize("wname", WRAP_NAMES)
def test_small_textures_and_uv_outside_the_unit_square(hf, oracle, TW, TH, wname):
    """the records of the `mirror_flip` scene with uv stretched to [-1, 2]^2, where the wrap decides what is read: N against
    the frame algebra on the slopes of hf_bitmap_eval within one ulp, the mask bitwise, and everything against the
    restatement.  These inputs are not those of the table F32, so the allowance is four times the larger of that table and
    the float32 restatement's own error against float64 on these very inputs."""
    sc = _scene(hf, oracle, "mirror_flip", True)
    scale = R.SCALES[1]
    uv = (3.0 * sc.rec["uv"] - 1.0).astype(np.float32)
    uv[:, ~sc.hit] = 0
    tex = R.texture(TW, TH, seed=TW + TH)
    wrap = R.WRAPS[wname]
    rec = dict(sc.rec, uv=uv)
    wv = _Wave(hf, *R.record_args(rec), sc.active, tex, wname, scale)
    _, _, s = R.forward(tex, *R.record_args(rec), sc.hit, wrap, scale)
    sh = R.shares(s, sc.hit)
    outside = ((uv < 0) | (uv > 1)).any(0)[sc.hit].mean()
    print((TW, TH), wname, sh, "outside [0, 1]^2", outside)
    R.conditions(sh, UNSURE_CAP)
    assert outside > 0.5 and sh["sigma_negative"] > 0
    keep = ~R.near_edge(s)
    x = R.inputs(sc.n, tex.shape)
    got = wv.evaluate(x, keep)
    pos = torch.stack([wv.uv[0] * float(TW), wv.uv[1] * float(TH)]).contiguous()
    L, slopes = torch.zeros(sc.n, device="cuda"), torch.zeros((2, sc.n), device="cuda")
    wv.check(wv.lib.hf_bitmap_eval(sc.n, rows(pos), sc.active.data_ptr(), TW, TH, wv.tex.data_ptr(), wrap, L.data_ptr(), rows(slopes),
                                   torch.cuda.current_stream().cuda_stream))
    Lx, Ly = _np(slopes)
    alg = R.frame(Lx, Ly, np.ones(sc.n, bool), sc.rec["sh_n"], sc.rec["n"], sc.rec["dp_du"], sc.rec["dp_dv"], TW, TH, np.float32(scale),
                  sc.hit)
    assert np.array_equal(got["mask"], alg.pert) and np.abs(got["N"].astype(np.float64) - alg.N).max() <= ULP
    args = (tex, *R.record_args(rec), sc.hit, wrap, scale, x, keep)
    r64, r32 = R.evaluate(*args), R.evaluate(*args, dtype=np.float32)
    own = R.errors(r32, r64, keep)
    err = R.errors(got, r64, keep)
    table = _table_row(TW, TH, scale)
    print("error", {k: "%.3g" % v for k, v in err.items()}, "float32 restatement", {k: "%.3g" % v for k, v in own.items()})
    if (TW, TH) == (1, 1):
        # one texel: no slope, and the four weights of a lane cancel.  Every one of the 4 n float adds is rounded at the size
        # of the running sum, which is at most M = 2 sum(|q_x| + |q_y|): the residue is at most 4 n 2^-24 M, where a weight
        # of the wrong sign would leave a sum of the order of sqrt(n) |q|, some 20 times that
        assert not got["grad_uv"].any()
        q = np.abs(R.adjoint(*args[:-2], x.gout * keep).q).sum()
        assert np.abs(got["grad_tex"]).max() <= 4 * sc.n * 2.0 ** -24 * 2 * q, (np.abs(got["grad_tex"]).max(), q)
        err.pop("grad_tex")
    for k, v in err.items():
        assert v <= 4 * max(table[k], own[k]), (k, v, own[k])


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    """one captured graph of a single-stream forward + tangent + adjoint, replayed: the capture succeeds only if no call
    allocates or synchronises the host"""
    sc = _scene(hf, oracle, "affine", True)
    TW, TH = R.TEXTURES[0]
    scale = R.SCALES[0]
    wv = _scene_wave(hf, sc, TW, TH, "repeat", scale)
    x = R.inputs(sc.n, (TH, TW))
    z = lambda *s, dtype=torch.float32: torch.zeros(s, device="cuda", dtype=dtype)
    N, dN, mask = z(3, sc.n), z(3, sc.n), z(sc.n, dtype=torch.uint8)
    gtex, guv, gn, gpu, gpv = torch.zeros_like(wv.tex), z(2, sc.n), z(3, sc.n), z(3, sc.n), z(3, sc.n)
    t = [_cu(np.ascontiguousarray(a, np.float32)) for a in (x.dtex, x.duv, x.db, x.ddu, x.ddv, x.gout)]

    def launch():
        gtex.zero_()                                                     # (accumulated into)
        wv.forward(rows(N), mask.data_ptr())
        wv.tangent(rows(dN), *t[:5])
        wv.adjoint(t[5], gtex, rows(guv), rows(gn), rows(gpu), rows(gpv))
    outs = (N, dN, mask, guv, gn, gpu, gpv)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first, first_tex = [v.clone() for v in outs], gtex.clone()
    assert float(N.abs().sum()) > 0 and float(gtex.abs().sum()) > 0 and bool(mask.any())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for v in outs:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)
    assert R.err_l2(_np(gtex), _np(first_tex).astype(np.float64)) <= R.TOL[R.table_key(TW, TH, scale)]["grad_tex"]   # to rounding


def test_inverse_bumpmap_example_descends(hf):
    import inverse_bumpmap
    hist, err0, err = inverse_bumpmap.run(size=48, steps=40, verbose=False)
    print("loss", hist[0], "->", hist[-1], "relief error", err0, "->", err)
    assert np.isfinite(hist[-1]) and hist[-1] < hist[0], (hist[0], hist[-1])

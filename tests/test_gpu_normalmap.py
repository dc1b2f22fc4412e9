"""The normal map on the GPU (hf_normalmap_eval, _tangent, _adjoint; hf_amd.NormalMap) on the scenes of
tests/row_scenes.py (CASES, the view `steep`: 25 x 23 x 4 wavefronts under to_world, flip_normals and a view from below,
flat and smooth shading), with the textures of normalmap_ref.TEXTURES (37 x 29 and 16 x 8) under both wraps.
  (1) the lookup: with c taken from three Bitmap.eval calls on the planes at pos, the fused N equals the float64
      restatement of the frame algebra within one float32 ulp at 1 (2^-23 absolute), the mask bitwise;
  (2) N, dN, grad_uv, grad_sh_n, grad_dp_du per component and grad_tex as a relative L2 against the restatement;
  (3) the transposition on the device through backward and jvp with all four inputs attached; the forward and the tangent
      bitwise repeatable, grad_tex to rounding;
  (4) the flat map: perturb returns sh_frame.n bit for bit, and directional_lighting of the perturbed interaction the
      bits it returns without a map;
  (5) the chain ray_intersect -> NormalMap.normal -> directional_lighting -> sum -> dL/dheight, flat and smooth shading;
  (6) the hand-placed pass-through lanes of tests/test_normalmap_ref.py: exact copies, identity gradient, no texel touched;
  (7) n = 0, 1, 63, 65, 257 and 3 * 151 with guard bands, every optional pointer NULL in turn, textures 1 x 1, 1 x 5,
      2 x 2 and 37 x 29, uv outside [0, 1] under both wraps;
  (8) -- none of the three kernels is grid-stride (one lane per sample, a grid of ceil(n / 256) blocks): HF_FORCE_GRID
      does not reach them, and there is no loop to take beyond its first iteration;
  (9) a captured graph of forward, tangent and adjoint replays to the same bits, grad_tex to rounding;
  (10) examples/inverse_normalmap.py descends.

Tolerances (scripts/normalmap_f32_error.py computes them on the CPU, profiles/normalmap/f32_error.json): the
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records, by at
most the figures of normalmap_ref.F32 (per component as the largest difference over max(1, the largest value); grad_tex
as a relative L2).  The GPU is allowed four times that (normalmap_ref.TOL): it differs from the float32 restatement only
in where it rounds, and it rounds later.  Samples whose position in the cell is within normalmap_ref.MARGIN of a cell
edge are left out of grad_uv and get a zero duv, at most row_helpers.UNSURE_CAP of the hits; asserted, with the distance
from the pass-through thresholds, on the GPU's own records before anything is compared."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import directional_ref as D
import normalmap_ref as R
import row_scenes as RS
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, guarded, intact, rows
from test_normalmap_ref import pass_through_lanes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ULP = 2.0 ** -23
WRAP_NAMES = ("clamp", "repeat")
_SCENES = {}


def _scene(hf, oracle, name, face_normals):
    """a scene of row_scenes on the device, once, with the records the map reads as numpy and the asserted shares"""
    key = (name, face_normals)
    if key not in _SCENES:
        sc = RS.device_scene(hf, oracle, name, "steep", face_normals)
        sc.rec = {"uv": _np(sc.si.uv), "sh_n": _np(sc.si.sh_frame.n), "dp_du": _np(sc.si.dp_du), "hit": sc.hit}
        sc.active = _cu(sc.hit.astype(np.uint8))
        sc.keep = {}
        for TW, TH in R.TEXTURES:
            for wname in WRAP_NAMES:
                _, _, s = R.forward(R.texture(TW, TH), sc.rec["uv"], sc.rec["sh_n"], sc.rec["dp_du"], sc.hit, R.WRAPS[wname])
                sh = R.shares(s, sc.hit)
                print(name, face_normals, (TW, TH), wname, sh)
                # (asserted before anything is compared)
                assert sh["near_edge"] <= UNSURE_CAP and sh["near_threshold"] == 0 and sh["perturbed_of_hits"] == 1.0, sh
                sc.keep[(TW, TH, wname)] = ~R.near_edge(s)
        _SCENES[key] = sc
    return _SCENES[key]


class _Wave:
    """device rows of a wavefront, a texture and a wrap, and the three C calls on them"""

    def __init__(self, hf, uv, sh_n, dp_du, active, tex, wname):
        f = lambda x: (x if isinstance(x, torch.Tensor) else _cu(np.asarray(x, np.float32))).detach().contiguous()
        self.uv, self.sn, self.du, self.tex = f(uv), f(sh_n), f(dp_du), f(tex)
        self.active = None if active is None else (active if isinstance(active, torch.Tensor) else _cu(np.asarray(active, np.uint8)))
        self.n, self.wrap = self.uv.shape[1], R.WRAPS[wname]
        self.lib, self.check = hf._capi.lib(), hf._capi.check

    def head(self, active=True):
        act = self.active.data_ptr() if (active and self.active is not None) else None
        return (self.n, rows(self.uv), rows(self.sn), rows(self.du), act, self.tex.shape[2], self.tex.shape[1], self.tex.data_ptr(),
                self.wrap)

    def forward(self, out, mask=None, active=True):
        self.check(self.lib.hf_normalmap_eval(*self.head(active), out, mask, torch.cuda.current_stream().cuda_stream))

    def tangent(self, out, dtex=None, duv=None, dn=None, dp=None):
        q = lambda x: None if x is None else rows(x)
        self.check(self.lib.hf_normalmap_eval_tangent(*self.head(), None if dtex is None else dtex.data_ptr(), q(duv), q(dn), q(dp),
                                                      out, torch.cuda.current_stream().cuda_stream))

    def adjoint(self, gout, gtex=None, guv=None, gn=None, gp=None):
        self.check(self.lib.hf_normalmap_eval_adjoint(*self.head(), rows(gout), None if gtex is None else gtex.data_ptr(), guv, gn, gp,
                                                      torch.cuda.current_stream().cuda_stream))

    def evaluate(self, x, keep):
        """forward, tangent and adjoint under the inputs x: the dict of normalmap_ref.evaluate, as numpy"""
        z = lambda *s: torch.zeros(s, device="cuda")
        N, dN, mask = z(3, self.n), z(3, self.n), torch.zeros(self.n, dtype=torch.uint8, device="cuda")
        gtex, guv, gn, gp = torch.zeros_like(self.tex), z(2, self.n), z(3, self.n), z(3, self.n)
        t = [_cu(np.ascontiguousarray(a, np.float32)) for a in (x.dtex, x.duv * keep, x.db, x.ddp, x.gout)]
        if self.n:
            self.forward(rows(N), mask.data_ptr())
            self.tangent(rows(dN), *t[:4])
            self.adjoint(t[4], gtex, rows(guv), rows(gn), rows(gp))
        torch.cuda.synchronize()
        return {"N": _np(N), "mask": _np(mask).astype(bool), "dN": _np(dN), "grad_uv": _np(guv), "grad_sh_n": _np(gn),
                "grad_dp_du": _np(gp), "grad_tex": _np(gtex)}


def _scene_wave(hf, sc, TW, TH, wname, lo=0, hi=None, seed=0):
    hi = sc.n if hi is None else hi
    cut = lambda v: v.detach()[..., lo:hi].contiguous()
    return _Wave(hf, cut(sc.si.uv), cut(sc.si.sh_frame.n), cut(sc.si.dp_du), cut(sc.active), R.texture(TW, TH, seed), wname)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_fused_normal_is_the_frame_algebra_on_three_bitmap_lookups_within_one_ulp(hf, oracle, name, face_normals):
    sc = _scene(hf, oracle, name, face_normals)
    for TW, TH in R.TEXTURES:
        tex = _cu(R.texture(TW, TH))
        for wname in WRAP_NAMES:
            nm = hf.NormalMap(tex, wrap=wname)
            N, mask = nm.normal(sc.si, active=sc.active, return_mask=True)
            # pos as the kernel forms it: one float32 product per coordinate
            pos = torch.stack([sc.si.uv[0].detach() * float(TW), sc.si.uv[1].detach() * float(TH)])
            c = np.stack([_np(hf.Bitmap(tex[k], wrap=wname).eval(pos, active=sc.active)) for k in range(3)])
            s = R.shade(c, np.isfinite(sc.rec["uv"]).all(0), sc.rec["sh_n"], sc.rec["dp_du"], sc.hit)
            assert np.array_equal(_np(mask).astype(bool), s.pert) and s.pert[sc.hit].all() and not s.pert[~sc.hit].any()
            err = np.abs(_np(N).astype(np.float64) - s.N).max()
            print(name, face_normals, (TW, TH), wname, "largest |N - restatement|", err, "in ulps at 1:", err / ULP)
            assert err <= ULP, err
            assert np.array_equal(_np(N)[:, ~sc.hit].view(np.uint32), sc.rec["sh_n"][:, ~sc.hit].view(np.uint32))   # a copy
            cosine = (s.N * sc.rec["sh_n"]).sum(0)[sc.hit]
            assert np.median(cosine) < 0.98                                       # (the map does something)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_values_gradients_and_tangents_against_the_restatement(hf, oracle, name, face_normals):
    sc = _scene(hf, oracle, name, face_normals)
    worst = {k: 0.0 for k in R.TOL}
    for TW, TH in R.TEXTURES:
        tex = R.texture(TW, TH)
        x = R.inputs(sc.n, tex.shape)
        for wname in WRAP_NAMES:
            keep = sc.keep[(TW, TH, wname)]
            wv = _scene_wave(hf, sc, TW, TH, wname)
            got = wv.evaluate(x, keep)
            ref = R.evaluate(tex, sc.rec["uv"], sc.rec["sh_n"], sc.rec["dp_du"], sc.hit, R.WRAPS[wname], x, keep)
            assert np.array_equal(got["mask"], ref["mask"])
            miss = ~sc.hit
            assert not got["grad_uv"][:, miss].any() and not got["grad_dp_du"][:, miss].any()       # exact zeros
            assert np.array_equal(got["grad_sh_n"][:, miss], x.gout[:, miss]) and np.array_equal(got["dN"][:, miss], x.db[:, miss])
            for k in ("dN", "grad_uv", "grad_sh_n", "grad_dp_du", "grad_tex"):
                assert np.abs(ref[k]).max() > 1e-3, k
            err = R.errors(got, ref, keep)
            print(name, face_normals, (TW, TH), wname, "left out", int((~keep & sc.hit).sum()), {k: "%.3g" % v for k, v in err.items()})
            for k, v in err.items():
                worst[k] = max(worst[k], v)
    print("worst", {k: "%.3g / %.3g" % (worst[k], R.TOL[k]) for k in R.TOL})
    for k in R.TOL:
        assert worst[k] <= R.TOL[k], (k, worst[k], R.TOL[k])


def _leaf_si(hf, sc, uv, sh_n, dp_du):
    si = hf.SurfaceInteraction3f()
    si.uv, si.dp_du, si.sh_frame = uv, dp_du, hf.Frame3f(None, None, sh_n)
    si.p, si.n, si.t = sc.si.p.detach(), sc.si.n.detach(), sc.si.t.detach()
    return si


def test_transposition_on_the_device_through_backward_and_jvp_and_repeatability(hf, oracle):
    """<J u, v> = <u, J^T v> through the public class with the texels, uv, sh_n and dp_du attached: forward_ad against
    backward, both sides float32 results added up in float64.  Each side is within its tolerance of the exact bilinear form,
    so by Cauchy-Schwarz the gap is at most the sum over the quantities of (tolerance x the quantity's scale x the root of
    its size x the L2 norm of what it is paired with); grad_tex, held as a relative L2, enters with its own norm."""
    sc = _scene(hf, oracle, "affine", False)
    TW, TH = R.TEXTURES[0]
    tex = R.texture(TW, TH)
    x = R.inputs(sc.n, tex.shape)
    leaves = lambda: [v.detach().clone().requires_grad_(True) for v in (_cu(tex), sc.si.uv, sc.si.sh_frame.n, sc.si.dp_du)]
    runs = []
    for _ in range(2):
        data, uv, sn, du = leaves()
        nm = hf.NormalMap(data, wrap="repeat")
        N, mask = nm.normal(_leaf_si(hf, sc, uv, sn, du), active=sc.active, return_mask=True)
        (N * _cu(x.gout)).sum().backward()
        with fwAD.dual_level():
            dual = [fwAD.make_dual(v.detach(), _cu(t)) for v, t in zip((data, uv, sn, du), (x.dtex, x.duv, x.db, x.ddp))]
            dN = fwAD.unpack_dual(hf.NormalMap(dual[0], wrap="repeat").normal(_leaf_si(hf, sc, *dual[1:]), active=sc.active)).tangent.clone()
        runs.append((N.detach().clone(), mask.clone(), dN, uv.grad.clone(), sn.grad.clone(), du.grad.clone(), data.grad.clone()))
    for a, b in zip(runs[0][:6], runs[1][:6]):
        assert torch.equal(a, b)                                                  # bitwise
    N, mask, dN, guv, gn, gp, gtex = (_np(a) for a in runs[0])
    again = R.err_l2(_np(runs[1][6]), gtex.astype(np.float64))
    print("grad_tex run to run, relative L2", again)
    assert again <= R.TOL["grad_tex"]                                              # float atomics: the order is free
    gap = abs((dN.astype(np.float64) * x.gout).sum() - sum((g.astype(np.float64) * t).sum() for g, t in
                                                          ((gtex, x.dtex), (guv, x.duv), (gn, x.db), (gp, x.ddp))))
    norm = np.linalg.norm
    scale = lambda a: max(1.0, float(np.abs(a).max()))
    bound = R.TOL["dN"] * scale(dN) * np.sqrt(dN.size) * norm(x.gout) + R.TOL["grad_tex"] * norm(gtex) * norm(x.dtex)
    for k, g, t in (("grad_uv", guv, x.duv), ("grad_sh_n", gn, x.db), ("grad_dp_du", gp, x.ddp)):
        bound += R.TOL[k] * scale(g) * np.sqrt(g.size) * norm(t)
    print("transposition gap", gap, "bound", bound, "<J u, v>", (dN.astype(np.float64) * x.gout).sum())
    assert norm(dN) > 0 and gap <= bound, (gap, bound)


def _rig(hf, sc):
    _, lights = RS.rig("directional", sc)
    return lights, [hf.DirectionalLight(L.to_light, L.irradiance) for L in lights]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_flat_map_changes_no_bit(hf, oracle, name, face_normals):
    sc = _scene(hf, oracle, name, face_normals)
    _, lights = _rig(hf, sc)
    bits = lambda v: v.detach().contiguous().view(torch.int32)
    base = hf.directional_lighting(sc.shape, sc.si, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP, return_value=True, return_visibility=True)
    for wname in WRAP_NAMES:
        for TW, TH in ((37, 29), (1, 1)):
            nm = hf.NormalMap.flat(TW, TH, device="cuda", wrap=wname)
            si = nm.perturb(sc.si)
            assert si is not sc.si and si.p is sc.si.p
            assert torch.equal(bits(si.sh_frame.n), bits(sc.si.sh_frame.n))
            _, mask = nm.normal(sc.si, return_mask=True)
            assert bool(mask[sc.active.bool()].all())                             # (perturbed lanes, not copies)
            lit = hf.directional_lighting(sc.shape, si, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP, return_value=True, return_visibility=True)
            for a, b in zip(base, lit):
                assert torch.equal(a, b)
    assert float(base[0].abs().sum()) > 0


@pytest.mark.parametrize("name,face_normals", RS.CHAINS)
def test_chain_to_the_heights(hf, oracle, name, face_normals):
    """ray_intersect -> NormalMap.normal -> directional_lighting -> loss -> backward() -> shape.heightfield.grad against the
    restatements' gradients (directional_ref.adjoint for dL/dN, normalmap_ref.adjoint for dL/d(uv, sh_n, dp_du), fed with the
    GPU's records and visibility), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Measure and bound:
    tests/test_gpu_directional.py::test_chain_to_the_heights' (row_scenes.CHAIN)."""
    sc = _scene(hf, oracle, name, face_normals)
    ref_lights, lights = _rig(hf, sc)
    K = len(lights)
    TW, TH = R.TEXTURES[0]
    tex = R.texture(TW, TH)
    x = D.inputs(sc.n, RS.SPP, K)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    nm = hf.NormalMap(_cu(tex), wrap="repeat")
    lit = nm.perturb(si, active=sc.active)
    N = _np(lit.sh_frame.n)
    img, vis = hf.directional_lighting(shape, lit, sc.ray, lights, albedo=D.ALBEDO, spp=RS.SPP, return_visibility=True)
    vis = D.unpack(_np(vis), K)
    # samples on which rounding may decide a mask of the lighting row are left out of the loss, as that row's tests do
    unsure = np.zeros(sc.n, bool)
    for L in ref_lights:
        unsure |= D.traced(L, N, sc.np["d"], sc.np["t"])[1]
    assert unsure.mean() <= UNSURE_CAP, unsure.mean()
    gi = np.where(~unsure.reshape(-1, RS.SPP).any(1)[None], x.gi, 0).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    gN = D.adjoint(ref_lights, N, None, D.ALBEDO, vis, RS.SPP, gi).gn
    g = R.adjoint(tex, _np(si.uv), _np(si.sh_frame.n), _np(si.dp_du), sc.hit, R.REPEAT, gN)
    up = {"uv": g.guv.astype(np.float32), "sh_n": g.gn.astype(np.float32), "dp_du": g.gp.astype(np.float32)}
    if face_normals:
        t, u, v, prim = sc.pi_oracle
        gh = sc.field.adjoint(sc.rays, t, u, v, prim, up, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[7:9], ybar[9:12], ybar[12:15] = _cu(up["uv"]), _cu(up["sh_n"]), _cu(up["dp_du"])
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    parts = {k: float(np.linalg.norm(v)) for k, v in up.items()}
    print(name, "face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh), "upstream norms", parts)
    assert np.linalg.norm(gh) > 0 and all(v > 0 for v in parts.values()) and err <= RS.CHAIN, err


@pytest.mark.parametrize("wname", WRAP_NAMES)
def test_pass_through_lanes_on_the_device(hf, wname):
    """the hand-placed lanes of tests/test_normalmap_ref.py: exact copies, the identity gradient, and no texel touched"""
    tex, uv, b, u, active, names = pass_through_lanes()
    n = len(names)
    wv = _Wave(hf, uv, b, u, active, tex, wname)
    x = R.inputs(n, tex.shape)
    got = wv.evaluate(x, np.ones(n, bool))
    assert got["mask"].tolist() == [True] + [False] * (n - 1), dict(zip(names, got["mask"]))
    assert np.array_equal(got["N"][:, 1:].view(np.uint32), b[:, 1:].view(np.uint32))         # bit for bit, the NaN lane too
    assert not np.array_equal(got["N"][:, 0], b[:, 0])
    assert np.array_equal(got["dN"][:, 1:], x.db[:, 1:]) and np.array_equal(got["grad_sh_n"][:, 1:], x.gout[:, 1:])
    assert not got["grad_uv"][:, 1:].any() and not got["grad_dp_du"][:, 1:].any()
    ref = R.evaluate(tex, uv, b, u, active, R.WRAPS[wname], x, np.ones(n, bool))
    assert np.abs(got["N"][:, 0] - ref["N"][:, 0]).max() <= R.TOL["N"]
    # the pass-through lanes alone: no texel is touched
    rest = _Wave(hf, uv[:, 1:], b[:, 1:], u[:, 1:], active[1:], tex, wname)
    gtex = torch.zeros_like(rest.tex)
    gn, gnp = guarded(n - 1, 8, 3)
    rest.adjoint(_cu(x.gout[:, 1:]), gtex, None, gnp, None)
    torch.cuda.synchronize()
    assert not bool(gtex.any()) and intact(gn, n - 1, 8)


SIZES = [0, 1, 63, 65, 257, 3 * 151]


@pytest.mark.parametrize("n", SIZES)
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, n):
    """a window of n samples of the `affine` scene with guard values around every output row, every optional pointer NULL
    in turn; a lane's arithmetic does not depend on its neighbours, so every per-lane output is bitwise the slice of the
    whole wavefront's"""
    sc = _scene(hf, oracle, "affine", True)
    TW, TH = R.TEXTURES[0]
    G, lo = 96, 512
    keep_all = sc.keep[(TW, TH, "repeat")]
    whole = _scene_wave(hf, sc, TW, TH, "repeat")
    x_all = R.inputs(sc.n, (3, TH, TW))
    full = whole.evaluate(x_all, keep_all)
    wv = _scene_wave(hf, sc, TW, TH, "repeat", lo, lo + n)
    x = R.types.SimpleNamespace(**{k: (v if k == "dtex" else v[:, lo:lo + n]) for k, v in vars(x_all).items()})
    keep = keep_all[lo:lo + n]
    dev = {k: _cu(np.ascontiguousarray(v, np.float32)) for k, v in (("dtex", x.dtex), ("duv", x.duv * keep), ("db", x.db), ("ddp", x.ddp),
                                                                    ("gout", x.gout))}
    if n == 0:
        # (the C entries with n = 0 are tests/test_normalmap_abi.py's: an empty tensor has no rows to point to; the Python
        # class launches nothing and hands back empty rows, in both directions)
        empty = torch.zeros((3, 0), device="cuda")
        si = hf.SurfaceInteraction3f()
        si.uv, si.dp_du, si.sh_frame = torch.zeros((2, 0), device="cuda"), empty, hf.Frame3f(None, None, empty.clone().requires_grad_(True))
        out, mask = hf.NormalMap(wv.tex.clone().requires_grad_(True)).normal(si, return_mask=True)
        assert out.shape == (3, 0) and mask.shape == (0,)
        out.sum().backward()
        return
    sl = lambda k: full[k][..., lo:lo + n]
    cut = lambda buf: _np(buf[:, G:G + n])

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
    hit = sc.hit[lo:lo + n]
    assert np.array_equal(cut(out3)[:, hit], sl("N")[:, hit]) and np.array_equal(_np(m3[G:G + n]).astype(bool)[hit], sl("mask")[hit])

    def tangent(use):
        o, op = guarded(n, G, 3)
        q = lambda k: dev[k] if k in use else None
        wv.tangent(op, q("dtex"), q("duv"), q("db"), q("ddp"))
        assert intact(o, n, G)
        return o
    names = ("dtex", "duv", "db", "ddp")
    dN = tangent(names)
    assert np.array_equal(cut(dN), sl("dN")) and torch.equal(tangent(names), dN)                 # bitwise repeatable
    assert not bool(tangent(())[:, G:G + n].any())
    parts = [cut(tangent((k,))).astype(np.float64) for k in names]
    # every part and the whole are float32 roundings of exact sums: five half ulps of the largest term, generously 2^-21
    assert np.abs(sum(parts) - cut(dN)).max() <= 2.0 ** -21 * max(1.0, max(np.abs(p).max() for p in parts))

    def adjoint(skip=None):
        o = {"gtex": torch.zeros_like(wv.tex)}
        ptr = {}
        for k, r in (("guv", 2), ("gn", 3), ("gp", 3)):
            o[k], ptr[k] = guarded(n, G, r)
        a = lambda k: None if skip == k else (o[k] if k == "gtex" else ptr[k])
        wv.adjoint(dev["gout"], a("gtex"), a("guv"), a("gn"), a("gp"))
        return o
    fulla = adjoint()
    assert all(intact(fulla[k], n, G) for k in ("guv", "gn", "gp"))
    for k, name in (("guv", "grad_uv"), ("gn", "grad_sh_n"), ("gp", "grad_dp_du")):
        assert np.array_equal(cut(fulla[k]), sl(name)), k
    gt = _np(fulla["gtex"]).astype(np.float64)
    for skip in ("gtex", "guv", "gn", "gp"):
        part = adjoint(skip)
        for k in part:
            if k == skip:
                assert not bool(part[k].any()) if k == "gtex" else bool((part[k] == GUARD).all())   # untouched
            elif k == "gtex":
                assert not hit.any() or R.err_l2(_np(part[k]), gt) <= R.TOL["grad_tex"]              # (float atomics)
            else:
                assert torch.equal(part[k], fulla[k]), (skip, k)
    # the texels' gradient of the window against the reverse sweep on the window's records
    if hit.sum() >= 32:
        ref = R.adjoint(R.texture(TW, TH), sc.rec["uv"][:, lo:lo + n], sc.rec["sh_n"][:, lo:lo + n], sc.rec["dp_du"][:, lo:lo + n], hit,
                        R.REPEAT, x.gout)
        assert R.err_l2(gt, ref.gtex) <= R.TOL["grad_tex"]
    torch.cuda.synchronize()


@pytest.mark.parametrize("TW,TH", [(1, 1), (1, 5), (2, 2), (37, 29)])
@pytest.mark.parametrize("wname", WRAP_NAMES)
def test_small_textures_and_uv_outside_the_unit_square(hf, oracle, TW, TH, wname):
    """the records of the `mirror_flip` scene with uv stretched to [-1, 2]^2, where the wrap decides what is read: N against
    the frame algebra on three Bitmap.eval lookups within one ulp (exact for every input), the mask bitwise, and the
    derivatives against the restatement.  These inputs are not those of the table F32, so the allowance is four times the
    larger of that table and the float32 restatement's own error against float64 on these very inputs."""
    sc = _scene(hf, oracle, "mirror_flip", True)
    uv = (3.0 * sc.rec["uv"] - 1.0).astype(np.float32)
    uv[:, ~sc.hit] = 0
    tex = R.texture(TW, TH, seed=TW + TH)
    wrap = R.WRAPS[wname]
    wv = _Wave(hf, uv, sc.rec["sh_n"], sc.rec["dp_du"], sc.active, tex, wname)
    _, _, s = R.forward(tex, uv, sc.rec["sh_n"], sc.rec["dp_du"], sc.hit, wrap)
    sh = R.shares(s, sc.hit)
    outside = ((uv < 0) | (uv > 1)).any(0)[sc.hit].mean()
    print((TW, TH), wname, sh, "outside [0, 1]^2", outside)
    assert sh["near_edge"] <= UNSURE_CAP and sh["near_threshold"] == 0 and sh["perturbed_of_hits"] == 1.0 and outside > 0.5
    keep = ~R.near_edge(s)
    x = R.inputs(sc.n, tex.shape)
    got = wv.evaluate(x, keep)
    tt, ut = _cu(tex), _cu(uv)
    pos = torch.stack([ut[0] * float(TW), ut[1] * float(TH)])
    c = np.stack([_np(hf.Bitmap(tt[k], wrap=wname).eval(pos, active=sc.active)) for k in range(3)])
    alg = R.shade(c, np.ones(sc.n, bool), sc.rec["sh_n"], sc.rec["dp_du"], sc.hit)
    assert np.array_equal(got["mask"], alg.pert) and np.abs(got["N"].astype(np.float64) - alg.N).max() <= ULP
    args = (tex, uv, sc.rec["sh_n"], sc.rec["dp_du"], sc.hit, wrap, x, keep)
    r64, r32 = R.evaluate(*args), R.evaluate(*args, dtype=np.float32)
    own = R.errors(r32, r64, keep)
    err = R.errors(got, r64, keep)
    print("error", {k: "%.3g" % v for k, v in err.items()}, "float32 restatement", {k: "%.3g" % v for k, v in own.items()})
    for k, v in err.items():
        assert v <= 4 * max(R.F32[k], own[k]), (k, v, own[k])
    if (TW, TH) == (1, 1):
        assert not got["grad_uv"].any()                                           # one texel: no slope


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    """one captured graph of a single-stream forward + tangent + adjoint, replayed: the capture succeeds only if no call
    allocates or synchronises the host"""
    sc = _scene(hf, oracle, "affine", True)
    TW, TH = R.TEXTURES[0]
    wv = _scene_wave(hf, sc, TW, TH, "repeat")
    x = R.inputs(sc.n, (3, TH, TW))
    z = lambda *s, dtype=torch.float32: torch.zeros(s, device="cuda", dtype=dtype)
    N, dN, mask = z(3, sc.n), z(3, sc.n), z(sc.n, dtype=torch.uint8)
    gtex, guv, gn, gp = torch.zeros_like(wv.tex), z(2, sc.n), z(3, sc.n), z(3, sc.n)
    t = [_cu(np.ascontiguousarray(a, np.float32)) for a in (x.dtex, x.duv, x.db, x.ddp, x.gout)]

    def launch():
        gtex.zero_()                                                     # (accumulated into)
        wv.forward(rows(N), mask.data_ptr())
        wv.tangent(rows(dN), *t[:4])
        wv.adjoint(t[4], gtex, rows(guv), rows(gn), rows(gp))
    outs = (N, dN, mask, guv, gn, gp)
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
    assert R.err_l2(_np(gtex), _np(first_tex).astype(np.float64)) <= R.TOL["grad_tex"]   # float atomics: to rounding


def test_inverse_normalmap_example_descends(hf):
    import inverse_normalmap
    hist, err0, err = inverse_normalmap.run(size=48, steps=40, verbose=False)
    print("loss", hist[0], "->", hist[-1], "mean angle", err0, "->", err)
    assert np.isfinite(hist[-1]) and hist[-1] < hist[0], (hist[0], hist[-1])
    assert err < err0, (err0, err)

"""Area-light lighting on the GPU (hf_rect_rays, hf_rect_lighting, _adjoint, _tangent) on row_helpers.base_scene:
sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from (1.2, 0.3, 1.2) and from (0.6, 0.35, 2.0),
both face_normals modes, the two lamps of tests/rect_ref.py (one above the terrain, one beside it), num_rays 1, 8, 32.
  (1) vis_bits against the two-call sequence hf_rect_rays + hf_ray_test bit for bit, the masks and the rays against the
      restatement, and both outcomes of a shadow ray and a penumbra present;
  (2) image, per-sample values, grad_sh_n, grad_p, grad_weight, grad_tex and the tangent image against the restatement fed
      with the GPU's bits, with and without a 16 x 8 texture; the transposition gap on the device;
  (3) the chain rect_lighting -> loss -> backward -> dL/dheight;
  (4) n = 0, an all-miss wavefront, odd sizes with guard bands, every optional pointer NULL in turn, spp 3, ray_index,
      bitwise repeatability, a captured graph;
  (5) a lamp that faces away, a flat field, the small-lamp limit against point_lighting;
  (6) examples/inverse_lamp.py descends.

Tolerances (scripts/rect_f32_error.py computes them on the CPU, profiles/rect/f32_error.json).  The
restatement evaluated in float32 numpy differs from itself in float64, on these scenes fed with the oracle's records and
visibility, over both lamps, no texture and both textures and K = 1, 8, 32, by at most the figures of F32 below (value and
image absolute, at RADIANCE and ALBEDO of rect_ref, values up to 7.6; every derivative as the L2 norm of the difference over
the L2 norm of the float64 result).  The GPU is allowed four times that: another operation order and fused multiply-adds.
The values depend on no mask but eligibility (the bits are an input); samples whose <sh_n, -d> is within MARGIN of zero
are left out, and so are lanes with a cosine within MARGIN from the mask comparisons: at most UNSURE_CAP of the samples
(the restatement alone leaves out at most 4.3e-4)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import rect_ref as A
from row_helpers import GUARD, UNSURE_CAP, _cu, _np, _rel, base_scene, guarded, intact, rows, sub, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ORIGINS = ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0))
TW, TH, SPP, K, KMAX, SEED = 16, 8, 4, 8, 32, 5
F32 = {"value": 2.08e-6, "image": 5.22e-7, "grad_sh_n": 2.24e-7, "grad_p": 4.93e-7, "grad_weight": 2.51e-7, "grad_tex": 1.69e-6,
       "dimage": 5.24e-7}          # the maxima of profiles/rect/f32_error.json, cut off after three digits
TOL = {k: 4 * v for k, v in F32.items()}
MARGIN = A.MARGIN
TEX = {None: None, **A.textures(TW, TH)}
COMBOS = [(oi, fn, lamp) for oi in range(2) for fn in (True, False) for lamp in A.LAMPS]


def _light(hf, lm, tex=None):
    return hf.RectLight(lm.center, lm.ex, lm.ey, lm.radiance, texture=tex)


_SCENES = {}


def _scene(hf, oracle, oi, face_normals):
    """the wavefront from origin `oi` on the shape in the given shading mode, its records as numpy, once for all tests"""
    key = (oi, face_normals)
    if key not in _SCENES:
        sc = base_scene(hf, oracle, (64, 64, SPP), ORIGINS[oi], face_normals)
        sc.ids = np.arange(sc.n, dtype=np.uint32)
        sc.draws = A.draws(sc.ids, KMAX, SEED)
        sc.eligible, sc.front = A.eligible(sc.np["sh_n"], sc.np["d"], sc.np["t"])
        sc.sure = (sc.front > MARGIN) | ~sc.hit
        sc.pix = sc.sure.reshape(-1, SPP).all(1)
        sc.runs = {}
        _SCENES[key] = sc
    return _SCENES[key]


def _run(hf, sc, lname):
    """one lamp on a scene: the 32 visibility bits of every sample and the restatement's masks, once"""
    if lname not in sc.runs:
        r = A.types.SimpleNamespace(lm=A.LAMPS[lname](A.RADIANCE))
        r.light = _light(hf, r.lm)
        _, vis = hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, albedo=A.ALBEDO, spp=SPP, num_rays=KMAX, seed=SEED,
                                  return_visibility=True)
        r.vis = vis
        r.words = _np(vis).view(np.uint32)
        r.bits = A.unpack(r.words, KMAX)
        r.g = A.geometry(sc.np["p"], sc.np["sh_n"], sc.draws, r.lm)
        r.traced, r.margin = A.traced(sc.np["sh_n"], sc.np["d"], sc.np["t"], r.g)
        sc.runs[lname] = r
    return sc.runs[lname]


def _args(sc, r, num_rays, tex, weight, m=None):
    """the restatement's arguments for the first m samples"""
    m = sc.n if m is None else m
    return (sc.np["p"][:, :m], sc.np["sh_n"][:, :m], sc.np["d"][:, :m], sc.np["t"][:m], weight, r.bits[:num_rays, :m], sc.ids[:m],
            SEED, r.lm, tex, A.ALBEDO)


def _leaf(hf, sc, sh_n=None, p=None):
    si = hf.SurfaceInteraction3f()
    si.n, si.t = sc.si.n.detach(), sc.si.t.detach()
    si.p = sc.si.p.detach().clone().requires_grad_(True) if p is None else p
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True) if sh_n is None else sh_n)
    return si


@pytest.mark.parametrize("oi,face_normals,lname", COMBOS)
def test_visibility_equals_the_two_call_sequence_bit_for_bit_and_the_masks_the_restatement(hf, oracle, oi, face_normals, lname):
    sc = _scene(hf, oracle, oi, face_normals)
    r = _run(hf, sc, lname)
    unsure = np.zeros(sc.n, bool)
    traced = np.zeros((KMAX, sc.n), bool)
    for k in range(KMAX):
        ray = hf.rect_rays(sc.si, sc.ray, r.light, k, seed=SEED)
        tr = ray.maxt >= 0
        two = tr & ~sc.shape.ray_test(ray)
        assert np.array_equal(r.bits[k], _np(two)), (k, int((r.bits[k] != _np(two)).sum()))
        traced[k] = _np(tr)
        sure = sc.sure & ((r.margin[k] > MARGIN) | ~sc.eligible)    # (a sample that is not eligible traces nothing)
        unsure |= ~sure
        assert np.array_equal(traced[k][sure], r.traced[k][sure]), k
        if k in (0, 7, 31):                                    # the materialised ray against the restatement's
            o, w, maxt, _ = A.rays(sc.np["p"], sc.np["n"], sc.np["sh_n"], sc.np["d"], sc.np["t"], sc.ids, k, SEED, r.lm)
            both = traced[k] & r.traced[k]
            assert np.abs(_np(ray.o) - o)[:, both].max() <= 1e-6 and np.abs(_np(ray.d) - w)[:, both].max() <= 2e-6
            assert np.abs(_np(ray.maxt) - maxt)[both].max() <= 1e-5 * maxt[both].max()
            assert not _np(ray.o)[:, ~traced[k]].any() and not _np(ray.d)[:, ~traced[k]].any() and (_np(ray.maxt)[~traced[k]] == -1).all()
    assert not r.bits[:, ~sc.eligible & sc.sure].any()
    print("unsure share", unsure.mean())
    assert unsure.mean() <= UNSURE_CAP, unsure.mean()
    # every num_rays is a prefix of the 32 draws
    for num_rays in (1, K):
        _, v = hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, spp=SPP, num_rays=num_rays, seed=SEED, return_visibility=True)
        assert np.array_equal(_np(v).view(np.uint32), r.words & np.uint32((1 << num_rays) - 1))
    # both outcomes of a shadow ray occur, and some samples see a part of the lamp: a run that shadows nothing cannot pass
    t8, b8 = traced[:K], r.bits[:K]
    occluded = 1.0 - b8.sum() / t8.sum()
    some, every = b8.any(0), (b8 == t8).all(0)
    penumbra = (some & ~every)[sc.eligible].mean()
    print(lname, "traced of eligible draws", t8[:, sc.eligible].mean(), "occluded of traced", occluded, "penumbra", penumbra)
    assert 0.03 <= occluded <= 0.8, occluded
    assert penumbra >= 0.05, penumbra


@pytest.mark.parametrize("oi,face_normals,lname", COMBOS)
def test_values_adjoint_and_tangent_against_the_restatement(hf, oracle, oi, face_normals, lname):
    sc = _scene(hf, oracle, oi, face_normals)
    r = _run(hf, sc, lname)
    x = A.inputs(sc.n, SPP, (TH, TW))
    sure, pix = sc.sure, sc.pix
    assert (~sure).mean() <= UNSURE_CAP
    worst = {k: 0.0 for k in TOL}
    for num_rays, name in ((K, None), (K, "smooth"), (K, "random"), (1, "random"), (KMAX, "smooth"), (KMAX, None)):
        tex = TEX[name]
        args = _args(sc, r, num_rays, tex, x.w)
        si, wt = _leaf(hf, sc), _cu(x.w).requires_grad_(True)
        td = _cu(tex).requires_grad_(True) if name else None
        kw = dict(albedo=A.ALBEDO, spp=SPP, num_rays=num_rays, seed=SEED)
        img, vis = hf.rect_lighting(sc.shape, si, sc.ray, _light(hf, r.lm, td), weight=wt, return_visibility=True, **kw)
        assert np.array_equal(_np(vis).view(np.uint32), r.words & np.uint32((1 << num_rays) - 1 if num_rays < 32 else 0xFFFFFFFF))
        ri, rv = A.forward(*args, SPP)
        err = {"image": np.abs(_np(img) - ri)[pix].max()}
        assert ri[pix].max() > 0.2
        (img * _cu(x.gi)).sum().backward()
        gn, gp, gw, gt = A.adjoint(*args, SPP, x.gi)
        got = {"grad_sh_n": _np(si.sh_frame.n.grad), "grad_p": _np(si.p.grad), "grad_weight": _np(wt.grad)}
        for k, ref in (("grad_sh_n", gn), ("grad_p", gp), ("grad_weight", gw)):
            assert not got[k][..., ~sc.eligible & sure].any()                       # exact zeros where nothing is shaded
            assert np.linalg.norm(ref) > 0
            err[k] = _rel(got[k][..., sure], ref[..., sure])
        if name:
            # (the texels' gradient adds up every sample: the few unsure ones stay in, their part is below the tolerance)
            got["grad_tex"] = _np(td.grad)
            err["grad_tex"] = _rel(got["grad_tex"], gt)
        with fwAD.dual_level():
            sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
            tdd = fwAD.make_dual(_cu(tex), _cu(x.dtex)) if name else None
            ti = hf.rect_lighting(sc.shape, sid, sc.ray, _light(hf, r.lm, tdd), weight=fwAD.make_dual(_cu(x.w), _cu(x.dw)), **kw)
            timg = _np(fwAD.unpack_dual(ti).tangent)
        dimg, _ = A.tangent(*args, SPP, x.dn, x.dp, x.dw, x.dtex if name else None)
        err["dimage"] = _rel(timg[pix], dimg[pix])
        # transposition on the device, forward_ad against backward through the public function: <J u, v> = <u, J^T v>,
        # both sides float32 results added up in float64; each side is within its tolerance of the exact bilinear form
        rhs = [(got["grad_sh_n"], x.dn), (got["grad_p"], x.dp), (got["grad_weight"], x.dw)] + ([(got["grad_tex"], x.dtex)] if name else [])
        gap = transposition_gap(((timg, x.gi),), rhs)
        size = np.linalg.norm(dimg) * np.linalg.norm(x.gi)
        assert gap <= (TOL["dimage"] + TOL["grad_p"]) * size, (gap, size)
        if num_rays == K and name is None:
            # the per-sample values: spp = 1, the image is the wavefront
            val = hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, weight=_cu(x.w), albedo=A.ALBEDO, spp=1, num_rays=K, seed=SEED)
            err["value"] = np.abs(_np(val) - rv)[sure].max()
            assert not _np(val)[~sc.eligible & sure].any() and rv.max() > 1.0
        print(num_rays, name, {k: "%.3g" % v for k, v in err.items()})
        for k in err:
            worst[k] = max(worst[k], err[k])
    print("worst", {k: "%.3g / %.3g" % (worst[k], TOL[k]) for k in TOL})
    for k in TOL:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


@pytest.mark.parametrize("face_normals", [True, False])
def test_chain_to_the_heights(hf, oracle, face_normals):
    """rect_lighting -> loss -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n and grad_p (fed
    with the GPU's records and bits), carried to the heights by the oracle's adjoint (flat shading) or by hf_adjoint, which
    tests/test_gpu_smooth_shading.py holds against float64 (smooth shading).  Bound: four times the float32 error of
    grad_p (the larger of the two gradients' errors) + the 1e-5 of the sky row's chain."""
    sc = _scene(hf, oracle, 0, face_normals)
    r = _run(hf, sc, "side")
    x = A.inputs(sc.n, SPP, (TH, TW))
    gi = np.where(sc.pix, x.gi, 0).astype(np.float32)
    shape = hf.Heightfield(heightfield=sc.h.clone(), max_height=0.5, face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.rect_lighting(shape, si, sc.ray, _light(hf, r.lm, _cu(TEX["smooth"])), albedo=A.ALBEDO, spp=SPP, num_rays=K,
                                seed=SEED, return_visibility=True)
    assert np.array_equal(_np(vis).view(np.uint32), r.words & np.uint32(0xFF))
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad)
    a = (_np(si.p), _np(si.sh_frame.n), _np(sc.ray.d), _np(si.t), None, r.bits[:K], sc.ids, SEED, r.lm, TEX["smooth"], A.ALBEDO)
    gn, gp, _, _ = A.adjoint(*a, SPP, gi)
    rr = _np(sc.rays)
    if face_normals:
        t, u, v, prim = sc.field.ray_intersect_preliminary(rr)
        gh = sc.field.adjoint(rr, t, u, v, prim, {"sh_n": gn.astype(np.float32), "p": gp.astype(np.float32)}, oracle.RAY_ALL)
    else:
        ybar = torch.zeros((18, sc.n), device="cuda")
        ybar[1:4] = _cu(gp.astype(np.float32)); ybar[9:12] = _cu(gn.astype(np.float32))
        pi = shape.ray_intersect_preliminary(sc.ray)
        gh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All)))
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print("face_normals", face_normals, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= TOL["grad_p"] + 1e-5, err


def test_repeatable_ray_index_and_edge_cases(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "above")
    x = A.inputs(sc.n, SPP, (TH, TW))
    runs = []
    for _ in range(2):
        si, wt = _leaf(hf, sc), _cu(x.w).requires_grad_(True)
        img, vis = hf.rect_lighting(sc.shape, si, sc.ray, _light(hf, r.lm, _cu(TEX["random"])), weight=wt, albedo=A.ALBEDO, spp=SPP,
                                    num_rays=K, seed=SEED, return_visibility=True)
        (img * _cu(x.gi)).sum().backward()
        with fwAD.dual_level():
            sid = _leaf(hf, sc, fwAD.make_dual(sc.si.sh_frame.n.detach(), _cu(x.dn)), fwAD.make_dual(sc.si.p.detach(), _cu(x.dp)))
            tan = fwAD.unpack_dual(hf.rect_lighting(sc.shape, sid, sc.ray, _light(hf, r.lm, _cu(TEX["random"])), albedo=A.ALBEDO,
                                                    spp=SPP, num_rays=K, seed=SEED)).tangent
        runs.append((vis.clone(), img.detach().clone(), si.sh_frame.n.grad.clone(), si.p.grad.clone(), wt.grad.clone(), tan.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                          # everything but grad_tex: bitwise
    # a permuted ray_index: the draws follow the id, and the fused kernel still equals the two-call sequence
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(6)).to(device="cuda", dtype=torch.int32)
    img, vis = hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, albedo=A.ALBEDO, spp=SPP, num_rays=2, seed=SEED, ray_index=ids,
                                return_visibility=True)
    b = A.unpack(_np(vis), 2)
    for k in range(2):
        ray = hf.rect_rays(sc.si, sc.ray, r.light, k, seed=SEED, ray_index=ids)
        assert np.array_equal(b[k], _np((ray.maxt >= 0) & ~sc.shape.ray_test(ray))), k
    assert not np.array_equal(b, r.bits[:2])
    ri, _ = A.forward(sc.np["p"], sc.np["sh_n"], sc.np["d"], sc.np["t"], None, b, _np(ids).view(np.uint32), SEED, r.lm, None, A.ALBEDO, SPP)
    assert np.abs(_np(img) - ri)[sc.pix].max() <= TOL["image"]
    same = hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, spp=SPP, num_rays=K, seed=SEED, return_visibility=True,
                            ray_index=torch.arange(sc.n, dtype=torch.int32, device="cuda"))[1]
    assert np.array_equal(_np(same).view(np.uint32), r.words & np.uint32(0xFF))
    # n = 0 is legal
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, vis0 = hf.rect_lighting(sc.shape, si0, ray0, r.light, spp=SPP, num_rays=K, return_visibility=True)
    assert img0.shape == (0,) and vis0.shape == (0,)
    img0.sum().backward()
    assert len(hf.rect_rays(si0, ray0, r.light, 0)) == 0
    # a wavefront with no eligible sample: rays that leave the terrain behind, and hits seen from behind
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    for s, ry in ((sim, up), (sc.si, up)):
        imgm, vism = hf.rect_lighting(sc.shape, s, ry, r.light, spp=SPP, num_rays=K, return_visibility=True)
        assert not bool(imgm.any()) and not bool(vism.any())
    for bad in (dict(spp=3), dict(num_rays=33), dict(num_rays=0)):
        with pytest.raises(hf.HfError):
            hf.rect_lighting(sc.shape, sc.si, sc.ray, r.light, **{"spp": SPP, **bad})


@pytest.mark.parametrize("spp", [1, 3])
def test_odd_sizes_guard_bands_and_optional_pointers(hf, oracle, spp):
    """n = spp * 151 (two whole workgroup batches of 64 and a part of one; spp 3 is no power of two: the film's other
    paths), guard values around every output row, and every optional pointer NULL in turn"""
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "side")
    lib, check = hf._capi.lib(), hf._capi.check
    n, G = spp * 151, 96
    start = int(torch.nonzero(sc.si.is_valid())[0]) // 64 * 64
    cut = lambda v: v.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    assert bool(torch.isfinite(t).any())
    ids = torch.arange(start, start + n, dtype=torch.int32, device="cuda")
    x = A.inputs(n, spp, (TH, TW))
    w, tex = _cu(x.w), _cu(TEX["random"])
    lamp = r.light._struct()
    stream = torch.cuda.current_stream().cuda_stream
    mid = lambda wp, tp: (wp, K, SEED, ids.data_ptr(), lamp, TW if tp else 0, TH if tp else 0, tp, A.ALBEDO)
    image, ip = guarded(n // spp, G)
    vis = torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    check(lib.hf_rect_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), *mid(w.data_ptr(), tex.data_ptr()),
                               ip[0], vis.data_ptr() + 4 * G, stream))
    assert intact(image, n // spp, G)
    assert bool((vis[:G] == 0x5A5A5A5A).all()) and bool((vis[G + n:] == 0x5A5A5A5A).all())
    words = vis[G:G + n].contiguous()
    assert np.array_equal(_np(words).view(np.uint32), r.words[start:start + n] & np.uint32(0xFF))   # the slice of the whole
    bits = A.unpack(_np(words), K)
    a = tuple(_np(v) for v in (p, sn, d, t))
    ref_img, _ = A.forward(*a, x.w, bits, _np(ids).view(np.uint32), SEED, r.lm, TEX["random"], A.ALBEDO, spp)
    front = A.eligible(*a[1:])[1]
    pix = ((front > MARGIN) | ~np.isfinite(a[3])).reshape(-1, spp).all(1)
    assert np.abs(_np(image[0, G:G + n // spp]) - ref_img)[pix].max() <= TOL["image"]
    # the forward without its optional pointers (weight, ray_id, tex, vis_bits) writes the same film as with them where
    # they say the same thing
    img2, ip2 = guarded(n // spp, G)
    one = torch.ones(n, device="cuda")
    check(lib.hf_rect_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), one.data_ptr(), K, SEED,
                               ids.data_ptr(), lamp, 0, 0, None, A.ALBEDO, ip2[0], None, stream))
    img3, ip3 = guarded(n // spp, G)
    check(lib.hf_rect_lighting(sc.shape._h, n, spp, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), None, K, SEED,
                               ids.data_ptr(), lamp, 0, 0, None, A.ALBEDO, ip3[0], None, stream))
    assert torch.equal(img2, img3) and intact(img2, n // spp, G)
    # the adjoint: all outputs, then each one NULL in turn -- the others are bitwise what they were, grad_tex to rounding
    gi = _cu(x.gi)
    head = (n, spp, rows(p), rows(sn), rows(d), t.data_ptr())

    def adjoint(skip=None):
        gn, gnp = guarded(n, G, 3); gp, gpp = guarded(n, G, 3); gw, gwp = guarded(n, G)
        gt = torch.zeros((TH, TW), device="cuda")
        check(lib.hf_rect_lighting_adjoint(*head, *mid(w.data_ptr(), tex.data_ptr()), words.data_ptr(), gi.data_ptr(),
                                           None if skip == "gn" else gnp, None if skip == "gp" else gpp,
                                           None if skip == "gw" else gwp[0], None if skip == "gt" else gt.data_ptr(), stream))
        return {"gn": gn, "gp": gp, "gw": gw, "gt": gt}
    full = adjoint()
    assert intact(full["gn"], n, G) and intact(full["gp"], n, G) and intact(full["gw"], n, G)
    gn_ref, gp_ref, gw_ref, gt_ref = A.adjoint(*a, x.w, bits, _np(ids).view(np.uint32), SEED, r.lm, TEX["random"], A.ALBEDO, spp, x.gi)
    sure = (front > MARGIN) | ~np.isfinite(a[3])
    assert _rel(_np(full["gn"][:, G:G + n])[:, sure], gn_ref[:, sure]) <= TOL["grad_sh_n"]
    assert _rel(_np(full["gp"][:, G:G + n])[:, sure], gp_ref[:, sure]) <= TOL["grad_p"]
    assert _rel(_np(full["gw"][0, G:G + n])[sure], gw_ref[sure]) <= TOL["grad_weight"]
    assert _rel(_np(full["gt"]), gt_ref) <= TOL["grad_tex"]
    for skip in ("gn", "gp", "gw", "gt"):
        part = adjoint(skip)
        for k in ("gn", "gp", "gw"):
            if k == skip:
                assert bool((part[k] == GUARD).all())                   # untouched
            else:
                assert torch.equal(part[k], full[k])
        if skip == "gt":
            assert not bool(part["gt"].any())
        else:
            assert _rel(_np(part["gt"]), _np(full["gt"]).astype(np.float64)) <= 1e-5   # (float atomics: the order differs)
    # the tangent: every tangent NULL in turn, and their sum is the whole (the map is linear)
    dn, dp, dw, dtex = _cu(x.dn), _cu(x.dp), _cu(x.dw), _cu(x.dtex)

    def tangent(use):
        out, op = guarded(n // spp, G)
        check(lib.hf_rect_lighting_tangent(*head, *mid(w.data_ptr(), tex.data_ptr()), words.data_ptr(),
                                           rows(dn) if "dn" in use else None, rows(dp) if "dp" in use else None,
                                           dw.data_ptr() if "dw" in use else None, dtex.data_ptr() if "dtex" in use else None,
                                           op[0], stream))
        assert intact(out, n // spp, G)
        return _np(out[0, G:G + n // spp]).astype(np.float64)
    whole = tangent(("dn", "dp", "dw", "dtex"))
    parts = sum(tangent((k,)) for k in ("dn", "dp", "dw", "dtex"))
    assert not tangent(()).any()
    dref, _ = A.tangent(*a, x.w, bits, _np(ids).view(np.uint32), SEED, r.lm, TEX["random"], A.ALBEDO, spp, x.dn, x.dp, x.dw, x.dtex)
    assert _rel(whole[pix], dref[pix]) <= TOL["dimage"]
    assert np.linalg.norm(whole - parts) <= 5 * TOL["dimage"] * np.linalg.norm(dref)      # (five results, each within its tolerance)
    # the rays
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G)
    check(lib.hf_rect_rays(n, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), 3, SEED, ids.data_ptr(), lamp, rop, rdp, rmp[0], stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G)
    torch.cuda.synchronize()


def test_captured_graph_replays_to_the_same_bits(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    r = _run(hf, sc, "side")
    lib = hf._capi.lib()
    lamp, tex = r.light._struct(), _cu(TEX["smooth"])
    p, nr, sn, d, t = (v.detach().contiguous() for v in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    img = torch.zeros(sc.n // SPP, device="cuda"); vis = torch.zeros(sc.n, dtype=torch.int32, device="cuda")
    gn = torch.zeros((3, sc.n), device="cuda"); gp = torch.zeros((3, sc.n), device="cuda")
    dimg = torch.zeros(sc.n // SPP, device="cuda")
    gi, ones = torch.ones(sc.n // SPP, device="cuda"), torch.ones((3, sc.n), device="cuda")
    mid = (None, K, SEED, None, lamp, TW, TH, tex.data_ptr(), A.ALBEDO)

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        hf._capi.check(lib.hf_rect_lighting(sc.shape._h, sc.n, SPP, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), *mid,
                                            img.data_ptr(), vis.data_ptr(), s))
        hf._capi.check(lib.hf_rect_lighting_adjoint(sc.n, SPP, rows(p), rows(sn), rows(d), t.data_ptr(), *mid, vis.data_ptr(),
                                                    gi.data_ptr(), rows(gn), rows(gp), None, None, s))
        hf._capi.check(lib.hf_rect_lighting_tangent(sc.n, SPP, rows(p), rows(sn), rows(d), t.data_ptr(), *mid, vis.data_ptr(),
                                                    rows(ones), rows(ones), None, None, dimg.data_ptr(), s))
    outs = (img, vis, gn, gp, dimg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert np.array_equal(_np(vis).view(np.uint32), r.words & np.uint32(0xFF)) and float(img.abs().sum()) > 0
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


def test_a_lamp_that_faces_away_lights_nothing_and_a_flat_field_sees_every_traced_draw(hf, oracle):
    sc = _scene(hf, oracle, 1, True)
    lm = A.lamp((0.2, -0.1, 1.1), (0.3, 0.0, 0.05), (0.0, 0.2, 0.0), A.RADIANCE)     # the lamp above, its normal up
    assert lm.nl[2] > 0
    img, vis = hf.rect_lighting(sc.shape, sc.si, sc.ray, _light(hf, lm), spp=SPP, num_rays=KMAX, seed=SEED, return_visibility=True)
    assert not bool(vis.any()) and not bool(img.any())                               # exactly 0
    shape, si, ray = _flat(hf)
    for lname in A.LAMPS:
        lm = A.LAMPS[lname](A.RADIANCE)
        light = _light(hf, lm)
        _, vis = hf.rect_lighting(shape, si, ray, light, spp=1, num_rays=K, seed=SEED, return_visibility=True)
        bits = A.unpack(_np(vis), K)
        for k in range(K):
            tr = _np(hf.rect_rays(si, ray, light, k, seed=SEED).maxt >= 0)
            assert np.array_equal(bits[k], tr), k                                    # nothing occludes
        assert bits.mean() > 0.1


def test_a_small_lamp_far_away_is_a_point_light(hf):
    """A square lamp with half-extents e = 1e-3 at distance r >= 1 over a flat field against hf_amd.point_lighting at
    intensity L A, times c_l towards the lamp's centre per sample.  To first order in e / r
        |G(q) - G(centre)| / G <= |grad_q log G| |q - centre| <= (4 + 1 / c_s + 1 / c_l) sqrt(2) e / r
    (grad_u log G = sh_n / <sh_n, u> - n_l / <n_l, u> - 4 u / r^2: three terms of norm 1 / (c_s r), 1 / (c_l r), 4 / r, and a
    point of the lamp is at most sqrt(2) e from its centre), taken over the scene's smallest cosines and r; plus the float32
    tolerance of a value (TOL["value"]) for each of the two kernels."""
    shape, si, ray = _flat(hf)
    e, L, albedo = 1e-3, 1e6, 0.8                                                    # (A = 4e-6: values of order 0.3)
    lm = A.lamp((0.1, -0.2, 1.7), (e, 0.0, 0.0), (0.0, -e, 0.0), L)                 # faces down, 1.2 above the field
    light = _light(hf, lm)
    img, vis = hf.rect_lighting(shape, si, ray, light, albedo=albedo, spp=1, num_rays=K, seed=SEED, return_visibility=True)
    assert bool((vis == 0xFF).all())
    area, _ = light.geometry()
    pt = hf.point_lighting(si, ray, [[*lm.center, L * area]], albedo=albedo, spp=1)[0]
    u = lm.center[:, None] - _np(si.p).astype(np.float64)
    rr = np.linalg.norm(u, axis=0)
    cl = -(lm.nl[:, None] * u).sum(0) / rr
    cs = (_np(si.sh_frame.n).astype(np.float64) * u).sum(0) / rr
    ref = _np(pt).astype(np.float64) * cl
    assert rr.min() >= 1.0 and ref.min() > 0.01
    bound = (4 + 1 / cs.min() + 1 / cl.min()) * np.sqrt(2) * e / rr.min()
    err = np.abs(_np(img) - ref)
    print("worst relative difference", (err / ref).max(), "bound", bound)
    assert (err <= bound * ref + 2 * TOL["value"]).all(), (err / ref).max()


def test_inverse_lamp_example_descends(hf):
    import inverse_lamp
    hist, err = inverse_lamp.run(size=48, steps=31, verbose=False)
    assert np.isfinite(hist[-1]) and hist[30] < hist[0], (hist[0], hist[30])

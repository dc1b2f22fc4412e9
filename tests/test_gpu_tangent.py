"""Forward mode on the GPU: hf_tangent, the two lighting tangents and the jvp of the autograd Functions
(torch.autograd.forward_ad), against
  * the reference's forward-mode known answers (src/render/tests/test_mesh.py test13 :380-422, test15 :458-531,
    test17 :674-735; src/shapes/tests/test_rectangle.py:116-155 test06), run directly in forward mode;
  * float64 central differences of tests/si_numpy.py along the same random direction (dh, do, dd), per ray, in all
    three modes, with flipped normals and a general affine to_world (the yardstick is itself checked against the
    oracle's adjoint in tests/test_tangent_abi.py);
  * hf_adjoint by transposition, <ybar, J delta> = <J^T ybar, delta>, up to the bench wavefront (4096^2, 67.1 M rays);
  * the reverse-mode derivative image (dual heights -> ray_intersect -> lighting -> film_gaussian).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import common
import si_numpy as S

pytestmark = pytest.mark.gpu

ROWS = {"t": (0, 1), "p": (1, 4), "n": (4, 7), "uv": (7, 9), "sh_n": (9, 12), "dp_du": (12, 15), "dp_dv": (15, 18)}
MODES = {"default": 0, "follow": S.RAY_FOLLOWSHAPE, "detach": S.RAY_DETACHSHAPE}


def _tan(x):
    t = fwAD.unpack_dual(x).tangent
    return torch.zeros_like(fwAD.unpack_dual(x).primal) if t is None else t


def _ray(hf, o, d):
    o = torch.tensor(o, dtype=torch.float32).reshape(3, 1).cuda()
    d = torch.tensor(d, dtype=torch.float32).reshape(3, 1).cuda()
    return o, d


# ---- 1. the reference's forward-mode known answers -------------------------------------------------------------

def _flat(hf, W=2, H=2):
    return hf.Heightfield(heightfield=torch.zeros((H, W)).cuda(), max_height=1.0)


def _fwd_ray(hf, shape, o, d, do=None, dd=None, dh=None, flags=None):
    """one ray through ray_intersect inside a dual level; returns the tangents of si (as numpy, [k] per field)"""
    flags = int(hf.RayFlags.All) if flags is None else int(flags)
    h0 = shape.heightfield
    with fwAD.dual_level():
        oo = fwAD.make_dual(o, torch.tensor(do, dtype=torch.float32).reshape(3, 1).cuda()) if do is not None else o
        ddd = fwAD.make_dual(d, torch.tensor(dd, dtype=torch.float32).reshape(3, 1).cuda()) if dd is not None else d
        if dh is not None:
            shape.heightfield = fwAD.make_dual(h0, torch.as_tensor(dh, dtype=torch.float32).cuda())
        try:
            si = shape.ray_intersect(hf.Ray3f(oo, ddd, torch.full((1,), math.inf).cuda()), flags)
            out = {nm: _tan(getattr(si, nm))[..., 0].cpu().numpy() for nm in ("t", "p", "n", "uv", "dp_du", "dp_dv")}
            out["sh_n"] = _tan(si.sh_frame.n)[:, 0].cpu().numpy()
        finally:
            shape.heightfield = h0
    return out


@pytest.mark.parametrize("W,H", [(2, 2), (5, 4), (33, 17)])
def test13_rectangle_test06_ray_forward(hf, W, H):
    shape = _flat(hf, W, H)
    o, d = _ray(hf, [-0.3, -0.3, -10.0], [0, 0, 1])
    ox = _fwd_ray(hf, shape, o, d, do=[1, 0, 0])
    assert np.allclose(ox["p"], [1, 0, 0], atol=1e-5) and np.allclose(ox["uv"], [0.5, 0], atol=1e-5)
    assert abs(float(ox["t"])) < 1e-5
    oy = _fwd_ray(hf, shape, o, d, do=[0, 1, 0])
    assert np.allclose(oy["p"], [0, 1, 0], atol=1e-5) and np.allclose(oy["uv"], [0, 0.5], atol=1e-5)
    oz = _fwd_ray(hf, shape, o, d, do=[0, 0, 1])
    assert abs(float(oz["t"]) - (-1.0)) < 1e-5 and np.allclose(oz["p"], 0, atol=1e-5)
    dx = _fwd_ray(hf, shape, o, d, dd=[1, 0, 0])
    assert np.allclose(dx["p"], [10, 0, 0], atol=1e-4)
    for r in (ox, oy, oz, dx):   # a ray perturbation does not turn a flat grid's normal
        assert np.allclose(r["n"], 0, atol=1e-6) and np.allclose(r["sh_n"], 0, atol=1e-6)


def test15_uniform_lift(hf):
    """test15: the vertex positions move up by one: dt = 1 (ray from below), dp = [0,0,1], duv = 0"""
    shape = _flat(hf, 4, 3)
    o, d = _ray(hf, [0.1, -0.2, -10.0], [0, 0, 1])
    r = _fwd_ray(hf, shape, o, d, dh=np.ones((3, 4)))
    assert abs(float(r["t"]) - 1.0) < 1e-5
    assert np.allclose(r["p"], [0, 0, 1], atol=1e-5) and np.allclose(r["uv"], 0, atol=1e-6)
    assert np.allclose(r["n"], 0, atol=1e-6) and np.allclose(r["dp_du"], 0, atol=1e-6)


def test17_default_followshape_detachshape(hf):
    """test17 in the form of a grid (test_gpu_known_answers.py::test17): uniform lift, slanted ray from above"""
    shape = _flat(hf)
    o, d = _ray(hf, [-0.5, 0.1, 2.0], [0.3, 0.1, -1.0])
    lift = np.ones((2, 2))
    A = hf.RayFlags.All
    r = _fwd_ray(hf, shape, o, d, dh=lift, flags=A)
    dn = np.array([0.3, 0.1, -1.0], np.float32)
    assert abs(float(r["t"]) - (-1.0)) < 1e-5 and np.allclose(r["p"], -dn, atol=1e-5)
    assert np.allclose(r["uv"], [-0.3 * 0.5, -0.1 * 0.5], atol=1e-5)
    r = _fwd_ray(hf, shape, o, d, dh=lift, flags=A | hf.RayFlags.FollowShape)
    assert np.allclose(r["p"], [0, 0, 1], atol=1e-5) and np.allclose(r["uv"], 0, atol=1e-6)
    # FollowShape: t = |p - o| / |d| with p glued to the lifted plane
    pd = np.array([-0.5 + 0.6, 0.1 + 0.2, 0.0]) - np.array([-0.5, 0.1, 2.0])
    assert abs(float(r["t"]) - float(pd @ np.array([0, 0, 1.0])) / float(np.linalg.norm(pd) * np.linalg.norm(dn))) < 1e-5
    r = _fwd_ray(hf, shape, o, d, dh=lift, flags=A | hf.RayFlags.DetachShape)
    assert all(np.all(v == 0) for v in r.values())


# ---- 2. per ray against float64 central differences ------------------------------------------------------------

def _fd(h, s, tw, flip, o, d, prim, flags, uvf, dh, do, dd, eps=1e-6):
    # (float64: eps = 1e-6 leaves ~1e-10 of rounding; 1e-4 is too coarse where FollowShape's t = |p - o| / |d| is small)
    def rows(e):
        si = S.surface_interaction(h + e * dh, s, tw, flip, o + e * do, d + e * dd, prim, flags, uvf, h)
        return np.concatenate([np.atleast_1d(np.asarray(si[nm], np.float64)) for nm, _ in S.GRAD_FIELDS])
    return (rows(eps) - rows(-eps)) / (2 * eps)


def _scene(hf, W, H, kind, flip, affine, n, seed):
    rng = np.random.default_rng(seed)
    s = 0.6
    h = common.heights(kind, W, H, rng) if kind != "rand" else rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
    tw = common.affine(seed) if affine else None
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).cuda(), max_height=s, flip_normals=flip,
                           to_world=torch.from_numpy(tw) if affine else None)
    r = common.to_world_rays(common.random_rays(n, rng, s), tw)
    rt = torch.from_numpy(r).cuda()
    ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
    return rng, h, s, (tw if affine else np.eye(4)[:3]), shape, r, ray


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", [(2, 2, "rand", 64), (9, 7, "rand", 256), (257, 257, "sine", 8000)])
def test_tangent_vs_float64_central_differences(hf, grid, mode, flip, affine):
    W, H, kind, n = grid
    rng, h, s, tw, shape, r, ray = _scene(hf, W, H, kind, flip, affine, n, seed=W + 3 * flip + 7 * affine)
    flags = int(hf.RayFlags.All) | MODES[mode]
    pi = shape.ray_intersect_preliminary(ray)
    dh = rng.normal(size=(H, W)).astype(np.float32)
    do = rng.normal(size=(3, n)).astype(np.float32); dd = rng.normal(size=(3, n)).astype(np.float32)
    tg = shape.tangent(ray, pi, torch.from_numpy(dh).cuda(), torch.from_numpy(do).cuda(), torch.from_numpy(dd).cuda(),
                       ray_flags=flags).cpu().numpy()
    t = pi.t.cpu().numpy(); uv = pi.prim_uv.cpu().numpy(); prim = pi.prim_index.cpu().numpy().view(np.uint32)
    hits = np.where(np.isfinite(t))[0]
    assert np.all(tg[:, ~np.isfinite(t)] == 0)
    h64 = h.astype(np.float64)
    checked = 0
    for k in hits[:2500]:
        o64, d64 = r[0:3, k].astype(np.float64), r[3:6, k].astype(np.float64)
        si = S.surface_interaction(h64, s, tw, flip, o64, d64, prim[k], flags, (uv[0, k], uv[1, k]), h64)
        if abs(float(si["n"] @ d64)) < 1e-2 * np.linalg.norm(d64):
            continue
        ref = _fd(h64, s, tw, flip, o64, d64, prim[k], flags, (uv[0, k], uv[1, k]),
                  dh.astype(np.float64), do[:, k].astype(np.float64), dd[:, k].astype(np.float64))
        assert np.allclose(tg[:, k], ref, rtol=2e-4, atol=2e-4 * (1 + np.abs(ref).max())), (k, tg[:, k], ref)
        checked += 1
    assert checked >= min(2000, len(hits) // 2) and checked >= 1
    # each tangent input alone = the combined run with the other two set to zero
    z3 = torch.zeros((3, n), device="cuda"); zh = torch.zeros((H, W), device="cuda")
    parts = [shape.tangent(ray, pi, torch.from_numpy(dh).cuda(), ray_flags=flags),
             shape.tangent(ray, pi, d_o=torch.from_numpy(do).cuda(), ray_flags=flags),
             shape.tangent(ray, pi, d_d=torch.from_numpy(dd).cuda(), ray_flags=flags)]
    zeros = [shape.tangent(ray, pi, torch.from_numpy(dh).cuda(), z3, z3, ray_flags=flags),
             shape.tangent(ray, pi, zh, torch.from_numpy(do).cuda(), z3, ray_flags=flags),
             shape.tangent(ray, pi, zh, z3, torch.from_numpy(dd).cuda(), ray_flags=flags)]
    for a, b in zip(parts, zeros):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6 * (1 + float(b.abs().max())))
    total = (parts[0].double() + parts[1].double() + parts[2].double()).cpu().numpy()
    assert np.allclose(total, tg, rtol=1e-4, atol=1e-4 * (1 + np.abs(tg).max()))


# ---- 3. transposition with hf_adjoint -----------------------------------------------------------------------------

def _transpose_check(hf, shape, ray, pi, flags, with_rays, seed, row_band=False):
    n = len(ray)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    ybar = torch.randn((18, n), device="cuda", generator=g)
    dh = torch.randn((shape.height, shape.width), device="cuda", generator=g)
    do = torch.randn((3, n), device="cuda", generator=g) if with_rays else None
    dd = torch.randn((3, n), device="cuda", generator=g) if with_rays else None
    jd = shape.tangent(ray, pi, dh, do, dd, ray_flags=flags)
    per_ray = (ybar.double() * jd.double()).sum(0)
    lhs = float(per_ray.sum()); scale = float(per_ray.abs().sum())
    del jd, per_ray
    band = shape.new_row_band() if row_band else None
    if with_rays:
        gh, go, gd = shape.adjoint(ray, pi, ybar, ray_flags=flags, ray_grads=True, row_band=band)
        rhs = float((dh.double() * gh.double()).sum() + (do.double() * go.double()).sum() + (dd.double() * gd.double()).sum())
    else:
        gh = shape.adjoint(ray, pi, ybar, ray_flags=flags, row_band=band)
        rhs = float((dh.double() * gh.double()).sum())
    if row_band:   # rows outside the band received nothing
        lo, hi = band.cpu().tolist()
        assert 0 <= lo < hi <= shape.height
        assert float(gh[:lo].abs().sum()) == 0 and float(gh[hi:].abs().sum()) == 0
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("mode", list(MODES))
def test_transpose_of_adjoint_configs1(hf, mode):
    """configs[1] size: 1024^2 sine field, 512^2 x 16 spp camera rays"""
    h = hf.workload.sine_heights(1024, 1024, device="cuda")
    shape = hf.Heightfield(heightfield=h, max_height=0.5)
    rays = hf.workload.ortho_rays(512, 512, 16, "cuda")
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    pi = shape.ray_intersect_preliminary(ray)
    assert int(pi.is_valid().sum()) > 100000
    _transpose_check(hf, shape, ray, pi, int(hf.RayFlags.All) | MODES[mode], with_rays=True, seed=5)


def test_transpose_of_adjoint_bench_workload(hf):
    """the bench wavefront (4096^2 sine field, 1024^2 x 64 spp = 67.1 M rays): the first independent check of the
    adjoint's LDS-tile and row-band path at that size (heights only, as the bench runs it) and of its ray gradients"""
    h = hf.workload.sine_heights(4096, 4096, device="cuda")
    shape = hf.Heightfield(heightfield=h, max_height=0.5)
    rays = hf.workload.ortho_rays(1024, 1024, 64, "cuda")
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    del rays
    pi = shape.ray_intersect_preliminary(ray)
    hit_frac = float(pi.is_valid().float().mean())
    assert 0.2 < hit_frac < 0.3, hit_frac
    _transpose_check(hf, shape, ray, pi, int(hf.RayFlags.All), with_rays=False, seed=6, row_band=True)
    _transpose_check(hf, shape, ray, pi, int(hf.RayFlags.All), with_rays=True, seed=7)


# ---- 4. edge lanes -------------------------------------------------------------------------------------------------

def _small(hf, n=512, seed=2):
    rng, h, s, tw, shape, r, ray = _scene(hf, 33, 17, "rand", False, True, n, seed)
    return rng, shape, ray


def test_missed_inactive_and_recursion_depth_lanes_are_zero(hf):
    rng, shape, ray = _small(hf)
    n = len(ray)
    pi = shape.ray_intersect_preliminary(ray)
    hit = pi.is_valid()
    assert 0 < int(hit.sum()) < n
    dh = torch.randn((shape.height, shape.width), device="cuda")
    do = torch.randn((3, n), device="cuda"); dd = torch.randn((3, n), device="cuda")
    active = torch.from_numpy(rng.uniform(size=n) < 0.5).cuda()
    tg = shape.tangent(ray, pi, dh, do, dd, active=active)
    assert torch.all(tg[:, ~(hit & active)] == 0)
    assert bool((tg[:, hit & active] != 0).any())
    full = shape.tangent(ray, pi, dh, do, dd)
    assert torch.equal(full[:, active], tg[:, active])
    # recursion_depth > 0 (mesh.cpp:680-682): zero record, zero tangent
    h0 = shape.heightfield
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(h0, dh)
        try:
            si = shape.compute_surface_interaction(ray, pi, hf.RayFlags.All, recursion_depth=1)
            assert torch.all(_tan(si.t) == 0) and torch.all(_tan(si.p) == 0) and torch.all(_tan(si.n) == 0)
            si = shape.compute_surface_interaction(ray, pi, hf.RayFlags.All)
            assert torch.allclose(_tan(si.p), shape.tangent(ray, pi, dh)[1:4])
        finally:
            shape.heightfield = h0


def test_null_inputs_are_zero_and_null_outputs_untouched_and_bitwise_repeatable(hf):
    rng, shape, ray = _small(hf)
    n = len(ray)
    pi = shape.ray_intersect_preliminary(ray)
    hit = pi.is_valid()
    assert torch.all(shape.tangent(ray, pi) == 0)
    dh = torch.randn((shape.height, shape.width), device="cuda")
    do = torch.randn((3, n), device="cuda")
    a = shape.tangent(ray, pi, dh, do)
    b = shape.tangent(ray, pi, dh, do)
    assert torch.equal(a, b)
    # the C ABI with only some output rows: the others are not written
    out = torch.full((18, n), float("nan"), device="cuda")
    ts = hf._capi.hf_si_tangent_t()
    ts.t = out[0].data_ptr()
    for c in range(3):
        ts.n[c] = out[4 + c].data_ptr()
    rays = shape._rays_struct(ray.o, ray.d, ray.maxt)
    pis = shape._pi_struct(pi.t, pi.prim_uv, pi.prim_index)
    dop = (C.c_void_p * 3)(do[0].data_ptr(), do[1].data_ptr(), do[2].data_ptr())
    nul = (C.c_void_p * 3)(None, None, None)
    hf._capi.check(hf._capi.lib().hf_tangent(shape._h, n, C.byref(rays), C.byref(pis), int(hf.RayFlags.All), None,
                                             dh.data_ptr(), C.byref(dop), C.byref(nul), C.byref(ts), shape._stream()))
    torch.cuda.synchronize()
    for k in range(18):
        if k == 0 or 4 <= k < 7:
            assert torch.equal(out[k], a[k]), k
        else:
            assert torch.all(torch.isnan(out[k])), k
    assert bool((a[:, hit] != 0).any())


def test_detach_shape_zero_height_part_nonzero_ray_part(hf):
    rng, shape, ray = _small(hf)
    n = len(ray)
    pi = shape.ray_intersect_preliminary(ray)
    hit = pi.is_valid()
    De = int(hf.RayFlags.All | hf.RayFlags.DetachShape)
    dh = torch.randn((shape.height, shape.width), device="cuda")
    assert torch.all(shape.tangent(ray, pi, dh, ray_flags=De) == 0)
    tr = shape.tangent(ray, pi, None, torch.randn((3, n), device="cuda"), torch.randn((3, n), device="cuda"), ray_flags=De)
    assert bool((tr[0:4, hit] != 0).all())   # t and p move with the ray
    # through forward AD: DetachShape drops the heights' tangent, keeps the ray's
    h0 = shape.heightfield
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(h0, dh)
        try:
            si = shape.ray_intersect(ray, De)
            assert torch.all(_tan(si.t) == 0)
            d2 = fwAD.make_dual(ray.d, torch.randn((3, n), device="cuda"))
            si = shape.ray_intersect(hf.Ray3f(ray.o, d2, ray.maxt), De)
            assert bool((_tan(si.t)[hit] != 0).all())
        finally:
            shape.heightfield = h0


# ---- 5. end-to-end derivative image ----------------------------------------------------------------------------

def _render(hf, shape, ray, pos, fw, lights_dir, lights_pt, weight):
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    a = hf.direct_lighting(si, ray, lights_dir, albedo=0.8, spp=1, weight=weight)
    b = hf.point_lighting(si, ray, lights_pt, albedo=0.8, spp=1)
    return hf.film_gaussian(torch.cat([a, b]), pos, fw, fw)


def test_derivative_image_equals_reverse_mode_transpose(hf):
    N, fw = 256, 96
    h = hf.workload.sine_heights(N, N, device="cuda")
    shape = hf.Heightfield(heightfield=h, max_height=0.5)
    rays = hf.workload.ortho_rays(fw, fw, 1, "cuda")
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    pos = hf.workload.film_positions(fw, fw, 1, "cuda")
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    weight = 0.5 + torch.rand(len(ray), device="cuda", generator=g)
    Ld = torch.tensor([[0.3, 0.2, 0.93, 2.0], [-0.5, 0.1, 0.86, 1.0]])
    Ld[:, :3] /= Ld[:, :3].norm(dim=1, keepdim=True)
    Lp = torch.tensor([[0.5, -0.3, 1.5, 3.0]])
    dh = torch.randn((N, N), device="cuda", generator=g)
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(h, dh)
        film = _render(hf, shape, ray, pos, fw, Ld, Lp, weight)
        dfilm = _tan(film).clone()
        primal = fwAD.unpack_dual(film).primal.clone()
    shape.heightfield = h.clone().requires_grad_(True)
    film_r = _render(hf, shape, ray, pos, fw, Ld, Lp, weight)
    assert torch.allclose(film_r.detach(), primal, rtol=1e-5, atol=1e-6)   # (the splat accumulates with atomics)
    Wt = torch.randn(film_r.shape, device="cuda", generator=g)
    (film_r * Wt).sum().backward()
    lhs = float((dfilm.double() * Wt.double()).sum())
    rhs = float((dh.double() * shape.heightfield.grad.double()).sum())
    scale = float((dfilm.double() * Wt.double()).abs().sum())
    assert float(dfilm.abs().sum()) > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("spp", [1, 4, 3])
def test_lighting_tangents_against_float64_formulas(hf, spp):
    n = 64 * 7 * spp
    g = torch.Generator(device="cuda"); g.manual_seed(spp)
    sh_n = torch.randn((3, n), device="cuda", generator=g); sh_n /= sh_n.norm(dim=0, keepdim=True)
    sh_n[2] = sh_n[2].abs()
    d = torch.randn((3, n), device="cuda", generator=g); d[2] = -d[2].abs() - 0.2
    t = torch.rand(n, device="cuda", generator=g); t[::11] = math.inf
    p = torch.randn((3, n), device="cuda", generator=g) * 0.3
    weight = 0.5 + torch.rand(n, device="cuda", generator=g)
    vis = (torch.rand((2, n), device="cuda", generator=g) > 0.2).to(torch.uint8)
    dn, dp, dw = (torch.randn((3, n), device="cuda", generator=g), torch.randn((3, n), device="cuda", generator=g),
                  torch.randn(n, device="cuda", generator=g))
    Ld = torch.tensor([[0.3, 0.2, 0.93, 2.0], [-0.5, 0.1, 0.86, 1.0]]); Ld[:, :3] /= Ld[:, :3].norm(dim=1, keepdim=True)
    Lp = torch.tensor([[0.5, -0.3, 1.5, 3.0], [-1.0, 0.4, 0.8, 1.5]])
    si = hf.SurfaceInteraction3f()
    ray = hf.Ray3f(torch.zeros((3, n), device="cuda"), d)
    with fwAD.dual_level():
        si.sh_frame = hf.Frame3f(None, None, fwAD.make_dual(sh_n, dn)); si.t = t; si.p = fwAD.make_dual(p, dp)
        img_d = _tan(hf.direct_lighting(si, ray, Ld, albedo=0.7, spp=spp, vis=vis, weight=fwAD.make_dual(weight, dw))).cpu().numpy()
        img_p = _tan(hf.point_lighting(si, ray, Lp, albedo=0.7, spp=spp, vis=vis)).cpu().numpy()
    N, D, T, P = (x.cpu().numpy().astype(np.float64) for x in (sh_n, d, t, p))
    dN, dP, dW, Wg = (x.cpu().numpy().astype(np.float64) for x in (dn, dp, dw, weight))
    V = vis.cpu().numpy() != 0
    lit = np.isfinite(T) & ((-(N * D).sum(0)) > 0)
    ref_d = np.zeros((2, n // spp)); ref_p = np.zeros((2, n // spp))
    for k in range(2):
        l = Ld[k, :3].numpy().astype(np.float64)[:, None]
        co = (N * l).sum(0)
        on = lit & (co > 0) & V[k]
        val = 0.7 / math.pi * float(Ld[k, 3]) * (Wg * (dN * l).sum(0) + co * dW)
        ref_d[k] = np.where(on, val, 0).reshape(-1, spp).mean(1)
        v = Lp[k, :3].numpy().astype(np.float64)[:, None] - P
        r = np.linalg.norm(v, axis=0); lp = v / r
        co = (N * lp).sum(0)
        on = lit & (co > 0) & V[k]
        val = 0.7 / math.pi * float(Lp[k, 3]) / r ** 2 * ((dN * lp).sum(0) + (3 * co * (lp * dP).sum(0) - (N * dP).sum(0)) / r)
        ref_p[k] = np.where(on, val, 0).reshape(-1, spp).mean(1)
    assert np.allclose(img_d, ref_d, rtol=1e-4, atol=1e-5 * np.abs(ref_d).max())
    assert np.allclose(img_p, ref_p, rtol=1e-4, atol=1e-5 * np.abs(ref_p).max())


# ---- 6. graph capture ------------------------------------------------------------------------------------------

def test_tangent_captured_in_a_graph_equals_eager(hf):
    rng, shape, ray = _small(hf, n=4096)
    n = len(ray)
    pi = shape.ray_intersect_preliminary(ray)
    dh = torch.randn((shape.height, shape.width), device="cuda")
    do = torch.randn((3, n), device="cuda"); dd = torch.randn((3, n), device="cuda")
    eager = shape.tangent(ray, pi, dh, do, dd)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        shape.tangent(ray, pi, dh, do, dd)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = shape.tangent(ray, pi, dh, do, dd)
    out.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    dh.mul_(2.0)   # the replay reads the tangent buffers where they are
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, shape.tangent(ray, pi, dh, do, dd))

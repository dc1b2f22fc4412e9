"""eval_parameterization (hf_eval_parameterization and its adjoint / tangent) on the GPU, against the float64
restatement tests/param_ref.py and against the library's own surface interaction:
  * the reference's known answers (test_mesh.py test09, test_rectangle.py test09) and p under an affine to_world;
  * the lookup: out_prim_index and b bit for bit on grids up to 4096^2, borders, diagonals, corners, signed zeros,
    one ulp outside, NaN and inactive lanes (the miss record);
  * the record, every field bitwise hf_compute_surface_interaction's on the UV-space rays for every RayFlags set,
    flat and smooth, flipped or not, under three transforms, and within 1e-5 of the restatement;
  * the adjoint against hf_adjoint(FollowShape) and float64 autograd, grad_to_world bitwise repeatable; the tangent
    against hf_tangent(FollowShape), the transpose identity, repeatability;
  * cross-feature identities: the area Jacobian of area.cpp against hf_surface_area, a (u, v, 0) vertex attribute
    gives the query back, traced hits map back to their triangle;
  * the Python mirror: backward, forward_ad and a captured forward + adjoint.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import common
import param_ref as R
from si_numpy import FLAG_SUBSETS, RAY_ALL, RAY_BOUNDARYTEST, RAY_DETACHSHAPE, RAY_DPDUV, RAY_FOLLOWSHAPE, RAY_MINIMAL, RAY_UV

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ALL_EDGES = 0x10000
MIRROR_SHEAR = np.array([[-1.2, 0.3, 0.1, 0.4], [0.0, 0.9, -0.2, -0.3], [0.2, 0.1, 0.7, 1.1]], np.float32)


def _tw(kind):
    return {"identity": np.eye(4, dtype=np.float32)[:3], "affine": common.affine(5), "mirror": MIRROR_SHEAR}[kind]


def _field(hf, W, H, kind="rand", flip=False, tw="identity", smooth=False, seed=0, s=0.6, **kw):
    rng = np.random.default_rng(seed + 7 * W + H)
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32) if kind == "rand" else common.heights(kind, W, H, rng)
    T = _tw(tw) if isinstance(tw, str) else np.asarray(tw, np.float32)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=s, flip_normals=flip,
                           to_world=torch.from_numpy(T), face_normals=not smooth, **kw)
    return shape, h, s, T.astype(np.float64)


def _uvp(uv):
    n = uv.shape[1]
    return (C.c_void_p * 2)(uv.data_ptr(), uv.data_ptr() + 4 * n)


def _rows28(n, fill=0.0):
    buf = torch.full((28, n), fill, dtype=torch.float32, device=DEV)
    from hf_amd import shape as sh
    out = sh._fill(sh._fill(sh.hf_si_t(), sh._DIFF_ROWS, sh._rows(buf[:18], n)), sh._AUX_ROWS, sh._rows(buf[18:], n))
    return buf, out


def _param(shape, uv, flags, active=None):
    """[28, n] record (18 differentiable rows, then boundary_test, sh_s, sh_t, wi) and prim_index"""
    from hf_amd import _capi
    n = uv.shape[1]
    buf, out = _rows28(n)
    prim = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    ap = active.data_ptr() if active is not None else None
    _capi.check(_capi.lib().hf_eval_parameterization(shape._h, n, C.byref(_uvp(uv)), flags, ap, C.byref(out),
                                                     prim.data_ptr(), shape._stream()))
    return buf, prim


def _synth(uv, prim, b):
    """the UV-space rays and pi = {1, b, prim} of the valid queries"""
    n = uv.shape[1]
    o = torch.stack([uv[0], uv[1], -torch.ones_like(uv[0])]).contiguous()
    d = torch.zeros((3, n), device=DEV)
    d[2] = 1.0
    maxt = torch.full((n,), math.inf, device=DEV)
    t = torch.ones(n, device=DEV)
    return o, d, maxt, t, b.contiguous(), prim.contiguous()


def _csi(shape, uv, prim, b, flags):
    from hf_amd import _capi
    n = uv.shape[1]
    o, d, maxt, t, bb, pp = _synth(uv, prim, b)
    buf, out = _rows28(n)
    rays = shape._rays_struct(o, d, maxt)
    pis = shape._pi_struct(t, bb, pp)
    f = flags & ~RAY_FOLLOWSHAPE
    if f & RAY_BOUNDARYTEST:
        f |= ALL_EDGES
    _capi.check(_capi.lib().hf_compute_surface_interaction(shape._h, n, C.byref(rays), C.byref(pis), f, None, C.byref(out),
                                                           shape._stream()))
    return buf


def _random_uv(n, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (lo + (hi - lo) * torch.rand((2, n), generator=g, dtype=torch.float32, device=DEV)).contiguous()


# ---- 1. known answers -------------------------------------------------------------------------------------------

def test_known_answers_on_the_device(hf):
    shape = hf.Heightfield(heightfield=torch.zeros((2, 2), device=DEV), max_height=1.0)
    uv = torch.tensor([[-0.01, 1 - 1e-7, 1e-7, 0.2], [0.5, 1 - 1e-7, 1e-7, 0.3]], dtype=torch.float32, device=DEV)
    si = shape.eval_parameterization(uv)
    assert si.is_valid().tolist() == [False, True, True, True]
    expect = torch.tensor([[1, 1, 0], [-1, -1, 0], [-0.6, -0.4, 0]], dtype=torch.float32, device=DEV).T
    assert torch.allclose(si.p[:, 1:], expect, atol=1e-6), si.p
    assert torch.allclose(si.uv[:, 1:], uv[:, 1:], atol=1e-7)
    assert torch.all(si.t[1:] == 1.0) and si.t[0] == math.inf
    assert torch.all(si.n[:, 1:] == torch.tensor([[0.0], [0.0], [1.0]], device=DEV))
    # test_rectangle.py test09: uv does not move with to_world; p moves as the object point does
    uv = _random_uv(256, 3)
    for kind in ("affine", "mirror"):
        T = _tw(kind)
        moved = hf.Heightfield(heightfield=torch.zeros((2, 2), device=DEV), max_height=1.0, to_world=torch.from_numpy(T))
        sm = moved.eval_parameterization(uv)
        assert torch.allclose(sm.uv, uv, atol=1e-7) and torch.allclose(sm.uv, shape.eval_parameterization(uv).uv, atol=1e-7)
        q = torch.stack([2 * uv[0].double() - 1, 2 * uv[1].double() - 1, torch.zeros_like(uv[0]).double()])
        A = torch.from_numpy(T.astype(np.float64)).to(DEV)
        p = A[:, :3] @ q + A[:, 3:4]
        assert float((sm.p.double() - p).abs().max()) <= 2e-6, kind


# ---- 2. the lookup ----------------------------------------------------------------------------------------------

def _special_uv(W, H):
    """exact borders, diagonals and corners of the grid, signed zeros, one ulp outside, NaN"""
    one_up, zero_dn = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(0), np.float32(-1))
    ed = np.array([0.0, 1.0, -0.0, one_up, zero_dn, np.nan, 0.5], np.float32)
    uu, vv = np.meshgrid(ed, ed)
    pts = [uu.ravel(), vv.ravel()]
    cw, ch = W - 1, H - 1
    if cw <= 64 and ch <= 64:
        j, i = np.meshgrid(np.arange(W), np.arange(H))
        a = np.float32(0.25)
        cu = (j.ravel() / np.float32(cw)).astype(np.float32)
        cv = (i.ravel() / np.float32(ch)).astype(np.float32)
        pts[0] = np.concatenate([pts[0], cu, np.clip(cu + a / cw, 0, 1), cu])
        pts[1] = np.concatenate([pts[1], cv, cv, np.clip(cv + (1 - a) / ch, 0, 1)])
    return np.stack(pts).astype(np.float32)


@pytest.mark.parametrize("grid", [(2, 2), (9, 7), (257, 257), (4096, 4096)])
def test_lookup_bitwise_and_the_miss_record(hf, grid):
    W, H = grid
    shape, h, s, T = _field(hf, W, H, "flat" if W > 300 else "rand")
    rnd = _random_uv(1 << 16, W).cpu().numpy()
    spec = _special_uv(W, H)
    uvn = np.concatenate([rnd, spec], 1)
    n = uvn.shape[1]
    act = np.ones(n, bool)
    act[::97] = False
    uv = torch.from_numpy(uvn).to(DEV)
    buf, prim = _param(shape, uv, RAY_MINIMAL, torch.from_numpy(act.astype(np.uint8)).to(DEV))
    valid, rprim, b1, b2 = R.lookup(uvn[0], uvn[1], W, H, act)
    got = prim.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, rprim)
    b = buf[7:9].cpu().numpy()   # without UV / dPdUV, uv is (b1, b2)
    assert np.array_equal(b[0][valid], b1[valid]) and np.array_equal(b[1][valid], b2[valid])
    assert np.array_equal(np.isfinite(buf[0].cpu().numpy()), valid)
    inv = torch.from_numpy(~valid).to(DEV)
    assert torch.all(buf[0][inv] == math.inf)
    assert torch.all(buf[1:, inv] == 0)           # every other row, wi included
    assert torch.all(buf[0][~inv] == 1.0)


# ---- 3. the record --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [False, True])
def test_record_bitwise_against_compute_surface_interaction(hf, smooth):
    W, H = 9, 7
    uv = torch.cat([_random_uv(2048, 11), torch.from_numpy(_special_uv(W, H)).to(DEV)], 1)
    uvn = uv.cpu().numpy()
    valid, rprim, b1, b2 = R.lookup(uvn[0], uvn[1], W, H)
    vm = torch.from_numpy(valid).to(DEV)
    flag_sets = [f | bt for f in FLAG_SUBSETS + [RAY_MINIMAL] for bt in (0, RAY_BOUNDARYTEST)] + [RAY_ALL | RAY_FOLLOWSHAPE]
    for flip in (False, True):
        for tw in ("identity", "affine", "mirror"):
            shape, h, s, T = _field(hf, W, H, flip=flip, tw=tw, smooth=smooth, seed=4)
            hd = torch.from_numpy(h).double()
            for flags in flag_sets:
                rec, prim = _param(shape, uv, flags)
                assert torch.equal(prim.cpu().long(), torch.from_numpy(rprim))
                ref = _csi(shape, uv[:, vm], prim[vm], torch.from_numpy(np.stack([b1, b2])[:, valid]).to(DEV), flags)
                got = rec[:, vm]
                same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
                assert bool(same.all()), (flip, tw, hex(flags), torch.nonzero(~same)[:4].tolist())
                r = R.record(hd, s, T, flip, uvn[0][valid], uvn[1][valid], rprim[valid], b1[valid], b2[valid],
                             flags & ~RAY_FOLLOWSHAPE, smooth)
                blk = R.block(r).float().to(DEV)
                err = (got[:18] - blk).abs().max()
                assert float(err) <= 1e-5 * max(1.0, float(blk.abs().max())), (flip, tw, hex(flags), float(err))


# ---- 4. adjoint and tangent -----------------------------------------------------------------------------------

def _grads(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((18, n), generator=g, dtype=torch.float32, device=DEV)


def _adjoint(shape, uv, flags, g, with_tw=False):
    from hf_amd import _capi
    from hf_amd import shape as sh
    n = uv.shape[1]
    gh = torch.zeros((shape.height, shape.width), device=DEV)
    gtw = torch.zeros(12, device=DEV) if with_tw else None
    gs = sh._fill(sh.hf_si_grad_t(), sh._DIFF_ROWS, sh._rows(g, n))
    _capi.check(_capi.lib().hf_eval_parameterization_adjoint(shape._h, n, C.byref(_uvp(uv)), flags, None, C.byref(gs),
                                                             gh.data_ptr(), gtw.data_ptr() if with_tw else None,
                                                             shape._stream()))
    return gh, gtw


def _tangent(shape, uv, flags, dh, dtw=None):
    from hf_amd import _capi
    from hf_amd import shape as sh
    n = uv.shape[1]
    out = torch.full((18, n), 7.0, device=DEV)
    ts = sh._fill(sh.hf_si_tangent_t(), sh._DIFF_ROWS, sh._rows(out, n))
    _capi.check(_capi.lib().hf_eval_parameterization_tangent(shape._h, n, C.byref(_uvp(uv)), flags, None,
                                                             dh.data_ptr() if dh is not None else None,
                                                             dtw.data_ptr() if dtw is not None else None,
                                                             C.byref(ts), shape._stream()))
    return out


def _rel(a, b):
    return float(torch.linalg.norm((a - b).double()) / max(float(torch.linalg.norm(b.double())), 1e-30))


@pytest.mark.parametrize("smooth", [False, True])
def test_adjoint_against_hf_adjoint_and_float64(hf, smooth):
    W, H = 33, 21
    shape, h, s, T = _field(hf, W, H, tw="affine", smooth=smooth, seed=2, differentiable_to_world=True)
    uv = torch.cat([_random_uv(20000, 5), torch.from_numpy(_special_uv(W, H)).to(DEV)], 1)
    n = uv.shape[1]
    flags = RAY_ALL | (0x20 if smooth else 0)
    g = _grads(n, 6)
    uvn = uv.cpu().numpy()
    valid, rprim, b1, b2 = R.lookup(uvn[0], uvn[1], W, H)
    g[:, ~torch.from_numpy(valid).to(DEV)] = 0.0
    gh, gtw = _adjoint(shape, uv, flags, g, with_tw=True)
    # hf_adjoint(FollowShape) on the synthesized input, grad_si.t = NULL
    o, d, maxt, t, bb, pp = _synth(uv, torch.from_numpy(rprim).int().to(DEV), torch.from_numpy(np.stack([b1, b2])).to(DEV))
    t = torch.where(torch.from_numpy(valid).to(DEV), t, torch.full_like(t, math.inf))
    g0 = g.clone()
    g0[0] = 0.0
    ray = hf.Ray3f(o, d, maxt)
    pi = hf.PreliminaryIntersection3f(t, bb, pp, shape)
    gtw_ref = torch.zeros(12, device=DEV)
    gh_ref = shape.adjoint(ray, pi, g0, flags | RAY_FOLLOWSHAPE, grad_to_world=gtw_ref)
    assert _rel(gh, gh_ref) <= 1e-6 and _rel(gtw, gtw_ref) <= 1e-6
    # bitwise repeatable transform gradient
    _, gtw2 = _adjoint(shape, uv, flags, g, with_tw=True)
    assert torch.equal(gtw, gtw2)
    # float64 autograd of the restatement (t and uv carry no derivative)
    hd = torch.from_numpy(h).double().requires_grad_(True)
    td = torch.from_numpy(T).requires_grad_(True)
    r = R.record(hd, s, td, False, uvn[0][valid], uvn[1][valid], rprim[valid], b1[valid], b2[valid], flags, smooth)
    gv = g[:, torch.from_numpy(valid).to(DEV)].double().cpu()
    gv[0] = 0.0
    gv[7:9] = 0.0
    (R.block(r) * gv).sum().backward()
    assert _rel(gh.cpu(), hd.grad) <= 2e-4 and _rel(gtw.cpu().reshape(3, 4), td.grad) <= 2e-4
    # DetachShape: nothing
    gd, gtd = _adjoint(shape, uv, flags | RAY_DETACHSHAPE, g, with_tw=True)
    assert torch.all(gd == 0) and torch.all(gtd == 0)


@pytest.mark.parametrize("smooth", [False, True])
def test_tangent_against_hf_tangent_and_repeatable(hf, smooth):
    W, H = 33, 21
    shape, h, s, T = _field(hf, W, H, tw="mirror", smooth=smooth, seed=3)
    uv = torch.cat([_random_uv(20000, 8), torch.from_numpy(_special_uv(W, H)).to(DEV)], 1)
    flags = RAY_ALL | (0x20 if smooth else 0)
    dh = torch.randn((H, W), generator=torch.Generator(device="cpu").manual_seed(9)).to(DEV)
    dtw = torch.randn(12, generator=torch.Generator(device="cpu").manual_seed(10)).to(DEV)
    out = _tangent(shape, uv, flags, dh, dtw)
    assert torch.equal(out, _tangent(shape, uv, flags, dh, dtw))
    uvn = uv.cpu().numpy()
    valid, rprim, b1, b2 = R.lookup(uvn[0], uvn[1], W, H)
    vm = torch.from_numpy(valid).to(DEV)
    o, d, maxt, t, bb, pp = _synth(uv, torch.from_numpy(rprim).int().to(DEV), torch.from_numpy(np.stack([b1, b2])).to(DEV))
    t = torch.where(vm, t, torch.full_like(t, math.inf))
    ref = shape.tangent(hf.Ray3f(o, d, maxt), hf.PreliminaryIntersection3f(t, bb, pp, shape), dh, ray_flags=flags | RAY_FOLLOWSHAPE,
                        d_to_world=dtw)
    assert torch.all(out[0] == 0) and torch.all(out[7:9] == 0)
    assert torch.equal(out[1:7], ref[1:7]) and torch.equal(out[9:], ref[9:])
    assert torch.all(out[:, ~vm] == 0)


@pytest.mark.parametrize("grid,n", [((257, 257), 1 << 18), ((4096, 4096), 1 << 24)])
def test_transpose_identity(hf, grid, n):
    W, H = grid
    for smooth in (False, True):
        shape, h, s, T = _field(hf, W, H, "sine", tw="affine", smooth=smooth, seed=1)
        uv = _random_uv(n, 12)
        flags = RAY_ALL | (0x20 if smooth else 0)
        ybar = _grads(n, 13)
        ybar[0] = 0.0
        ybar[7:9] = 0.0
        delta = torch.randn((H, W), generator=torch.Generator(device="cpu").manual_seed(14)).to(DEV)
        jd = _tangent(shape, uv, flags, delta)
        lhs = float((ybar.double() * jd.double()).sum())
        gh, _ = _adjoint(shape, uv, flags, ybar)
        rhs = float((gh.double() * delta.double()).sum())
        assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), 1.0), (grid, smooth, lhs, rhs)
        del jd, ybar, gh
        torch.cuda.empty_cache()


# ---- 5. cross-feature identities ------------------------------------------------------------------------------

def test_area_jacobian_equals_surface_area(hf):
    W, H = 17, 12
    shape, h, s, T = _field(hf, W, H, tw="affine", seed=5)
    cx, cy = np.meshgrid(np.arange(W - 1), np.arange(H - 1))
    cx, cy = cx.ravel().astype(np.float64), cy.ravel().astype(np.float64)
    u = np.concatenate([(cx + 1 / 3) / (W - 1), (cx + 2 / 3) / (W - 1)])
    v = np.concatenate([(cy + 1 / 3) / (H - 1), (cy + 2 / 3) / (H - 1)])
    uv = torch.from_numpy(np.stack([u, v]).astype(np.float32)).to(DEV)
    rec, prim = _param(shape, uv, RAY_ALL)
    assert len(set(prim.cpu().tolist())) == 2 * (W - 1) * (H - 1)
    jac = torch.linalg.cross(rec[12:15].double(), rec[15:18].double(), dim=0).norm(dim=0).sum()
    area = float(jac) / (2 * (W - 1) * (H - 1))
    assert abs(area - shape.surface_area()) <= 1e-5 * area


def test_vertex_attribute_gives_the_query_back(hf):
    W, H = 23, 15
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    tex = np.stack([j / (W - 1.0), i / (H - 1.0), np.zeros_like(j, dtype=np.float64)], -1).astype(np.float32)
    shape, h, s, T = _field(hf, W, H, tw="affine", seed=6, vertex_uvw=torch.from_numpy(tex))
    uv = _random_uv(50000, 15)
    si = shape.eval_parameterization(uv)
    val = shape.eval_attribute_3("vertex_uvw", si)
    assert float((val[0:2] - uv).abs().max()) <= 1e-6 and float(val[2].abs().max()) <= 1e-6


def test_traced_hits_map_back(hf):
    W, H = 65, 49
    shape, h, s, T = _field(hf, W, H, "sine", tw="affine", seed=7)
    rays = common.to_world_rays(common.random_rays(1 << 16, np.random.default_rng(3)), T)
    r = torch.from_numpy(rays).to(DEV)
    ray = hf.Ray3f(r[0:3].contiguous(), r[3:6].contiguous(), r[6].contiguous())
    si = shape.ray_intersect(ray, RAY_ALL)
    hit = si.is_valid()
    assert int(hit.sum()) > 10000
    uv = si.uv[:, hit].contiguous()
    back = shape.eval_parameterization(uv)
    uvn = uv.cpu().numpy().astype(np.float64)
    fx, fy = uvn[0] * (W - 1) % 1.0, uvn[1] * (H - 1) % 1.0
    far = (np.minimum(fx, 1 - fx) > 1e-6) & (np.minimum(fy, 1 - fy) > 1e-6) & (np.abs(fx + fy - 1) > 1e-6)
    far = torch.from_numpy(far).to(DEV)
    assert torch.equal(back.prim_index[far], si.prim_index[hit][far])
    # "a cell": the longest world-space edge of the grid's triangles
    P = np.einsum("rc,ijc->ijr", T[:, :3], np.stack(list(np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H))) + [h * s], -1)) \
        + T[:, 3]
    cell = max(np.linalg.norm(np.diff(P, axis=0), axis=-1).max(), np.linalg.norm(np.diff(P, axis=1), axis=-1).max(),
               np.linalg.norm(P[1:, :-1] - P[:-1, 1:], axis=-1).max())
    assert float((back.p - si.p[:, hit]).norm(dim=0).max()) <= 1e-5 * cell


# ---- 6. the Python mirror ----------------------------------------------------------------------------------------

def test_python_backward_forward_ad_and_capture(hf):
    W, H = 40, 30
    shape, h, s, T = _field(hf, W, H, tw="affine", seed=8, smooth=True)
    uv = _random_uv(30000, 16, -0.05, 1.05)
    flags = RAY_ALL | 0x20
    g = _grads(30000, 17)
    # backward() = the explicit adjoint
    shape.heightfield.requires_grad_(True)
    si = shape.eval_parameterization(uv, flags)
    loss = (si.p * g[1:4]).sum() + (si.n * g[4:7]).sum() + (si.sh_frame.n * g[9:12]).sum() \
        + (si.dp_du * g[12:15]).sum() + (si.dp_dv * g[15:18]).sum()
    loss.backward()
    gsel = g.clone()
    gsel[0] = 0.0
    gsel[7:9] = 0.0
    ref = shape.eval_parameterization_adjoint(uv, gsel, flags)
    assert _rel(shape.heightfield.grad, ref) <= 1e-6
    # forward_ad = the tangent
    dh = torch.randn((H, W), generator=torch.Generator(device="cpu").manual_seed(18)).to(DEV)
    shape.heightfield.requires_grad_(False)
    shape.heightfield.grad = None
    h0 = shape.heightfield
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(h0, dh)
        si = shape.eval_parameterization(uv, flags)
        tp = fwAD.unpack_dual(si.p).tangent
    shape.heightfield = h0
    ref = shape.eval_parameterization_tangent(uv, dh, flags)
    assert torch.equal(tp, ref[1:4])
    # a captured forward + adjoint replays to eager
    from hf_amd import _capi
    from hf_amd import shape as sh
    n = uv.shape[1]
    buf, out = _rows28(n)
    prim = torch.empty(n, dtype=torch.int32, device=DEV)
    gh = torch.zeros((H, W), device=DEV)
    gs = sh._fill(sh.hf_si_grad_t(), sh._DIFF_ROWS, sh._rows(gsel, n))
    uvp = _uvp(uv)
    lib = _capi.lib()

    def step(stream):
        _capi.check(lib.hf_eval_parameterization(shape._h, n, C.byref(uvp), flags, None, C.byref(out), prim.data_ptr(), stream))
        gh.zero_()
        _capi.check(lib.hf_eval_parameterization_adjoint(shape._h, n, C.byref(uvp), flags, None, C.byref(gs),
                                                         gh.data_ptr(), None, stream))
    step(torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    eager = (buf.clone(), prim.clone(), gh.clone())
    s_ = torch.cuda.Stream(DEV)
    s_.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s_):
        step(s_.cuda_stream)
    torch.cuda.current_stream(DEV).wait_stream(s_)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step(torch.cuda.current_stream(DEV).cuda_stream)
    buf.zero_(); prim.zero_(); gh.zero_()
    torch.cuda.synchronize()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager[0]) and torch.equal(prim, eager[1]) and _rel(gh, eager[2]) <= 1e-6
    # a parameter change between forward and backward is refused
    shape.heightfield.requires_grad_(True)
    si = shape.eval_parameterization(uv, flags)
    shape.parameters_changed(["heightfield"])
    with pytest.raises(RuntimeError, match="changed between forward and backward"):
        si.p.sum().backward()

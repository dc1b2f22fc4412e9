"""Area sampling (hf_set_area_sampling, hf_sample_position and its derivatives) on the GPU, against the float64
restatement tests/area_ref.py:
  * the reference rectangle's known answers on the device, pdf_position = (float) (1 / sum);
  * the CDF against the sequential double sum, bitwise repeatable rebuilds;
  * index exactness against np.searchsorted on the device's CDF, and b, p, n, uv against the restatement;
  * the distribution: a chi-square test of the per-triangle counts, an area light's irradiance, pdf_direction;
  * reverse / forward mode against float64 autograd / torch.func.jvp, the transpose identity at 4096^2, the chain
    through sample_direction;
  * a captured [Adam step -> sample_position -> adjoint] step replays to the eager trajectory;
  * enabling and disabling the table changes nothing else; without it hf_sample_position is refused.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import area_ref as A
import common

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GRIDS = {"2x2": (2, 2, "rand"), "9x7": (9, 7, "rand"), "257": (257, 257, "sine")}


def _tw(kind):
    if kind == "identity":
        return np.eye(4, dtype=np.float32)[:3]
    return common.affine(5)   # rotation * anisotropic scale + translation


def _field(hf, W, H, kind, flip=False, tw="identity", smooth=False, seed=0, s=0.6):
    rng = np.random.default_rng(seed + W * 7 + H)
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32) if kind == "rand" else common.heights(kind, W, H, rng)
    T = _tw(tw)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=s, flip_normals=flip,
                           to_world=torch.from_numpy(T), face_normals=not smooth)
    return shape, h, s, T.astype(np.float64)


def _table(shape, h, s, tw):
    """device CDF, its scalars, and the restatement's areas / CDF"""
    area, norm = shape._area_scalars()
    cdf = shape.area_cdf().cpu().numpy()
    a64 = A.areas(torch.from_numpy(h).double().to(DEV), s, tw, device_rounding=True).cpu().numpy()
    return cdf, np.float32(area), np.float32(norm), a64


def _samples(n, seed, extra=()):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand((2, n), generator=g, dtype=torch.float32)
    if extra:
        k = len(extra)
        x[1, :k] = torch.tensor(extra, dtype=torch.float32)
    return x.to(DEV)


# ---- 1. known answers -------------------------------------------------------------------------------------------

def test_known_answers_on_the_device(hf):
    h = torch.full((4, 5), 0.5, device=DEV)
    cases = [(np.eye(4)[:3], 4.0), (np.diag([2.0, 2.0, 1.0, 1.0])[:3], 16.0),
             (np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0]], np.float64), 4.0 * math.sqrt(2.0)),
             (np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64), 4.0)]
    for sx in (1, 2, 4):
        tw = np.diag([sx, 2.5, 1.0, 1.0])[:3].copy(); tw[:, 3] = (1.3, -3.0, 5.0)
        cases.append((tw, 4.0 * sx * 2.5))
    for tw, ref in cases:
        shape = hf.Heightfield(heightfield=h, max_height=0.7, to_world=torch.from_numpy(tw))
        area = shape.surface_area()
        assert abs(area - ref) <= 2e-6 * ref, (tw, area, ref)
        ps = shape.sample_position(0.0, _samples(64, 1))
        pdf = shape.pdf_position(ps)
        _, norm = shape._area_scalars()
        assert torch.all(ps.pdf == norm) and torch.all(pdf == norm)
        assert abs(norm * area - 1.0) <= 3e-7   # (float) (1 / sum) with sum the double behind (float) sum


# ---- 2. the CDF -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,tw", [(g, t) for g in GRIDS for t in ("identity", "affine")] + [("4096", "identity")])
def test_cdf_against_the_sequential_double_sum(hf, grid, tw):
    if grid == "4096":   # the bench field
        h = hf.workload.sine_heights(4096, 4096, device=DEV)
        shape = hf.Heightfield(heightfield=h, max_height=0.5)
        hn, s, T = h.cpu().numpy(), 0.5, np.eye(4)[:3]
    else:
        W, H, kind = GRIDS[grid]
        shape, hn, s, T = _field(hf, W, H, kind, tw=tw)
    cdf, area, norm, a64 = _table(shape, hn, s, T)
    run = np.cumsum(a64)
    assert cdf.shape == a64.shape
    assert np.all(np.diff(cdf) >= 0), "the device CDF must be sorted"
    rel = np.abs(cdf.astype(np.float64) - run) / run
    assert rel.max() <= 2e-6, rel.max()
    if grid in ("2x2", "9x7"):
        # a few float32 ulps: the device's areas are float32 arithmetic, the restatement's float64
        ulp = np.spacing(run.astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(cdf.astype(np.float64) - run) <= 4 * ulp), (np.abs(cdf - run) / ulp).max()
    assert abs(float(area) - run[-1]) <= 1e-6 * run[-1]
    assert cdf[-1] == area
    # a rebuild of the same heights is bitwise the same table
    shape.parameters_changed(["heightfield"])
    assert np.array_equal(shape.area_cdf().cpu().numpy(), cdf)


# ---- 3. index exactness -----------------------------------------------------------------------------------------

def _check_samples(shape, h, s, T, flip, smooth, n, seed):
    cdf, area, norm, a64 = _table(shape, h, s, T)
    valid = (int(np.nonzero(a64 > 0)[0][0]), int(np.nonzero(a64 > 0)[0][-1]))
    edge = [0.0, 1.0 - 2.0 ** -24] + [float(v) / float(area) for v in cdf[:: max(1, len(cdf) // 64)]]
    smp = _samples(n, seed, extra=edge)
    # values that land exactly on table entries: y with y * sum == cdf[i] in float32
    y = smp[1].cpu().numpy()
    ps = shape.sample_position(0.0, smp)
    idx = ps.prim_index.cpu().numpy().astype(np.int64)
    ref = A.sample_index(cdf, area, valid, y)
    assert np.array_equal(idx, ref), int((idx != ref).sum())
    # with the index fixed: b, p, n, uv against the restatement
    pmf32 = a64.astype(np.float32)
    reused = A.reuse(cdf, pmf32, norm, idx, y)
    bx, by = A.warp(smp[0].cpu().numpy(), reused)
    b = ps.b.cpu().numpy()
    assert np.allclose(b[0], bx, rtol=0, atol=2e-6) and np.allclose(b[1], by, rtol=0, atol=2e-5)
    hd = torch.from_numpy(h).double().to(DEV)
    bt = torch.from_numpy(b).double().to(DEV)
    p, nn, uv = A.position(hd, s, T, flip, ps.prim_index.long(), bt[0], bt[1], smooth, device_rounding=True)
    scale = float(p.abs().max())
    assert float((ps.p.T.double() - p).abs().max()) <= 1e-5 * scale
    assert float((ps.n.T.double() - nn).abs().max()) <= 1e-5
    assert float((ps.uv.T.double() - uv).abs().max()) <= 1e-5
    return ps


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("tw", ["identity", "affine"])
def test_index_and_sample_against_restatement(hf, grid, smooth, flip, tw):
    W, H, kind = GRIDS[grid]
    shape, h, s, T = _field(hf, W, H, kind, flip=flip, tw=tw, smooth=smooth)
    _check_samples(shape, h, s, T, flip, smooth, 1 << 20 if grid == "257" else 1 << 16, seed=W + int(flip) + 2 * int(smooth))


def test_index_exactness_on_the_bench_field(hf):
    h = hf.workload.sine_heights(4096, 4096, device=DEV)
    shape = hf.Heightfield(heightfield=h, max_height=0.5)
    _check_samples(shape, h.cpu().numpy(), 0.5, np.eye(4)[:3], False, False, 1 << 20, seed=11)


# ---- 4. the distribution ----------------------------------------------------------------------------------------

def test_chi_square_of_triangle_counts(hf):
    from scipy import stats
    shape, h, s, T = _field(hf, 9, 7, "rand", s=1.5)
    n = 1 << 22
    ps = shape.sample_position(0.0, _samples(n, 3))
    counts = torch.bincount(ps.prim_index.long(), minlength=2 * 8 * 6).cpu().numpy().astype(np.float64)
    a64 = A.areas(torch.from_numpy(h).double(), s, T).numpy()
    expected = n * a64 / a64.sum()
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    dof = len(a64) - 1
    p = stats.chi2.sf(chi2, dof)
    assert p > 1e-3, (chi2, dof, p)


def _irradiance_closed_form(h):
    X = 1.0 / h
    return 4.0 * X / math.sqrt(1 + X * X) * math.atan(X / math.sqrt(1 + X * X))


def test_area_light_irradiance_and_pdf_direction(hf):
    # a flat emitter [-1, 1]^2 at z = 0 (radiance 1), receiver at (0, 0, h) facing down
    hgt = 0.75
    # the closed form, confirmed by float64 quadrature of cos_r cos_e / r^2 over the square
    m = 2000
    u = (np.arange(m) + 0.5) / m * 2 - 1
    X, Y = np.meshgrid(u, u)
    r2 = X * X + Y * Y + hgt * hgt
    quad = float((hgt * hgt / r2 ** 2).sum() * (2.0 / m) ** 2)
    E = _irradiance_closed_form(hgt)
    assert abs(quad - E) <= 1e-5 * E
    shape = hf.Heightfield(heightfield=torch.zeros((17, 17), device=DEV), max_height=1.0)
    n = 1 << 24

    class It:
        pass
    it = It()
    it.p = torch.tensor([[0.0], [0.0], [hgt]], device=DEV).expand(3, n).contiguous()
    it.time = 0.0
    ds = shape.sample_direction(it, _samples(n, 5))
    cos_r = (-ds.d[2]).clamp(min=0)
    est = float((cos_r.double() / ds.pdf.double()).mean())
    assert abs(est - E) <= 1e-3 * E, (est, E)
    pdf = shape.pdf_direction(it, ds)
    assert torch.allclose(pdf, ds.pdf, rtol=1e-6, atol=0)


# ---- 5. adjoint and tangent -------------------------------------------------------------------------------------

def _ref_loss(hd, s, T, flip, smooth, ps, gp, gn):
    p, n, _ = A.position(hd, s, T, flip, ps.prim_index.long(), ps.b[0].double(), ps.b[1].double(), smooth)
    return (p * gp.T.double()).sum() + (n * gn.T.double()).sum()


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("tw", ["identity", "affine"])
def test_adjoint_and_tangent_against_float64(hf, smooth, flip, tw):
    shape, h, s, T = _field(hf, 9, 7, "rand", flip=flip, tw=tw, smooth=smooth)
    n = 4096
    ps = shape.sample_position(0.0, _samples(n, 7))
    g = torch.Generator(device="cpu").manual_seed(8)
    gp = torch.randn((3, n), generator=g).to(DEV)
    gn = torch.randn((3, n), generator=g).to(DEV)
    grad = shape.sample_position_adjoint(ps, gp, gn)
    hd = torch.from_numpy(h).double().to(DEV).requires_grad_(True)
    _ref_loss(hd, s, T, flip, smooth, ps, gp, gn).backward()
    ref = hd.grad
    assert float((grad.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    dh = torch.randn((7, 9), generator=g).to(DEV)
    dp, dn = shape.sample_position_tangent(ps, dh)

    def f(x):
        p, nn, _ = A.position(x, s, T, flip, ps.prim_index.long(), ps.b[0].double(), ps.b[1].double(), smooth)
        return p, nn
    _, (rp, rn) = torch.func.jvp(f, (torch.from_numpy(h).double().to(DEV),), (dh.double(),))
    assert float((dp.T.double() - rp).abs().max()) <= 1e-4 * float(rp.abs().max())
    assert float((dn.T.double() - rn).abs().max()) <= 1e-4 * float(rn.abs().max())
    # bitwise repeatable forward mode
    dp2, dn2 = shape.sample_position_tangent(ps, dh)
    assert torch.equal(dp, dp2) and torch.equal(dn, dn2)
    # autograd through the mirror: heightfield.grad from sample_position
    shape.heightfield.requires_grad_(True)
    ps2 = shape.sample_position(0.0, _samples(n, 7))
    ((ps2.p * gp).sum() + (ps2.n * gn).sum()).backward()
    assert float((shape.heightfield.grad.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("smooth", [False, True])
def test_transpose_identity_on_the_bench_field(hf, smooth):
    h = hf.workload.sine_heights(4096, 4096, device=DEV)
    shape = hf.Heightfield(heightfield=h, max_height=0.5, face_normals=not smooth)
    n = 1 << 26 if not smooth else 1 << 24
    ps = shape.sample_position(0.0, _samples(n, 9))
    g = torch.Generator(device=DEV).manual_seed(10)
    gp = torch.randn((3, n), generator=g, device=DEV)
    gn = torch.randn((3, n), generator=g, device=DEV)
    dh = torch.randn((4096, 4096), generator=g, device=DEV)
    grad = shape.sample_position_adjoint(ps, gp, gn)
    dp, dn = shape.sample_position_tangent(ps, dh)
    lhs = float((gp.double() * dp.double()).sum() + (gn.double() * dn.double()).sum())
    rhs = float((grad.double() * dh.double()).sum())
    # relative to the sum of the terms' magnitudes: the two sides are sums of 10^8 terms of either sign
    scale = float((gp.double() * dp.double()).abs().sum() + (gn.double() * dn.double()).abs().sum())
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)


def test_chain_through_sample_direction(hf):
    shape, h, s, T = _field(hf, 9, 7, "rand", tw="affine")
    n = 2048
    shape.heightfield.requires_grad_(True)
    g = torch.Generator(device="cpu").manual_seed(12)
    ref_p = (torch.randn((3, n), generator=g) * 0.3 + torch.tensor([[0.0], [0.0], [2.5]])).to(DEV).requires_grad_(True)

    class It:
        pass
    it = It(); it.p = ref_p; it.time = 0.0
    smp = _samples(n, 13)
    ds = shape.sample_direction(it, smp)
    w = torch.randn((3, n), generator=g).to(DEV)
    loss = (ds.d * w).sum() + ds.dist.sum() + (ds.pdf * 1e-3).sum()
    loss.backward()
    hd = torch.from_numpy(h).double().to(DEV).requires_grad_(True)
    rp = ref_p.detach().T.double().requires_grad_(True)
    p, nn, _ = A.position(hd, s, T, False, ds.prim_index.long(), ds.b[0].double(), ds.b[1].double(), False)
    d, dist, pdf = A.direction(rp, p, nn, float(shape._area_scalars()[1]))
    (((d * w.T.double()).sum() + dist.sum() + (pdf * 1e-3).sum())).backward()
    assert torch.allclose(ds.d.T.double(), d, atol=1e-5) and torch.allclose(ds.pdf.double(), pdf, rtol=1e-4)
    assert float((shape.heightfield.grad.double() - hd.grad).abs().max()) <= 1e-4 * float(hd.grad.abs().max())
    assert float((ref_p.grad.T.double() - rp.grad).abs().max()) <= 1e-4 * float(rp.grad.abs().max())


# ---- 6. capture -------------------------------------------------------------------------------------------------

def test_captured_adam_sample_adjoint_step_replays_to_eager(hf):
    from hf_amd import _capi
    lib = _capi.lib()
    N, n = 65, 1 << 16
    h0 = hf.workload.sine_heights(N, N, device=DEV)
    shape = hf.Heightfield(heightfield=h0.clone(), max_height=0.5)
    shape.ensure_pmf_built()
    smp = _samples(n, 14)
    out = torch.empty((11, n), device=DEV)
    prim = torch.empty(n, dtype=torch.int32, device=DEV)
    grad = torch.zeros((N, N), device=DEV)
    m, v = torch.zeros_like(grad), torch.zeros_like(grad)
    gsel = torch.zeros((6, n), device=DEV)
    gsel[2] = 1.0
    gsel[5] = 0.5
    lr_t = torch.tensor([lib.hf_adam_lr_t(1e-2, 0.9, 0.999, k + 1) for k in range(8)], device=DEV)
    step_ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    heights = shape.heightfield.detach()
    ps_s = _capi.hf_position_sample_t()
    rows = [out.data_ptr() + 4 * n * k for k in range(11)]
    for k in range(3):
        ps_s.p[k], ps_s.n[k] = rows[k], rows[3 + k]
    ps_s.uv[0], ps_s.uv[1], ps_s.pdf = rows[6], rows[7], rows[8]
    ps_s.prim_index = prim.data_ptr()
    ps_s.b[0], ps_s.b[1] = rows[9], rows[10]
    sp = (C.c_void_p * 2)(smp.data_ptr(), smp.data_ptr() + 4 * n)
    bp = (C.c_void_p * 2)(rows[9], rows[10])
    gp = (C.c_void_p * 3)(*[gsel.data_ptr() + 4 * n * k for k in range(3)])
    gn = (C.c_void_p * 3)(*[gsel.data_ptr() + 4 * n * k for k in range(3, 6)])

    def step(stream):
        _capi.check(lib.hf_adam_step_scheduled(shape._h, heights.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                               lr_t.data_ptr(), step_ctr.data_ptr(), 0.9, 0.999, 1e-8, 0, stream))
        _capi.check(lib.hf_sample_position(shape._h, n, C.byref(sp), None, C.byref(ps_s), stream))
        grad.zero_()
        _capi.check(lib.hf_sample_position_adjoint(shape._h, n, prim.data_ptr(), C.byref(bp), None, C.byref(gp),
                                                   C.byref(gn), grad.data_ptr(), stream))

    def reset():
        heights.copy_(h0); shape.parameters_changed(["heightfield"])
        m.zero_(); v.zero_(); step_ctr.zero_()
        grad.fill_(1e-3)
        torch.cuda.synchronize()
    cur = torch.cuda.current_stream(DEV).cuda_stream
    reset()
    step(cur); torch.cuda.synchronize()
    eager = [(heights.clone(), out.clone(), grad.clone())]
    reset()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):   # warm-up on a side stream before capture
        step(s.cuda_stream)
    torch.cuda.current_stream(DEV).wait_stream(s)
    torch.cuda.synchronize()
    reset()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step(torch.cuda.current_stream(DEV).cuda_stream)
    reset()
    state = (heights, m, v, step_ctr, grad)
    for k in range(3):
        # every replay against an eager step from the same state: the adjoint's float atomics add in any order, so the
        # gradient the next Adam step starts from is equal only up to rounding -- which Adam's normalised update
        # amplifies where the gradient is nearly zero; from one state everything but that sum is bitwise the same
        snap = [t.clone() for t in state]
        gr.replay(); torch.cuda.synchronize()
        rh, ro, rp, rg = heights.clone(), out.clone(), prim.clone(), grad.clone()
        for t, s_ in zip(state, snap):
            t.copy_(s_)
        step(cur); torch.cuda.synchronize()
        assert torch.equal(heights, rh) and torch.equal(out, ro) and torch.equal(prim, rp), k
        assert float((grad - rg).abs().max()) <= 1e-5 * float(rg.abs().max()), k
        if k == 0:   # the first step also equals the first step of the eager trajectory
            eh, eo, eg = eager[0]
            assert torch.equal(heights, eh) and torch.equal(out, eo)
    # the switch itself is not capturable
    s2 = torch.cuda.Stream(DEV)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s2):
        rc = lib.hf_set_area_sampling(shape._h, 0, s2.cuda_stream)
    assert rc == _capi.HF_EINVAL and b"not capturable" in lib.hf_last_error_string()


# ---- 7. no existing behaviour changes ---------------------------------------------------------------------------

def test_enable_disable_changes_nothing_else(hf):
    from hf_amd import _capi
    N = 129
    h = hf.workload.sine_heights(N, N, device=DEV)
    rays = hf.workload.ortho_rays(96, 96, 2, DEV)
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())

    def run(shape):
        si = shape.ray_intersect(ray, hf.RayFlags.All)
        pi = hf.PreliminaryIntersection3f(si.t, si.prim_uv, si.prim_index, shape)
        g = torch.ones((18, len(ray)), device=DEV)
        grad = shape.adjoint(ray, pi, g)
        tan = shape.tangent(ray, pi, dheights=torch.ones((N, N), device=DEV))
        return [si.t, si.p, si.n, si.sh_frame.n, si.uv, grad, tan, shape.mip(1)]
    for smooth in (False, True):
        a = hf.Heightfield(heightfield=h, max_height=0.5, face_normals=not smooth)
        base = run(a)
        b = hf.Heightfield(heightfield=h, max_height=0.5, face_normals=not smooth)
        b.ensure_pmf_built()
        b.parameters_changed(["heightfield"])
        with_table = run(b)
        _capi.check(_capi.lib().hf_set_area_sampling(b._h, 0, b._stream()))
        after = run(b)
        for k, (x, y, z) in enumerate(zip(base, with_table, after)):
            if k == 5:   # the adjoint's float atomics add in any order
                tol = 1e-6 * float(x.abs().max())
                assert float((x - y).abs().max()) <= tol and float((x - z).abs().max()) <= tol
            else:
                assert torch.equal(x.cpu(), y.cpu()) and torch.equal(x.cpu(), z.cpu()), k


def test_without_the_table_sampling_is_refused_and_inactive_lanes_are_zero(hf):
    from hf_amd import _capi
    lib = _capi.lib()
    shape = hf.Heightfield(heightfield=hf.workload.sine_heights(33, 33, device=DEV), max_height=0.5)
    n = 256
    smp = _samples(n, 15)
    out = torch.full((11, n), 7.0, device=DEV)
    prim = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    ps_s = _capi.hf_position_sample_t()
    rows = [out.data_ptr() + 4 * n * k for k in range(11)]
    for k in range(3):
        ps_s.p[k], ps_s.n[k] = rows[k], rows[3 + k]
    ps_s.uv[0], ps_s.uv[1], ps_s.pdf = rows[6], rows[7], rows[8]
    ps_s.prim_index = prim.data_ptr()
    ps_s.b[0], ps_s.b[1] = rows[9], rows[10]
    sp = (C.c_void_p * 2)(smp.data_ptr(), smp.data_ptr() + 4 * n)
    st = shape._stream()
    assert lib.hf_sample_position(shape._h, n, C.byref(sp), None, C.byref(ps_s), st) == _capi.HF_EINVAL
    assert b"not enabled" in lib.hf_last_error_string()
    f = C.c_float()
    assert lib.hf_surface_area(shape._h, C.byref(f), None) == _capi.HF_EINVAL
    cnt, ptr = C.c_size_t(), C.c_void_p()
    assert lib.hf_area_cdf(shape._h, C.byref(ptr), C.byref(cnt)) == 0 and cnt.value == 0 and not ptr.value
    shape.ensure_pmf_built()
    active = (torch.arange(n, device=DEV) % 3 != 0).to(torch.uint8)
    _capi.check(lib.hf_sample_position(shape._h, n, C.byref(sp), active.data_ptr(), C.byref(ps_s), st))
    torch.cuda.synchronize()
    off = active == 0
    assert torch.all(out[:, off] == 0) and torch.all(prim[off] == 0)
    assert torch.all(out[8, ~off] > 0)
    ps = shape.sample_position(0.0, smp, active=active.bool())
    assert torch.equal(ps.p, out[0:3]) and torch.equal(ps.pdf, out[8])

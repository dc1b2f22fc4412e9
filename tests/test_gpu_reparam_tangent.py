"""Forward-mode warped-area reparameterisation on the GPU (hf_reparam_tangent, _ReparameterizeOp.jvp,
reparameterize_ray_tangent):
  1. the reference's test01 (src/render/tests/test_reparameterization.py:29-98) as written: a shape translated along x,
     the tangent through torch.autograd.forward_ad;
  2. heights tangents against oracle.reparam_forward;
  3. transposition against the shipped reverse mode (heights, ray.o, ray.d, to_world);
  4. the fused kernel against a per-sample host composition of the existing entry points;
  5. chunking, repeat launches, two streams and graph capture: bitwise;
  6. edge cases: inactive lanes, all-miss batches, no tangents;
  7. the silhouette example: forward mode = reverse mode, and close to finite differences."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import common

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def _ray(hf, o, d):
    return hf.Ray3f(torch.as_tensor(o, dtype=torch.float32).to(DEV).contiguous(),
                    torch.as_tensor(d, dtype=torch.float32).to(DEV).contiguous())


def _translate_x(th):
    one, z = torch.ones_like(th), torch.zeros_like(th)
    return torch.stack([torch.stack(r) for r in [[one, z, z, th], [z, one, z, z], [z, z, one, z]]])


# ---- 1. test01 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ray_o", [[0, 1, -5], [0, 0.0, -5], [0.99, -0.99, -5]], ids=["side", "centre", "corner"])
def test_reference_test01_forward(hf, ray_o):
    shape = hf.Heightfield(heightfield=torch.zeros((9, 9), device=DEV), max_height=1.0, differentiable_to_world=True)
    ray = _ray(hf, np.array(ray_o, np.float32)[:, None], np.array([[0.0], [0.0], [1.0]], np.float32))
    with fwAD.dual_level():
        th = fwAD.make_dual(torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64))
        shape.to_world = _translate_x(th)
        shape.parameters_changed(["to_world"])
        d, det = hf.reparameterize_ray(shape, ray, num_rays=32, kappa=1e6, exponent=3.0)
        assert torch.equal(fwAD.unpack_dual(d).primal, ray.d)
        assert torch.equal(fwAD.unpack_dual(det).primal, torch.ones(1, device=DEV))
        grad_d = fwAD.unpack_dual(d).tangent
    shape.to_world = torch.eye(4, dtype=torch.float64)[:3]
    shape.parameters_changed(["to_world"])
    assert grad_d is not None
    grad_d = grad_d[:, 0].double().cpu()
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    assert bool(si.is_valid()[0])
    new_d = si.p[:, 0].double().cpu() + torch.tensor([1.0, 0, 0], dtype=torch.float64) - ray.o[:, 0].double().cpu()
    new_d = new_d / torch.linalg.norm(new_d)
    assert abs(float(new_d[0] - ray.d[0, 0].cpu()) - float(grad_d[0])) <= 1e-2, (new_d, grad_d)
    assert abs(float(grad_d[1])) < 1e-4 and abs(float(grad_d[2])) < 1e-4, grad_d


# ---- 2. heights tangents vs the oracle ---------------------------------------------------------------------------------

def _field(kind, W=41, H=37, seed=0):
    return common.heights(kind, W, H, np.random.default_rng(seed))


def _rays_np(n, rng, M=None, spread=1.1, far=1.0):
    tgt = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), np.full(n, 0.25)])
    o = tgt + np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.0, 2.0, n)]) * far
    if M is not None:
        A = np.asarray(M, np.float64)
        o, tgt = A[:, :3] @ o + A[:, 3:4], A[:, :3] @ tgt + A[:, 3:4]
    d = tgt - o; d /= np.linalg.norm(d, axis=0)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("kind,kappa,anti,K", [("rand", 30.0, False, 5), ("sine", 2e3, True, 32), ("rand", 1e5, True, 1),
                                               ("sine", 1e5, False, 5), ("sine", 30.0, True, 32)])
def test_heights_tangent_matches_the_oracle(hf, oracle, kind, kappa, anti, K):
    h = _field(kind)
    f = oracle.OracleField(h, max_height=0.5)
    rng = np.random.default_rng(3)
    n = 1500
    o, d = _rays_np(n, rng)
    active = (rng.uniform(size=n) > 0.15).astype(np.uint8)
    ids = rng.permutation(1 << 20)[:n].astype(np.uint32)
    dh = rng.normal(size=h.shape).astype(np.float32)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5)
    Vt, div = hf.reparameterize_ray_tangent(shape, _ray(hf, o, d), dheights=torch.from_numpy(dh).to(DEV), num_rays=K,
                                            kappa=kappa, exponent=3.0, antithetic=anti, seed=9,
                                            active=torch.from_numpy(active).to(DEV),
                                            ray_index=torch.from_numpy(ids.view(np.int32)).to(DEV))
    with oracle.with_ray_ids(ids):
        rV, rdiv = oracle.reparam_forward(f, o, d, dh.astype(np.float64), num_rays=K, kappa=kappa, exponent=3.0,
                                          antithetic=anti, seed=9, active=active)
    assert np.abs(rV).max() > 0
    assert _rel(Vt, rV) <= 2e-4, _rel(Vt, rV)
    if K == 1:   # one sample: div = (<dw, dV> - <(w dV) / w, dw>) / w is 0 up to rounding, and |dw| / w ~ 3 kappa sin(theta)
        assert float(div.abs().max()) <= 1e-3 * float(np.abs(rV).max()) and np.abs(rdiv).max() <= 1e-6 * np.abs(rV).max()
    else:
        assert _rel(div, rdiv) <= 2e-4, _rel(div, rdiv)
    off = torch.from_numpy(active == 0).to(DEV)
    assert bool((Vt[:, off] == 0).all()) and bool((div[off] == 0).all())


# ---- 3. transposition -----------------------------------------------------------------------------------------------

def _transpose_check(hf, shape, o, d, dh, do, dd, dM, K, kappa, seed, M0=None, tol=1e-5):
    """<J t, g> against <t, J^T g>.  The forward tangent of the direction is V_theta; reverse mode differentiates
    normalize(d + V_theta) (reparam.py:262-281), so the pairing is with P V_theta, P = (I - d d^T / |d|^2) / |d|.
    The error is measured relative to sum_i |<(J t)_i, g_i>|, the size of the per-ray terms of the pairing: with random g
    those terms cancel in the sum (|lhs| ~ scale / sqrt(n)), but the float32 rounding of each term, and of the reverse
    mode's float32 accumulation into texels and into the 12 to_world sums, does not cancel with them, so a bound on
    |lhs| alone would measure that rounding rather than the derivative.  A second, looser bound on |lhs| is kept."""
    n = o.shape[1]
    g_dir = torch.randn((3, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    g_div = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    ray = hf.Ray3f(o, d)
    Vt, div = hf.reparameterize_ray_tangent(shape, ray, dheights=dh, d_o=do, d_d=dd, d_to_world=dM, num_rays=K,
                                            kappa=kappa, exponent=3.0, seed=seed)
    dd64, V64 = d.double(), Vt.double()
    n2 = (dd64 * dd64).sum(0)
    PV = (V64 - dd64 * ((dd64 * V64).sum(0) / n2)) / n2.sqrt()
    per_ray = (PV * g_dir.double()).sum(0) + div.double() * g_div.double()
    lhs = float(per_ray.sum())
    # reverse mode
    hl = shape.heightfield.detach().clone().requires_grad_(dh is not None)
    shape.heightfield = hl
    ol = o.clone().requires_grad_(do is not None); dl = d.clone().requires_grad_(dd is not None)
    th = torch.zeros((), dtype=torch.float64, requires_grad=True)
    if dM is not None:
        shape.to_world = torch.as_tensor(M0, dtype=torch.float64) + th * dM.detach().double().cpu().reshape(3, 4)
        shape.parameters_changed(["to_world"])
    dirn, det = hf.reparameterize_ray(shape, hf.Ray3f(ol, dl), num_rays=K, kappa=kappa, exponent=3.0, seed=seed)
    ((dirn * g_dir).sum() + (det * g_div).sum()).backward()
    rhs = 0.0
    if dh is not None:
        rhs += float((hl.grad.double() * dh.double()).sum())
    if do is not None:
        rhs += float((ol.grad.double() * do.double()).sum())
    if dd is not None:
        rhs += float((dl.grad.double() * dd.double()).sum())
    if dM is not None:
        rhs += float(th.grad)
    scale = float(per_ray.abs().sum())
    assert scale > 0 and lhs != 0.0
    print(f"transposition: lhs {lhs:.9g} rhs {rhs:.9g} |lhs - rhs| / scale {abs(lhs - rhs) / scale:.3g}")
    assert abs(lhs - rhs) <= tol * scale, (lhs, rhs, abs(lhs - rhs) / scale)
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs, abs(lhs - rhs) / abs(lhs))


@pytest.mark.parametrize("case", ["moderate", "grazing", "far"])
def test_transposition_against_reverse_mode(hf, case):
    M0 = common.affine(5).astype(np.float64)
    h = _field("sine", 65, 57)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5, to_world=M0,
                           differentiable_to_world=True)
    rng = np.random.default_rng(12)
    n = 256 * 1024 if case == "moderate" else 20000
    if case == "grazing":
        # nearly horizontal in object space, skimming the crests from one side
        lo = np.stack([rng.uniform(-1.5, 1.5, n), np.full(n, -1.6), rng.uniform(0.2, 0.5, n)])
        dl_ = np.stack([rng.uniform(-0.3, 0.3, n), np.ones(n), rng.uniform(-0.12, -0.02, n)])
        A = np.asarray(M0)
        o = (A[:, :3] @ lo + A[:, 3:4]).astype(np.float32)
        dw = A[:, :3] @ dl_
        d = (dw / np.linalg.norm(dw, axis=0)).astype(np.float32)
    else:
        o, d = _rays_np(n, rng, M0, far=(20.0 if case == "far" else 1.0))
    o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(4)
    dh = torch.randn(h.shape, device=DEV, generator=gen)
    do = torch.randn((3, n), device=DEV, generator=gen)
    dd = torch.randn((3, n), device=DEV, generator=gen)
    dM = torch.randn(12, device=DEV, generator=gen) * 0.1
    _transpose_check(hf, shape, o, d, dh, do, dd, dM, 8, 2e3 if case != "far" else 1e5, 5, M0)


def test_transposition_on_the_bench_wavefront(hf):
    h = hf.workload.sine_heights(4096, 4096, device=DEV)
    shape = hf.Heightfield(heightfield=h, max_height=0.5)
    rays = hf.workload.ortho_rays(4096, 4096, 4, DEV)
    dh = torch.randn((4096, 4096), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    _transpose_check(hf, shape, rays[0:3].contiguous(), rays[3:6].contiguous(), dh, None, None, None, 4, 1e5, 0)


# ---- 4. fused kernel vs per-sample composition ------------------------------------------------------------------------

def test_fused_equals_the_per_sample_composition(hf):
    from hf_amd import _capi
    from hf_amd import shape as sh
    L = _capi.lib()
    M0 = common.affine(7).astype(np.float64)
    h = _field("rand", 49, 45, seed=3)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5, to_world=M0,
                           differentiable_to_world=True)
    rng = np.random.default_rng(21)
    n = 30000
    o, d = _rays_np(n, rng, M0, spread=1.2)
    o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(8)
    dh = torch.randn(h.shape, device=DEV, generator=gen)
    do = torch.randn((3, n), device=DEV, generator=gen)
    dd = torch.randn((3, n), device=DEV, generator=gen)
    dM = torch.randn(12, device=DEV, generator=gen) * 0.1
    K, kappa, seed = 6, 500.0, 13
    Vt, div = hf.reparameterize_ray_tangent(shape, hf.Ray3f(o, d), dheights=dh, d_o=do, d_d=dd, d_to_world=dM,
                                            num_rays=K, kappa=kappa, exponent=3.0, antithetic=True, seed=seed)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    o_p, d_p = sh._p3(o), sh._p3(d)
    flags = int(hf.RayFlags.All | hf.RayFlags.FollowShape | hf.RayFlags.BoundaryTest)
    Z = torch.zeros(n, device=DEV, dtype=torch.float64); dZ = torch.zeros((3, n), device=DEV, dtype=torch.float64)
    gV = torch.zeros((3, n), device=DEV, dtype=torch.float64); gdiv = torch.zeros(n, device=DEV, dtype=torch.float64)
    aux_d = torch.empty((3, n), device=DEV); aux_maxt = torch.empty(n, device=DEV)
    h0 = shape.heightfield
    for k in range(K):
        _capi.check(L.hf_reparam_aux_rays(n, C.byref(o_p), C.byref(d_p), None, k, kappa, 1, seed, None,
                                          C.byref(sh._p3(aux_d)), aux_maxt.data_ptr(), stream))
        # omega_local (detached) and the tangent of d_aux = Frame3f(d).to_world(omega) by torch autograd over d
        s0, t0 = sh._coordinate_system(d)
        om = torch.stack([(s0 * aux_d).sum(0), (t0 * aux_d).sum(0), (d * aux_d).sum(0)])

        def d_aux_of(x):
            s_, t_ = sh._coordinate_system(x)
            return s_ * om[0] + t_ * om[1] + x * om[2]
        dd_aux = torch.autograd.functional.jvp(d_aux_of, (d,), (dd,))[1]
        with fwAD.dual_level():
            shape.heightfield = fwAD.make_dual(h0, dh)
            shape.to_world = fwAD.make_dual(torch.as_tensor(M0, dtype=torch.float64), dM.double().cpu().reshape(3, 4))
            shape.parameters_changed(["to_world"])
            ray = hf.Ray3f(fwAD.make_dual(o, do), fwAD.make_dual(aux_d.clone(), dd_aux), aux_maxt.clone())
            si = shape.ray_intersect(ray, flags)
            p, t = fwAD.unpack_dual(si.p), fwAD.unpack_dual(si.t)
            bt = fwAD.unpack_dual(si.boundary_test).primal.contiguous()
        shape.heightfield = h0
        shape.to_world = torch.as_tensor(M0, dtype=torch.float64)
        shape.parameters_changed(["to_world"])
        w = torch.zeros(n, device=DEV); dw = torch.zeros((3, n), device=DEV)
        tt, pp = t.primal.contiguous(), p.primal.contiguous()
        _capi.check(L.hf_reparam_weights(0, n, C.byref(o_p), C.byref(d_p), None, k, kappa, 3.0, 1, seed, None,
                                         tt.data_ptr(), C.byref(sh._p3(pp)), bt.data_ptr(), w.data_ptr(),
                                         C.byref(sh._p3(dw)), None, None, None, None, None, stream))
        hit = torch.isfinite(tt)
        T, P = tt.double(), pp.double()
        dT, dP = t.tangent.double(), p.tangent.double()
        po = P - o.double()
        dV = (dP - do.double()) / T - po * dT / (T * T)
        dV = torch.where(hit, dV, dd.double())
        Z += w.double(); dZ += dw.double()
        gV += w.double() * dV; gdiv += (dw.double() * dV).sum(0)
    iZ = 1.0 / Z.clamp_min(1e-8)
    rV = gV * iZ
    rdiv = (gdiv - (rV * dZ).sum(0)) * iZ
    assert float(rV.abs().max()) > 0
    assert _rel(Vt, rV) <= 5e-5, _rel(Vt, rV)     # float32 t / p of two code paths, one rounding apart per step
    assert _rel(div, rdiv) <= 5e-5, _rel(div, rdiv)


# ---- 5. chunks, repeats, streams, capture -----------------------------------------------------------------------------

def _bits_setup(hf, n=50000):
    h = _field("sine", 129, 129)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5)
    o, d = _rays_np(n, np.random.default_rng(2))
    dh = torch.randn(h.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    dd = torch.randn((3, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    return shape, _ray(hf, o, d), dh, dd


def test_chunked_repeated_and_captured_runs_are_bitwise(hf, monkeypatch):
    from hf_amd import shape as sh
    shape, ray, dh, dd = _bits_setup(hf)
    kw = dict(dheights=dh, d_d=dd, num_rays=5, kappa=2e3, antithetic=True, seed=3)
    V0, D0 = hf.reparameterize_ray_tangent(shape, ray, **kw)
    V1, D1 = hf.reparameterize_ray_tangent(shape, ray, **kw)
    assert torch.equal(V0, V1) and torch.equal(D0, D1)
    monkeypatch.setattr(sh, "REPARAM_KEEP_BYTES", 20 * 5 * 7001)          # 8 chunks, the last one short
    V2, D2 = hf.reparameterize_ray_tangent(shape, ray, **kw)
    assert torch.equal(V0, V2) and torch.equal(D0, D2)
    monkeypatch.undo()
    # a captured launch replays to the eager result
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        hf.reparameterize_ray_tangent(shape, ray, **kw)
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Vg, Dg = hf.reparameterize_ray_tangent(shape, ray, **kw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(V0, Vg) and torch.equal(D0, Dg)


def test_two_streams_on_one_handle_give_the_serial_results(hf):
    shape, ray, dh, dd = _bits_setup(hf)
    kw = dict(num_rays=4, kappa=1e5, seed=1)
    ref_a = hf.reparameterize_ray_tangent(shape, ray, dheights=dh, **kw)
    ref_b = hf.reparameterize_ray_tangent(shape, ray, d_d=dd, **kw)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for s in (sa, sb):
        s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(sa):
        got_a = hf.reparameterize_ray_tangent(shape, ray, dheights=dh, **kw)
    with torch.cuda.stream(sb):
        got_b = hf.reparameterize_ray_tangent(shape, ray, d_d=dd, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got_a, ref_a))
    assert all(torch.equal(x, y) for x, y in zip(got_b, ref_b))


# ---- 6. edge cases ------------------------------------------------------------------------------------------------------

def test_edge_cases(hf):
    shape, ray, dh, dd = _bits_setup(hf, n=4096)
    n = len(ray)
    active = torch.arange(n, device=DEV) % 3 != 0
    V, D = hf.reparameterize_ray_tangent(shape, ray, dheights=dh, d_d=dd, num_rays=8, kappa=300.0, active=active)
    assert bool((V[:, ~active] == 0).all()) and bool((D[~active] == 0).all())
    assert float(V[:, active].abs().max()) > 0
    # all rays miss (pointing up, away from the field): V_theta = dd (sum w_k / Z = 1) and div = 0
    up = _ray(hf, torch.stack([ray.o[0], ray.o[1], ray.o[2] + 3.0]).cpu(), torch.tensor([[0.0], [0.0], [1.0]]).expand(3, n))
    Vm, Dm = hf.reparameterize_ray_tangent(shape, up, dheights=dh, d_d=dd, num_rays=8, kappa=300.0)
    assert torch.allclose(Vm, dd, rtol=1e-5, atol=1e-6)
    # div = (sum <dw_k, dd> - <dd, dZ> sum w_k / Z) / Z cancels up to rounding: |dZ| / Z ~ 3 kappa sin(theta) ~ 1e2 here
    assert float(Dm.abs().max()) <= 1e-2
    # hits, no tangent on anything: exactly zero
    V0, D0 = hf.reparameterize_ray_tangent(shape, ray, num_rays=4, kappa=1e5)
    assert bool((V0 == 0).all()) and bool((D0 == 0).all())


# ---- 7. the silhouette example ------------------------------------------------------------------------------------------

def test_silhouette_forward_mode_equals_reverse_mode_and_finite_differences(hf):
    import silhouette_gradient as sg
    film, spp, eps = 160, 64, 0.02
    h, ridge = sg.scene(device=DEV)
    rays = sg.camera(film, spp, DEV)
    hp, hm = h.clone(), h.clone()
    hp[ridge] += eps; hm[ridge] -= eps
    fd = (sg.render_sum(hp, rays, spp) - sg.render_sum(hm, rays, spp)) / (2 * eps)
    _, g_rev = sg.gradients(h, ridge, rays, spp, aux=32, kappa=1e5)
    _, g_fwd = sg.forward_derivative(h, ridge, rays, spp, aux=32, kappa=1e5)
    assert fd > 0
    assert abs(g_fwd - g_rev) <= 1e-4 * abs(g_rev), (g_fwd, g_rev)
    assert abs(g_fwd - fd) < 0.12 * fd, (g_fwd, fd)

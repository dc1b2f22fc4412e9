"""Reverse-mode warped-area reparameterisation with respect to the heights, ray.o, ray.d and to_world on the GPU
(hf_reparam_backward_full, reparameterize_ray_adjoint, the routing of _ReparameterizeOp.backward):
  1. against the oracle (heights, ray.o, ray.d) and the float64 restatement (to_world);
  2. against the per-sample path (REPARAM_FUSED = False), which defines the accuracy to expect of a float32 chain;
  3. transposition against hf_reparam_tangent on the device;
  4. subsets of the outputs, repeat launches, graph capture, two streams, chunking;
  5. edge cases and the routing of backward().
Every set-up has auxiliary hits AND active misses; the shares are asserted."""
import numpy as np
import pytest
import torch

import common
import reparam_backward_ref as B
import reparam_tangent_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HEIGHTS_ATOMICS = 2e-6      # the project's bound for the same sums in a different atomics order (test_reparam.py:119)


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def _rays_np(n, rng, M=None, spread=1.1, far=1.0):
    tgt = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), np.full(n, 0.25)])
    o = tgt + np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.0, 2.0, n)]) * far
    if M is not None:
        A = np.asarray(M, np.float64)
        o, tgt = A[:, :3] @ o + A[:, 3:4], A[:, :3] @ tgt + A[:, 3:4]
    d = tgt - o; d /= np.linalg.norm(d, axis=0)
    return o.astype(np.float32), d.astype(np.float32)


class _Case:
    """a small wavefront with random ray ids and 10 % inactive lanes, on the device and in the oracle"""

    def __init__(self, hf, oracle, kappa, anti, K, tw=None, n=1500, seed=9, kind="sine"):
        rng = np.random.default_rng(3)
        self.hf, self.oracle, self.n, self.tw = hf, oracle, n, tw
        self.h = common.heights(kind, 41, 37, np.random.default_rng(0))
        self.M = np.eye(4)[:3] if tw is None else np.asarray(tw, np.float64)
        self.f = oracle.OracleField(self.h, max_height=0.5, to_world=self.M)
        self.o, self.d = _rays_np(n, rng, None if tw is None else self.M)
        self.active = (rng.uniform(size=n) > 0.1).astype(np.uint8)
        self.ids = rng.permutation(1 << 20)[:n].astype(np.uint32)
        self.gd = rng.normal(size=(3, n)).astype(np.float32)
        self.gdiv = rng.normal(size=n).astype(np.float32)
        self.cfg = dict(num_rays=K, kappa=kappa, exponent=3.0, antithetic=anti, seed=seed)
        with oracle.with_ray_ids(self.ids):
            self.S, self.act = R.samples(oracle, self.f, self.o, self.d, K, kappa, 3.0, anti, seed, self.active)
        hits = sum(int(s[1].sum()) for s in self.S)
        misses = sum(int((~s[1] & self.act).sum()) for s in self.S)
        total = int(self.act.sum()) * K
        assert 0.02 < misses / total < 0.9 and hits / total > 0.1, (hits, misses, total)   # as test_reparam.py:404
        self.t = {k: torch.from_numpy(v).to(DEV) for k, v in
                  dict(o=self.o, d=self.d, gd=self.gd, gdiv=self.gdiv, active=self.active, ids=self.ids.view(np.int32)).items()}

    def shape(self):
        kw = {} if self.tw is None else dict(to_world=self.M, differentiable_to_world=True)
        return self.hf.Heightfield(heightfield=torch.from_numpy(self.h).to(DEV), max_height=0.5, **kw)

    def adjoint(self, shape=None, **want):
        want = want or dict(heights=True, o=True, d=True, to_world=True)
        t = self.t
        return self.hf.reparameterize_ray_adjoint(shape or self.shape(), self.hf.Ray3f(t["o"], t["d"]), t["gd"], t["gdiv"],
                                                  active=t["active"], ray_index=t["ids"], **self.cfg, **want)

    def autograd(self):
        """(grad_h, grad_o, grad_d, grad_to_world or None) through reparameterize_ray(...).backward()"""
        hf, t = self.hf, self.t
        shape = self.shape()
        shape.heightfield.requires_grad_(True)
        ol, dl = t["o"].clone().requires_grad_(True), t["d"].clone().requires_grad_(True)
        tw = None
        if self.tw is not None:
            tw = torch.as_tensor(self.M, dtype=torch.float64).requires_grad_(True)
            shape.to_world = tw
            shape.parameters_changed(["to_world"])
        dirn, det = hf.reparameterize_ray(shape, hf.Ray3f(ol, dl), active=t["active"], ray_index=t["ids"], **self.cfg)
        ((dirn * t["gd"]).sum() + (det * t["gdiv"]).sum()).backward()
        return shape.heightfield.grad, ol.grad, dl.grad, None if tw is None else tw.grad

    def oracle_grads(self):
        with self.oracle.with_ray_ids(self.ids):
            return self.oracle.reparam_backward(self.f, self.o, self.d, self.gd, self.gdiv, active=self.active,
                                                ray_grads=True, **self.cfg)

    def restatement(self):
        return B.reparam_backward(self.f, self.S, self.act, self.o, self.d, self.M, self.h, self.gd, self.gdiv)


def _per_sample(case, monkeypatch):
    from hf_amd import shape as sh
    with monkeypatch.context() as m:
        m.setattr(sh, "REPARAM_FUSED", False)
        return case.autograd()


def _aux_shares(shape, ray, K, kappa, anti=False, seed=0, active=None):
    """(share of auxiliary hits, share of active misses) among the samples of the active rays: the t row that
    hf_reparam_trace_all writes for exactly the samples the backward regenerates"""
    import ctypes as C
    from hf_amd import _capi, shape as sh
    n = len(ray)
    store = torch.empty((K, 5, n), dtype=torch.float32, device=DEV)
    _, si_s, pi_s = sh._sample_structs(store[0])
    o_p, d_p = sh._p3(ray.o), sh._p3(ray.d)
    act = None if active is None else active.to(torch.uint8).contiguous()
    _capi.check(_capi.lib().hf_reparam_trace_all(shape._h, n, C.byref(o_p), C.byref(d_p), sh._ptr(act), K, kappa, int(anti),
                                                 seed, None, C.byref(pi_s), C.byref(si_s), 5 * n,
                                                 torch.cuda.current_stream(DEV).cuda_stream))
    keep = torch.ones(n, dtype=torch.bool, device=DEV) if act is None else act != 0
    hit = float(torch.isfinite(store[:, 1][:, keep]).float().mean())
    return hit, 1.0 - hit


def _assert_both_branches(shape, ray, K, kappa, anti=False, seed=0, active=None):
    hit, miss = _aux_shares(shape, ray, K, kappa, anti, seed, active)
    print(f"auxiliary samples: {hit:.3f} hit, {miss:.3f} miss")
    assert 0.02 < miss < 0.9 and hit > 0.1, (hit, miss)   # both branches of V_direct, as test_reparam.py:404


GRID = [(30.0, False, 5), (2000.0, True, 8), (1e5, True, 32)]


# ---- 1. the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa,anti,K", GRID)
def test_matches_the_oracle(hf, oracle, kappa, anti, K):
    c = _Case(hf, oracle, kappa, anti, K)
    gh, go, gd, _ = c.adjoint(heights=True, o=True, d=True)
    rh, ro, rd = c.oracle_grads()
    errs = _rel(gh, rh), _rel(go, ro), _rel(gd, rd)
    print(f"oracle kappa {kappa:g} K {K}: heights {errs[0]:.3g} grad_o {errs[1]:.3g} grad_d {errs[2]:.3g}")
    assert np.linalg.norm(rh) > 0 and np.linalg.norm(ro) > 0 and np.linalg.norm(rd) > 0
    assert errs[0] <= 3e-5 and errs[1] <= 2e-4 and errs[2] <= 2e-4, errs
    off = c.t["active"] == 0
    assert bool((go[:, off] == 0).all()) and bool((gd[:, off] == 0).all())


# ---- 2. to_world, and the per-sample path as the measure of a float32 chain ----------------------------------------

@pytest.mark.parametrize("kappa,anti,K", GRID)
def test_to_world_and_the_ray_are_as_accurate_as_the_per_sample_path(hf, oracle, monkeypatch, kappa, anti, K):
    """No bound for the twelve to_world sums exists, so none is invented: the per-sample path's error against the same
    float64 values is measured on the same inputs and the fused error may be at most twice that (two float32 chains of
    equal length in a different order).  The same criterion for grad_o / grad_d against the oracle."""
    _fused_vs_per_sample(_Case(hf, oracle, kappa, anti, K, tw=common.affine(2)), monkeypatch, f"kappa {kappa:g} K {K}")


def _fused_vs_per_sample(c, monkeypatch, label):
    gh, go, gd, gM = c.adjoint()
    ph, po, pd, pM = _per_sample(c, monkeypatch)
    _, ro, rd = c.oracle_grads()
    _, _, _, rM = c.restatement()
    assert np.linalg.norm(rM) > 0
    for name, fused, per, ref in (("grad_to_world", gM.reshape(3, 4), pM, rM), ("grad_o", go, po, ro), ("grad_d", gd, pd, rd)):
        ef, ep = _rel(fused, ref), _rel(per, ref)
        print(f"accuracy {label} {name}: fused {ef:.3g} per-sample {ep:.3g}")
        assert ef <= 2 * ep, (name, ef, ep)
    assert _rel(gh, ph) <= HEIGHTS_ATOMICS, _rel(gh, ph)


@pytest.mark.parametrize("K", [1, 32])
def test_one_and_thirty_two_samples(hf, oracle, monkeypatch, K):
    """num_rays at both ends of 1..32 (32: the top bit of the kernel's hit mask and its k + 1 < K guard): every output
    against the float64 values, by the criterion above"""
    _fused_vs_per_sample(_Case(hf, oracle, 2000.0, False, K, tw=common.affine(2), seed=11), monkeypatch, f"num_rays {K}")


# ---- 3. transposition on the device -------------------------------------------------------------------------------------

def _transposition(hf, case, xform, orient):
    M0 = common.affine(5).astype(np.float64) if xform == "affine" else np.eye(4)[:3]
    h = common.heights("sine", 65, 57, np.random.default_rng(0))
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5, to_world=M0,
                           differentiable_to_world=True)
    rng = np.random.default_rng(12)
    n = 256 * 1024 if case == "moderate" else 20000
    K, kappa, seed = 8, (2e3 if case != "far" else 1e5), 5
    if case == "grazing":   # nearly horizontal in object space, skimming the crests from one side
        lo = np.stack([rng.uniform(-1.5, 1.5, n), np.full(n, -1.6), rng.uniform(0.2, 0.5, n)])
        dl_ = np.stack([rng.uniform(-0.3, 0.3, n), np.ones(n), rng.uniform(-0.12, -0.02, n)])
        o = (M0[:, :3] @ lo + M0[:, 3:4]).astype(np.float32)
        dw = M0[:, :3] @ dl_
        d = (dw / np.linalg.norm(dw, axis=0)).astype(np.float32)
    else:
        o, d = _rays_np(n, rng, M0, far=(20.0 if case == "far" else 1.0))
    o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(4)
    dh = torch.randn(h.shape, device=DEV, generator=gen)
    do = torch.randn((3, n), device=DEV, generator=gen)
    dd = torch.randn((3, n), device=DEV, generator=gen)
    dM = torch.randn(12, device=DEV, generator=gen) * 0.1
    g_dir = torch.randn((3, n), device=DEV, generator=gen)
    g_div = torch.randn(n, device=DEV, generator=gen)
    ray = hf.Ray3f(o, d)
    _assert_both_branches(shape, ray, K, kappa, seed=seed)
    Vt, div = hf.reparameterize_ray_tangent(shape, ray, dheights=dh, d_o=do, d_d=dd, d_to_world=dM, num_rays=K,
                                            kappa=kappa, exponent=3.0, seed=seed)
    # reverse mode differentiates normalize(d + V_theta): the pairing is with P V_theta (test_gpu_reparam_tangent.py)
    dd64, V64 = d.double(), Vt.double()
    n2 = (dd64 * dd64).sum(0)
    PV = (V64 - dd64 * ((dd64 * V64).sum(0) / n2)) / n2.sqrt()
    per_ray = (PV * g_dir.double()).sum(0) + div.double() * g_div.double()
    if orient:
        # Orient every ray's (g_dir, g_div) so that its term of the pairing is positive.  With signs left random the
        # terms cancel in the sum (grazing rays: |lhs| = 5e-5 of the term scale) and the bound relative to |lhs| then asks
        # for less than the float32 rounding of the terms themselves (2^-24 of the scale).  Oriented, |lhs| IS the scale:
        # only the first bound below (1e-5 of the scale) is effective, the second is implied by it.  The adjoint is
        # linear in g, so this is still the transposition identity.  The random-sign pairing, where the relative bound
        # is the binding one, is test_transposition_with_random_signs.
        sgn = torch.where(per_ray < 0, -1.0, 1.0)
        g_dir, g_div, per_ray = g_dir * sgn.float(), g_div * sgn.float(), per_ray * sgn
    lhs, scale = float(per_ray.sum()), float(per_ray.abs().sum())
    assert abs(lhs) >= 1e-3 * scale          # 2^-24 scale <= 1e-4 |lhs|: the relative bound is above float32 rounding
    gh, go, gd, gM = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, num_rays=K, kappa=kappa, exponent=3.0,
                                                   seed=seed, heights=True, o=True, d=True, to_world=True)
    rhs = float((gh.double() * dh.double()).sum() + (go.double() * do.double()).sum() + (gd.double() * dd.double()).sum()
                + (gM.double() * dM.double()).sum())
    assert scale > 0 and lhs != 0.0
    print(f"transposition {case} {xform}: lhs {lhs:.9g} rhs {rhs:.9g} |lhs - rhs| / scale {abs(lhs - rhs) / scale:.3g}")
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, abs(lhs - rhs) / scale)
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs, abs(lhs - rhs) / abs(lhs))


@pytest.mark.parametrize("case", ["moderate", "grazing", "far"])
@pytest.mark.parametrize("xform", ["identity", "affine"])
def test_transposition_against_the_tangent_kernel(hf, case, xform):
    _transposition(hf, case, xform, orient=True)


@pytest.mark.parametrize("xform", ["identity", "affine"])
def test_transposition_with_random_signs(hf, xform):
    """the pairing as test_gpu_reparam_tangent.py's _transpose_check forms it, signs of g left random: the terms cancel
    and the bound relative to |lhs| binds.  On the 256 k-ray set, whose sum keeps |lhs| >= 1e-3 of the scale (asserted)"""
    _transposition(hf, "moderate", xform, orient=False)


# ---- 4. subsets, repeats, capture, streams, chunks ---------------------------------------------------------------------

def _big(hf, cfgs, n=50000):
    """cfgs: the (num_rays, kappa, antithetic, seed) the calling test samples with; the shares are asserted for each"""
    M0 = common.affine(7).astype(np.float64)
    h = common.heights("sine", 129, 129, np.random.default_rng(0))
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=0.5, to_world=M0, differentiable_to_world=True)
    o, d = _rays_np(n, np.random.default_rng(2), M0, spread=1.3)
    gen = torch.Generator(device=DEV).manual_seed(5)
    g_dir = torch.randn((3, n), device=DEV, generator=gen)
    g_div = torch.randn(n, device=DEV, generator=gen)
    ray = hf.Ray3f(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))
    for K, kappa, anti, seed in cfgs:
        _assert_both_branches(shape, ray, K, kappa, anti, seed)
    return shape, ray, g_dir, g_div


ALL = dict(heights=True, o=True, d=True, to_world=True)


def test_subsets_equal_the_all_outputs_call(hf):
    shape, ray, g_dir, g_div = _big(hf, [(5, 2e3, True, 3)])
    kw = dict(num_rays=5, kappa=2e3, antithetic=True, seed=3)
    gh, go, gd, gM = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, **ALL)
    assert all(float(x.abs().max()) > 0 for x in (gh, go, gd, gM))
    h1 = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, heights=True)
    o1 = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, heights=False, o=True)
    d1 = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, heights=False, d=True)
    m1 = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, heights=False, to_world=True)
    assert h1[1] is None and h1[2] is None and h1[3] is None and o1[0] is None and o1[2] is None and m1[0] is None
    assert torch.equal(o1[1], go) and torch.equal(d1[2], gd) and torch.equal(m1[3], gM)
    assert _rel(h1[0], gh) <= HEIGHTS_ATOMICS
    # heights alone: the heights-only kernel (hf_reparam_backward) through backward()
    hl = shape.heightfield.detach().clone().requires_grad_(True)
    shape.heightfield = hl
    dirn, det = hf.reparameterize_ray(shape, ray, **kw)
    ((dirn * g_dir).sum() + (det * g_div).sum()).backward()
    assert _rel(h1[0], hl.grad) <= HEIGHTS_ATOMICS, _rel(h1[0], hl.grad)
    # the caller's accumulators are added to
    acc_h, acc_M = gh.clone(), gM.clone()
    r = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, heights=True, to_world=True, grad_heightfield=acc_h,
                                      grad_to_world=acc_M)
    assert r[0] is acc_h and r[3] is acc_M
    assert _rel(acc_h, 2 * gh) <= HEIGHTS_ATOMICS and _rel(acc_M, 2 * gM) <= 1e-6


def test_repeated_and_captured_launches(hf):
    shape, ray, g_dir, g_div = _big(hf, [(5, 2e3, True, 3)])
    kw = dict(num_rays=5, kappa=2e3, antithetic=True, seed=3, **ALL)
    a = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw)
    b = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert _rel(b[0], a[0]) <= HEIGHTS_ATOMICS
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw)
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
    assert _rel(c[0], a[0]) <= HEIGHTS_ATOMICS


def test_two_streams_on_one_handle_give_the_serial_results(hf):
    shape, ray, g_dir, g_div = _big(hf, [(4, 1e5, False, 1)])
    kw = dict(num_rays=4, kappa=1e5, seed=1)
    wa, wb = dict(heights=True, o=True), dict(heights=False, d=True, to_world=True)
    ref_a = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, **wa)
    ref_b = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, **wb)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for s in (sa, sb):
        s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(sa):
        got_a = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, **wa)
    with torch.cuda.stream(sb):
        got_b = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, **kw, **wb)
    torch.cuda.synchronize()
    assert torch.equal(got_a[1], ref_a[1]) and _rel(got_a[0], ref_a[0]) <= HEIGHTS_ATOMICS
    assert torch.equal(got_b[2], ref_b[2]) and torch.equal(got_b[3], ref_b[3])


def test_chunked_equals_unchunked(hf, oracle, monkeypatch):
    from hf_amd import shape as sh
    c = _Case(hf, oracle, 2000.0, True, 8, tw=common.affine(2), n=3000)
    gh, go, gd, gM = c.adjoint()
    ph, po, pd, pM = _per_sample(c, monkeypatch)
    monkeypatch.setattr(sh, "REPARAM_KEEP_BYTES", 20 * 8 * 431)          # 7 chunks, the last one short
    ch, co, cd, cM = c.adjoint()
    monkeypatch.undo()
    assert torch.equal(co, go) and torch.equal(cd, gd)
    assert _rel(ch, gh) <= HEIGHTS_ATOMICS
    rM = c.restatement()[3]
    ec, ep = _rel(cM.reshape(3, 4), rM), _rel(pM, rM)
    print(f"chunked grad_to_world: fused {ec:.3g} per-sample {ep:.3g}")
    assert ec <= 2 * ep, (ec, ep)


# ---- 5. edge cases and routing -------------------------------------------------------------------------------------------

def test_edge_cases(hf):
    shape, ray, g_dir, g_div = _big(hf, [(1, 2e3, False, 0), (32, 2e3, False, 0)], n=4096)
    n = len(ray)
    e = hf.Ray3f(torch.empty((3, 0), device=DEV), torch.empty((3, 0), device=DEV))
    r = hf.reparameterize_ray_adjoint(shape, e, torch.empty((3, 0), device=DEV), torch.empty(0, device=DEV), **ALL)
    assert r[1].shape == (3, 0) and r[2].shape == (3, 0) and bool((r[0] == 0).all()) and bool((r[3] == 0).all())
    off = torch.zeros(n, dtype=torch.bool, device=DEV)
    r = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, num_rays=8, kappa=300.0, active=off, **ALL)
    assert all(bool((x == 0).all()) for x in r)
    for K in (1, 32):   # (their values: test_one_and_thirty_two_samples)
        r = hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, num_rays=K, kappa=2e3, **ALL)
        assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in r), K
    with pytest.raises(ValueError):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, num_rays=33)
    with pytest.raises(ValueError):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, heights=False)
    with pytest.raises(ValueError, match="grad_heightfield lives on cpu"):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, grad_heightfield=torch.zeros(129, 129))
    with pytest.raises(ValueError, match="grad_to_world lives on cpu"):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, to_world=True, grad_to_world=torch.zeros(12))
    with pytest.raises(ValueError, match="grad_to_world"):
        hf.reparameterize_ray_adjoint(shape, ray, g_dir, g_div, to_world=True, grad_to_world=torch.zeros(12, device=DEV).double())


def test_a_wavefront_that_misses_entirely(hf, monkeypatch):
    """every auxiliary ray misses: V_direct = ray.d for every sample, so grad_o = 0 and grad_d = sum_k gVd_k.  Against the
    per-sample path, which adds the same float32 values sample by sample in the same order: K roundings at most."""
    from hf_amd import shape as sh
    shape, ray, g_dir, g_div = _big(hf, [], n=4096)      # (no shares: this test's rays are made to miss, asserted below)
    n, K = len(ray), 8
    up = hf.Ray3f(torch.stack([ray.o[0], ray.o[1], ray.o[2] + 30.0]),
                  torch.tensor([[0.0], [0.6], [0.8]], device=DEV).expand(3, n).contiguous())
    r = hf.reparameterize_ray_adjoint(shape, up, g_dir, g_div, num_rays=K, kappa=300.0, **ALL)
    assert bool((r[0] == 0).all()) and bool((r[1] == 0).all()) and bool((r[3] == 0).all())
    assert float(r[2].abs().max()) > 0
    monkeypatch.setattr(sh, "REPARAM_FUSED", False)
    ol, dl = up.o.clone().requires_grad_(True), up.d.clone().requires_grad_(True)
    dirn, det = hf.reparameterize_ray(shape, hf.Ray3f(ol, dl), num_rays=K, kappa=300.0)
    ((dirn * g_dir).sum() + (det * g_div).sum()).backward()
    assert bool((ol.grad == 0).all())
    assert _rel(r[2], dl.grad) <= K * 2.0 ** -23, _rel(r[2], dl.grad)


def test_backward_routes_to_the_fused_kernel(hf, monkeypatch):
    from hf_amd import shape as sh
    shape, ray, g_dir, g_div = _big(hf, [(4, 2e3, False, 0)], n=4096)

    def boom(*a, **k):
        raise AssertionError("the per-sample path was taken")
    monkeypatch.setattr(sh, "_reparam_backward_per_sample", boom)

    def run(ray_grad, tw_grad):
        shape.heightfield = shape.heightfield.detach().clone().requires_grad_(True)
        tw = torch.as_tensor(common.affine(7), dtype=torch.float64).requires_grad_(tw_grad)
        shape.to_world = tw
        shape.parameters_changed(["to_world"])
        ol, dl = ray.o.clone().requires_grad_(ray_grad), ray.d.clone().requires_grad_(ray_grad)
        dirn, det = hf.reparameterize_ray(shape, hf.Ray3f(ol, dl), num_rays=4, kappa=2e3)
        ((dirn * g_dir).sum() + (det * g_div).sum()).backward()
        return shape.heightfield.grad, ol.grad, dl.grad, tw.grad
    gh, go, gd, gM = run(True, False)
    assert gM is None and all(float(x.abs().max()) > 0 for x in (gh, go, gd))
    gh, go, gd, gM = run(False, True)
    assert go is None and gd is None and float(gM.abs().max()) > 0 and float(gh.abs().max()) > 0
    monkeypatch.setattr(sh, "REPARAM_FUSED", False)
    with pytest.raises(AssertionError, match="per-sample path"):
        run(True, True)

"""Large-steps preconditioning on the device (hf_large_steps_apply / _solve, hf_amd.LargeSteps) against the restatement
in tests/largesteps_ref.py: the float64 matrix, its direct solve and conjugate gradients in the kernels' operation order.

The two solve assertions, used throughout (A = I + lambda L has its spectrum in [1, 1 + 12 lambda], so |A^-1| <= 1):
  * with R = |A v_gpu - u|_2 evaluated in float64 on the host, |v_gpu - v_direct|_2 <= R (1 + 1e-6) + 1e-12 |v_direct|_2;
  * R / |u|_2 <= 2 max(rel_tol, the restatement's own true residual on the same input): the factor 2 covers a different
    order of the terms of a dot product.
Measured on an MI355X over the 42 solve cases below (grid x lambda x right-hand side) and the forced-grid repeats: R / |u|
is between 0.015 and 1.00 of max(rel_tol, the restatement's), i.e. at most half the bound, and the iteration counts equal
the restatement's in every case (margin 3); at 257x130: 21 / 21 (lambda 1, random / spike), 86 / 85 (19), 190 / 191 (100)."""
import functools
import os
import sys

import numpy as np
import pytest

import largesteps_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every degree case (2x2), W not a multiple of 4, a row shorter than one lane group (2, 5, 7), items of 4 rows crossed
# (H = 7, 17, 130), block borders crossed in both directions (257x130: 9 blocks of 256 items), an exact fit (64x64)
GRIDS = [(2, 2), (2, 7), (7, 2), (5, 4), (33, 17), (64, 64), (257, 130)]
TOL, MAX_ITER = 1e-6, 256


@functools.lru_cache(maxsize=None)
def _case(W, H, lam, kind):
    """(u, v_direct, the restatement's iterations, its true relative residual): computed once, read-only"""
    u = R.rhs(kind, W, H, seed=W * 1000 + H)
    x, it, _ = R.cg_f32(W, H, lam, u, max_iter=MAX_ITER, rel_tol=TOL)
    true = R.true_residual(W, H, lam, x, u) / np.linalg.norm(u.astype(np.float64))
    u.setflags(write=False)
    return u, R.solve_direct(W, H, lam, u), it, true


def _dev(torch, a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")


def _check_solution(W, H, lam, v_gpu, u, v_direct=None, ref_true=None, what=""):
    """the two solve assertions; returns R / |u|.  ref_true: the restatement's true residual on u (None: computed here)"""
    u64 = np.asarray(u, np.float64)
    if ref_true is None:
        x = R.cg_f32(W, H, lam, u, max_iter=MAX_ITER, rel_tol=TOL)[0]
        ref_true = R.true_residual(W, H, lam, x, u64) / np.linalg.norm(u64)
    v_direct = R.solve_direct(W, H, lam, u64) if v_direct is None else v_direct
    Rn = R.true_residual(W, H, lam, v_gpu, u64)
    err = np.linalg.norm(np.asarray(v_gpu, np.float64) - v_direct)
    rel = Rn / np.linalg.norm(u64)
    print(f"{what} {W}x{H} lambda {lam}: |v - v_direct| {err:.3e}, R {Rn:.3e}, R/|u| {rel:.3e}, restatement {ref_true:.3e}")
    assert err <= Rn * (1 + 1e-6) + 1e-12 * np.linalg.norm(v_direct), (what, err, Rn)
    assert rel <= 2 * max(TOL, ref_true), (what, rel, ref_true)
    return rel


@pytest.mark.parametrize("W,H", GRIDS)
def test_apply(hf, W, H):
    import torch
    v = R.rhs("random", W, H, seed=7 * W + H) * np.float32(3.0)
    for lam in (0.0, 1.0, 19.0):
        ls = hf.LargeSteps(W, H, lambda_=lam)
        u = ls.to_differential(_dev(torch, v)).cpu().numpy()
        if lam == 0.0:
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))               # the identity, bit for bit
        err = np.abs(u - R.apply_f64(W, H, lam, v)).max()
        # seven terms and the scale, each rounded once: derived, not measured
        assert err <= 8 * 2.0 ** -24 * (1 + 12 * lam) * np.abs(v).max(), (lam, err)


def _solve_case(hf, W, H, lam, kind):
    import torch
    u, v_direct, ref_it, ref_true = _case(W, H, lam, kind)
    ls = hf.LargeSteps(W, H, lambda_=lam, max_iter=MAX_ITER, tol=TOL)
    v = ls.from_differential(_dev(torch, u), check=True)
    it, res = ls.last_info()
    v = v.cpu().numpy()
    _check_solution(W, H, lam, v, u, v_direct, ref_true, kind)
    print(f"   iterations {it} (restatement {ref_it}), reported residual {res:.3e}")
    assert abs(it - ref_it) <= 3, (it, ref_it)
    assert res <= TOL
    assert abs(v.astype(np.float64).sum() - u.astype(np.float64).sum()) <= 64 * 2.0 ** -24 * np.abs(v).sum()   # 1^T A = 1^T
    return v


@pytest.mark.parametrize("kind", ["random", "spike"])
@pytest.mark.parametrize("lam", [1.0, 19.0, 100.0])
@pytest.mark.parametrize("W,H", GRIDS)
def test_solve(hf, W, H, lam, kind):
    _solve_case(hf, W, H, lam, kind)


def test_solve_grid_stride(hf, monkeypatch):
    """3 blocks for the 2145 items of 257x130: every block goes round its loop three times, and a sum has 3 partials"""
    from hf_amd import _capi
    free = _solve_case(hf, 257, 130, 19.0, "random")
    monkeypatch.setenv("HF_FORCE_GRID", "3")
    assert _capi.lib().hf_grid_blocks(65 * 33, 0) == 3
    forced = _solve_case(hf, 257, 130, 19.0, "random")
    again = _solve_case(hf, 257, 130, 19.0, "random")
    assert np.array_equal(forced, again) and forced.shape == free.shape


def test_iteration_cap(hf):
    import torch
    W, H = 33, 17
    u = _dev(torch, _case(W, H, 19.0, "random")[0])
    ls = hf.LargeSteps(W, H, lambda_=19.0, max_iter=5, tol=TOL)
    ls.from_differential(u)
    it, res = ls.last_info()
    assert it == 5 and res > TOL
    with pytest.raises(RuntimeError, match="residual"):
        ls.from_differential(u, check=True)


def test_warm_start(hf):
    import torch
    W, H, lam = 257, 130, 19.0
    u, v_direct, _, _ = _case(W, H, lam, "random")
    ls = hf.LargeSteps(W, H, lambda_=lam)
    ls.from_differential(_dev(torch, u))
    cold = ls.last_info()[0]
    exact = _dev(torch, v_direct)
    keep = exact.clone()
    v = ls.from_differential(_dev(torch, u), guess=exact)
    assert ls.last_info()[0] <= 1
    assert torch.equal(exact, keep)                                    # the guess is the caller's: not written
    _check_solution(W, H, lam, v.cpu().numpy(), u, v_direct, what="warm/exact")
    du = R.rhs("random", W, H, seed=99) * np.float32(1e-3 * np.linalg.norm(u) / np.sqrt(u.size))
    u2 = u + du                                                        # perturbed by 1e-3 relative
    v2 = ls.from_differential(_dev(torch, u2), guess=exact)
    warm = ls.last_info()[0]
    print(f"cold {cold} iterations, warm after a 1e-3 step {warm}")
    assert warm < cold
    _check_solution(W, H, lam, v2.cpu().numpy(), u2, what="warm/perturbed")


def test_zero_and_nan_right_hand_sides(hf):
    import torch
    W, H = 33, 17
    ls = hf.LargeSteps(W, H)
    zero = torch.zeros((H, W), device="cuda")
    for guess in (None, torch.full((H, W), 0.75, device="cuda")):
        v = ls.from_differential(zero, guess=guess, check=True)
        assert not v.cpu().numpy().view(np.uint32).any()               # exact zeros
        assert ls.last_info() == (0, 0.0)
    u = _dev(torch, _case(W, H, 19.0, "random")[0]).clone()
    u[5, 7] = float("nan")
    v = ls.from_differential(u)                                        # returns: the launch count is fixed
    it, res = ls.last_info()
    assert it == ls.max_iter and np.isnan(res)
    assert torch.isnan(v).any()
    with pytest.raises(RuntimeError):
        ls.from_differential(u, check=True)


def test_repeatable_and_capturable(hf):
    import torch
    W, H, lam = 257, 130, 19.0
    u = _dev(torch, _case(W, H, lam, "random")[0])
    ls = hf.LargeSteps(W, H, lambda_=lam)
    a = ls.from_differential(u)
    b = ls.from_differential(u)
    assert torch.equal(a, b)                                           # no atomics, one order of every sum
    back = ls.to_differential(a)
    info = ls.last_info()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ls.to_differential(ls.from_differential(u))                    # warm-up on a side stream before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv = ls.from_differential(u)
        gu = ls.to_differential(gv)
    for _ in range(2):
        gv.zero_(); gu.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gv, a) and torch.equal(gu, back)
        assert ls.last_info() == info


def test_autograd(hf):
    import torch
    import torch.autograd.forward_ad as fwAD
    W, H, lam = 33, 17, 19.0
    ls = hf.LargeSteps(W, H, lambda_=lam)
    u_np, w_np = R.rhs("random", W, H, seed=1), R.rhs("random", W, H, seed=2)
    w = _dev(torch, w_np)
    # reverse mode of the solve: d<w, A^-1 u>/du = A^-1 w
    u = _dev(torch, u_np).requires_grad_(True)
    (w * ls.from_differential(u)).sum().backward()
    _check_solution(W, H, lam, u.grad.cpu().numpy(), w_np, what="solve backward")
    # reverse mode of the apply: A w
    v = _dev(torch, u_np).requires_grad_(True)
    (w * ls.to_differential(v)).sum().backward()
    assert np.abs(v.grad.cpu().numpy() - R.apply_f64(W, H, lam, w_np)).max() <= 8 * 2.0 ** -24 * (1 + 12 * lam) * np.abs(w_np).max()
    # forward mode: the tangents go through the same two operators
    with fwAD.dual_level():
        dual = fwAD.make_dual(_dev(torch, u_np), w)
        t_solve = fwAD.unpack_dual(ls.from_differential(dual)).tangent
        t_apply = fwAD.unpack_dual(ls.to_differential(dual)).tangent
    _check_solution(W, H, lam, t_solve.cpu().numpy(), w_np, what="solve jvp")
    assert np.abs(t_apply.cpu().numpy() - R.apply_f64(W, H, lam, w_np)).max() <= 8 * 2.0 ** -24 * (1 + 12 * lam) * np.abs(w_np).max()
    # symmetry: |<solve(a), b> - <a, solve(b)>| <= |b| R_a + |a| R_b
    a64, b64 = u_np.astype(np.float64), w_np.astype(np.float64)
    with torch.no_grad():
        sa = ls.from_differential(_dev(torch, u_np)).cpu().numpy().astype(np.float64)
        sb = ls.from_differential(w).cpu().numpy().astype(np.float64)
    Ra, Rb = R.true_residual(W, H, lam, sa, a64), R.true_residual(W, H, lam, sb, b64)
    assert abs((sa * b64).sum() - (a64 * sb).sum()) <= np.linalg.norm(b64) * Ra + np.linalg.norm(a64) * Rb
    # round trip: from_differential(to_differential(v)) against v itself
    with torch.no_grad():
        lat = ls.to_differential(_dev(torch, u_np))
        rt = ls.from_differential(lat).cpu().numpy()
    _check_solution(W, H, lam, rt, lat.cpu().numpy(), what="round trip")
    _check_solution(W, H, lam, rt, lat.cpu().numpy(), v_direct=u_np.astype(np.float64), what="round trip against v")


def test_preconditioned_loop(hf):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import inverse_heights
    hist, err, _ = inverse_heights.run(grid=32, film=32, steps=5, large_steps=19.0, verbose=False)
    ls, latent, shape = inverse_heights.run.last_large_steps
    h = shape.heightfield.detach()
    assert len(hist) == 5 and np.isfinite(hist).all() and np.isfinite(err) and bool(torch.isfinite(h).all())
    assert ls.lambda_ == 19.0 and tuple(latent.shape) == (32, 32)
    _check_solution(32, 32, 19.0, h.cpu().numpy(), latent.detach().cpu().numpy(), what="loop")
    # the default stays what it was: the heights themselves are the optimised tensor
    inverse_heights.run(grid=32, film=32, steps=1, verbose=False)
    assert inverse_heights.run.last_large_steps is None

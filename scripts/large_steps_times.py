#!/usr/bin/env python3
"""Time large-steps preconditioning (hf_amd.LargeSteps) with HIP events on 1024^2 and 4096^2 grids at lambda = 19:
    apply            to_differential, one stencil launch;
    cold solve       from_differential of a random latent, max_iter 256, tol 1e-6;
    warm solve       the same after a step of 1e-3 (relative) on the latent, started from the previous answer;
    idle launches    what the launches after convergence cost: the cold solve with max_iter 256 against the same solve
                     with max_iter = the iterations it needs;
    torch CG         the same conjugate gradients, the same number of iterations, written with torch slicing (what a user
                     would have written without the kernels): the comparison column.  Its answer is compared first.
usage: python scripts/large_steps_times.py [--warmup 2 --iters 5 --out profiles/large_steps/times.jsonl
       --stats profiles/large_steps/kernel_stats.txt] [--grids 1024 4096] [--stats-only]
One JSON line per measurement (mean / min ms over the timed calls).  `model_gbps` is the traffic the algorithm needs by
its own count -- 11 passes of 4 W H bytes per iteration, 2 per apply -- over the measured time of the WHOLE
call: an end-to-end figure, not a kernel's share of peak.  --stats: registers, LDS, private segment and occupancy of the
hf_large_steps_* kernels, read from the metadata of the library that ran (compiles nothing; --stats-only needs no device)."""
import argparse, json, os, sys
from regs import kernel_stats, occupancy_line
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--grids", type=int, nargs="*", default=[1024, 4096])
ap.add_argument("--out", default=None)
ap.add_argument("--stats", default=None)
ap.add_argument("--stats-only", action="store_true")
a = ap.parse_args()
LAMBDA, MAX_ITER, TOL, STEP = 19.0, 256, 1e-6, 1e-3
PASSES_PER_ITERATION, PASSES_PER_APPLY = 11, 2


import hf_amd  # noqa: E402
if a.stats or a.stats_only:
    text = "\n".join(map(occupancy_line, kernel_stats(hf_amd.build.LIB_PATH, "hf_large_steps")))
    print(text)
    if a.stats:
        os.makedirs(os.path.dirname(os.path.abspath(a.stats)), exist_ok=True)
        open(a.stats, "w").write("hf_large_steps_* kernels of libhf.so (code-object metadata; occupancy from the VGPR count)\n" + text + "\n")
if a.stats_only:
    sys.exit(0)

import torch  # noqa: E402
assert torch.cuda.is_available(), "large_steps_times.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return sum(ms) / len(ms), min(ms)


def report(kind, N, mean, mn, passes=None, **extra):
    rec = dict(kind=kind, grid=N, lambda_=LAMBDA, ms_mean=round(mean, 4), ms_min=round(mn, 4), **extra)
    if passes:
        rec["model_gbps"] = round(passes * 4.0 * N * N / (mn * 1e-3) / 1e9, 1)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n"); out_f.flush()


def torch_apply(v, deg, lam):
    """A v with torch slicing: the neighbours in the kernels' order"""
    p = torch.nn.functional.pad(v, (1, 1, 1, 1))
    H, W = v.shape
    s = p[1:H + 1, 0:W] + p[1:H + 1, 2:W + 2]
    s = s + p[0:H, 1:W + 1]
    s = s + p[2:H + 2, 1:W + 1]
    s = s + p[2:H + 2, 0:W]
    s = s + p[0:H, 2:W + 2]
    return v + lam * (deg * v - s)


def torch_cg(u, deg, lam, iterations):
    """`iterations` steps of conjugate gradients from 0 with no host synchronisation: float32 vectors, float64 dots"""
    x, r = torch.zeros_like(u), u.clone()
    p = r.clone()
    rr = (r.double() * r.double()).sum()
    for _ in range(iterations):
        q = torch_apply(p, deg, lam)
        alpha = (rr / (p.double() * q.double()).sum()).float()
        x = x + alpha * p
        r = r - alpha * q
        rr_new = (r.double() * r.double()).sum()
        p = r + (rr_new / rr).float() * p
        rr = rr_new
    return x


for N in a.grids:
    g = torch.Generator(device=dev); g.manual_seed(N)
    u = torch.rand((N, N), device=dev, generator=g) * 2.0 - 1.0
    ls = hf_amd.LargeSteps(N, N, lambda_=LAMBDA, max_iter=MAX_ITER, tol=TOL)
    with torch.no_grad():
        v = ls.from_differential(u)
        it_cold, res_cold = ls.last_info()
        du = (torch.rand((N, N), device=dev, generator=g) * 2.0 - 1.0) * (STEP * float(u.norm()) / N)
        u2 = u + du
        ls.from_differential(u2, guess=v)
        it_warm, res_warm = ls.last_info()
        ones = torch.ones_like(u)
        deg = torch_apply(ones, torch.zeros_like(u), -1.0) - ones          # v + (-1)(0 v - sum) - v: the neighbour count
        ref = torch_cg(u, deg, LAMBDA, it_cold)
        diff = float((ref - v).norm() / v.norm())
        print(json.dumps(dict(kind="check", grid=N, iterations_cold=it_cold, residual_cold=res_cold, iterations_warm=it_warm,
                              residual_warm=res_warm, rel_diff_torch_cg_vs_kernels=diff)), flush=True)
        assert diff < 1e-4, "the torch conjugate gradients and the kernels disagree"
        exact = hf_amd.LargeSteps(N, N, lambda_=LAMBDA, max_iter=max(1, it_cold), tol=TOL)   # no launch after convergence
        exact.from_differential(u)
        report("apply", N, *timed(lambda: ls.to_differential(u)), passes=PASSES_PER_APPLY)
        c_mean, c_min = timed(lambda: ls.from_differential(u))
        e_mean, e_min = timed(lambda: exact.from_differential(u))
        t_mean, t_min = timed(lambda: torch_cg(u, deg, LAMBDA, it_cold))
        c2_mean, c2_min = timed(lambda: ls.from_differential(u))                # again: both saw the same machine
        w_mean, w_min = timed(lambda: ls.from_differential(u2, guess=v))
        report("solve_cold", N, c_mean, c_min, passes=PASSES_PER_ITERATION * it_cold, iterations=it_cold, residual=res_cold)
        report("solve_cold_again", N, c2_mean, c2_min, passes=PASSES_PER_ITERATION * it_cold, iterations=it_cold)
        report("solve_cold_max_iter_equals_iterations", N, e_mean, e_min, passes=PASSES_PER_ITERATION * it_cold, iterations=it_cold)
        idle = 2 * (MAX_ITER - it_cold)
        report("idle_launches", N, c_mean - e_mean, c_min - e_min, launches=idle,
               us_per_launch=round(1e3 * (c_min - e_min) / max(1, idle), 3))
        report("torch_cg_same_iterations", N, t_mean, t_min, iterations=it_cold, times_the_kernels=round(t_min / e_min, 2))
        report("solve_warm", N, w_mean, w_min, passes=PASSES_PER_ITERATION * it_warm, iterations=it_warm, residual=res_warm)
    del u, u2, du, v, ref, ones, deg, ls, exact
    torch.cuda.empty_cache()

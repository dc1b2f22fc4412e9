#!/usr/bin/env python3
"""Time the reverse pass of reparameterize_ray with gradients for the heights, ray.o, ray.d and to_world (HIP events,
warm-up, median of the timed runs) on a camera wavefront over a field built with hf_amd.workload.  The same script times
any checkout: --root names the repository whose hf_amd is imported (default: this one), --label goes into the record.
usage: python scripts/time_reparam_backward_full.py [--root DIR --label NAME --grid 1024 --film 1024 --spp 4
       --aux 4 16 --warmup 2 --iters 10 --out FILE]   (appends one JSON line per sample count)"""
import argparse, json, os, statistics, sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit")
ap.add_argument("--grid", type=int, default=1024)
ap.add_argument("--film", type=int, default=1024)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--aux", type=int, nargs="*", default=[4, 16])
ap.add_argument("--kappa", type=float, default=1e5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch
import hf_amd

dev = torch.device("cuda", 0)
h = hf_amd.workload.sine_heights(a.grid, a.grid, device=dev)
shape = hf_amd.Heightfield(heightfield=h, max_height=0.5, differentiable_to_world=True)
shape.heightfield.requires_grad_(True)
tw = torch.eye(4, dtype=torch.float64)[:3].clone().requires_grad_(True)
shape.to_world = tw
shape.parameters_changed(["to_world"])
rays = hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)
n = rays.shape[1]
o = rays[0:3].contiguous().requires_grad_(True)
d = rays[3:6].contiguous().requires_grad_(True)
del rays
gen = torch.Generator(device=dev).manual_seed(1)
gdir = torch.randn((3, n), device=dev, generator=gen)
gdiv = torch.randn(n, device=dev, generator=gen)

for K in a.aux:
    def step():
        # (forward is the identity: the time is the backward's)
        dirn, det = hf_amd.reparameterize_ray(shape, hf_amd.Ray3f(o, d), num_rays=K, kappa=a.kappa, exponent=3.0)
        return torch.autograd.grad((dirn, det), (shape.heightfield, o, d, tw), (gdir, gdiv))
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record(); g = step(); e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    rec = dict(commit=a.label, kind="reverse(heights, o, d, to_world)", grid=a.grid, rays=n, aux=K, kappa=a.kappa,
               ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), runs=a.iters,
               grad_to_world_norm=round(float(g[3].norm()), 6), grad_o_norm=round(float(g[1].norm()), 6))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

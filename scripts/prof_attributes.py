#!/usr/bin/env python3
"""Time the shape-attribute kernels on the bench wavefront with HIP events: hf_eval_attribute, _adjoint and _tangent for
a size-3 vertex attribute and a size-1 face attribute, at the hits of the bench's rays (one ray_intersect up front).
usage: python scripts/prof_attributes.py [--grid 4096 --film 8192 --warmup 5 --iters 20
       --out profiles/attributes/times.jsonl]
One JSON line per measurement: mean / min ms over the timed launches and the streamed byte count of DESIGN 4.9 (rows
read or written by every ray, rows read by hits only; the gathered texels come on top, at most once each)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hf_amd

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=8192)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.grid
M = 2 * (N - 1) * (N - 1)
h = hf_amd.workload.sine_heights(N, N, device=dev)
g = torch.Generator(device=dev).manual_seed(0)
shape = hf_amd.Heightfield(heightfield=h, max_height=0.5)
shape.add_attribute("vertex_color", 3, torch.rand(N * N * 3, device=dev, generator=g))
shape.add_attribute("face_mono", 1, torch.rand(M, device=dev, generator=g))
rays = hf_amd.workload.ortho_rays(a.film, a.film, 1, dev)
ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
del rays
with torch.no_grad():
    si = shape.ray_intersect(ray, hf_amd.RayFlags.Minimal)
n = len(ray)
p, prim, t = shape._attr_si(si)
hits = int(torch.isfinite(t).sum())
del si, ray
torch.cuda.empty_cache()
out_f = open(a.out, "w") if a.out else None


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


def report(kind, name, mean, mn, nbytes):
    rec = dict(kind=kind, attribute=name, grid=N, rays=n, hits=hits, ms_mean=round(mean, 4), ms_min=round(mn, 4),
               bytes=nbytes, GB_per_s=round(nbytes / mean / 1e6, 1))
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n")


for name, size, vertex in (("vertex_color", 3, True), ("face_mono", 1, False)):
    attr = shape.attributes[name]
    # DESIGN 4.9's count: every ray reads t (4 B) and writes its rows; only a hit reads prim_index (4 B) and, for a vertex
    # attribute, p (12 B).  The gathered texels (heights, attribute values) come on top, at most once each
    per_hit = 4 + (12 if vertex else 0)
    mean, mn = timed(lambda: shape._attr_forward_raw(name, attr, p, prim, t, None))
    report("forward", name, mean, mn, n * (4 + 4 * size) + hits * per_hit)
    gout = torch.randn((size, n), device=dev, generator=g)
    ga = torch.zeros_like(attr)
    gh = torch.zeros((N, N), device=dev)
    # every ray: t, and dL/dp written (vertex attributes); a hit also reads its upstream rows; the scatters come on top
    mean, mn = timed(lambda: shape._attr_adjoint_raw(name, attr, p, prim, t, None, gout, grad_attr=ga, grad_h=gh))
    report("adjoint", name, mean, mn, n * (4 + (12 if vertex else 0)) + hits * (per_hit + 4 * size))
    da = torch.randn_like(attr)
    dp = torch.randn((3, n), device=dev, generator=g) if vertex else None
    dh = torch.randn((N, N), device=dev, generator=g)
    # every ray: t and the size tangent rows; a hit also reads the tangent of p
    mean, mn = timed(lambda: shape._attr_tangent_raw(name, attr, p, prim, t, None, da, dp, dh))
    report("tangent", name, mean, mn, n * (4 + 4 * size) + hits * (per_hit + (12 if vertex else 0)))
    del gout, ga, gh, da, dp, dh
    torch.cuda.empty_cache()

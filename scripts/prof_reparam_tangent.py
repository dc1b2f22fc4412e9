#!/usr/bin/env python3
"""Time the forward mode of reparameterize_ray on the bench field and wavefront with HIP events: hf_reparam_tangent alone
(heights tangent; heights + ray + to_world tangents), hf_reparam_trace_all, the whole forward-mode step
(reparameterize_ray_tangent = trace_all + tangent) and, next to it, the reverse-mode step (reparameterize_ray +
backward, heights only: trace_all + hf_reparam_backward).
usage: python scripts/prof_reparam_tangent.py [--grid 4096 --film 4096 --spp 4 --aux 4 16 --warmup 3 --iters 10
       --out profiles/reparam_tangent/times.jsonl]
One JSON line per measurement: mean / min ms over the timed runs and, for the tangent kernel, the bytes it must move
(24 B of ray, 20 B of records per sample, 16 B of output per ray) and the fraction of the 8 TB/s roofline."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hf_amd
from hf_amd import _capi
from hf_amd import shape as sh

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=4096)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--aux", type=int, nargs="*", default=[4, 16])
ap.add_argument("--kappa", type=float, default=1e5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ROOFLINE = 8e12
lib = _capi.lib()
h = hf_amd.workload.sine_heights(a.grid, a.grid, device=dev)
shape = hf_amd.Heightfield(heightfield=h, max_height=0.5)
rays = hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)
n = rays.shape[1]
o, d = rays[0:3].contiguous(), rays[3:6].contiguous()
del rays
ray = hf_amd.Ray3f(o, d)
stream = torch.cuda.current_stream(dev).cuda_stream
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


def report(kind, mean, mn, nbytes=None, **extra):
    rec = dict(kind=kind, grid=a.grid, rays=n, ms_mean=round(mean, 4), ms_min=round(mn, 4), **extra)
    if nbytes:
        rec.update(bytes=nbytes, GB_per_s=round(nbytes / mean / 1e6, 1), roofline_ms=round(nbytes / ROOFLINE * 1e3, 4),
                   roofline_fraction=round(nbytes / ROOFLINE * 1e3 / mn, 3))
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n")


dh = torch.randn((a.grid, a.grid), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
gdir = torch.randn((3, n), device=dev); gdv = torch.randn(n, device=dev)
for K in a.aux:
    # the kept records, as reparameterize_ray_tangent lays them out: [K][bt, t, u, v, prim][n]
    store = torch.empty((K, 5, n), dtype=torch.float32, device=dev)
    rows = [store[0, r].data_ptr() for r in range(5)]
    si_s = _capi.hf_si_t(); si_s.boundary_test = rows[0]
    pi_s = _capi.hf_pi_t()
    pi_s.t, pi_s.prim_uv[0], pi_s.prim_uv[1], pi_s.prim_index = rows[1], rows[2], rows[3], rows[4]
    o_p, d_p = sh._p3(o), sh._p3(d)
    trace = lambda: _capi.check(lib.hf_reparam_trace_all(shape._h, n, C.byref(o_p), C.byref(d_p), None, K, a.kappa, 0, 0,
                                                          None, C.byref(pi_s), C.byref(si_s), 5 * n, stream))
    trace(); torch.cuda.synchronize()
    hits = float(torch.isfinite(store[:, 1]).float().mean())
    ray_hit = float(torch.isfinite(store[:, 1]).any(0).float().mean())
    mean, mn = timed(trace)
    report("trace_all", mean, mn, aux=K, kappa=a.kappa, sample_hit_fraction=round(hits, 4))
    out_dir = torch.empty((3, n), device=dev); out_div = torch.empty(n, device=dev)
    od_p = sh._p3(out_dir)
    dd = torch.randn((3, n), device=dev) * 1e-2
    dtw = torch.randn(12, device=dev) * 1e-2

    def tangent(dhp, ddp=None, dtwp=None):
        _capi.check(lib.hf_reparam_tangent(shape._h, n, C.byref(o_p), C.byref(d_p), None, K, a.kappa, 3.0, 0, 0, None,
                                           C.byref(pi_s), rows[0], 5 * n, dhp, ddp, ddp, dtwp, C.byref(od_p),
                                           out_div.data_ptr(), stream))
    # per ray: d (12 B), o (12 B, rays with a hit), pi.t per sample (4 B), bt/u/v/prim per hit sample (16 B), 16 B out;
    # the gathered heights stay in the Infinity Cache / L2 and are not counted
    nbytes = int(n * (12 + 12 * ray_hit + 4 * K + 16 * K * hits + 16))
    mean, mn = timed(lambda: tangent(dh.data_ptr()))
    report("tangent(heights)", mean, mn, nbytes, aux=K, kappa=a.kappa)
    dd_p = C.byref(sh._p3(dd))
    mean, mn = timed(lambda: tangent(dh.data_ptr(), dd_p, dtw.data_ptr()))
    # + d_o, d_d (24 B per ray)
    report("tangent(heights, ray, to_world)", mean, mn, nbytes + 24 * n, aux=K, kappa=a.kappa)
    del store, out_dir, out_div, dd
    torch.cuda.empty_cache()
    mean, mn = timed(lambda: hf_amd.reparameterize_ray_tangent(shape, ray, dheights=dh, num_rays=K, kappa=a.kappa))
    report("forward_step(trace_all + tangent)", mean, mn, aux=K, kappa=a.kappa)
    torch.cuda.empty_cache()
    shape.heightfield.requires_grad_(True)

    def reverse():
        shape.heightfield.grad = None
        dd_, det = hf_amd.reparameterize_ray(shape, ray, num_rays=K, kappa=a.kappa, exponent=3.0)
        torch.autograd.backward((dd_, det), (gdir, gdv))
    mean, mn = timed(reverse)
    report("reverse_step(trace_all + backward)", mean, mn, aux=K, kappa=a.kappa)
    shape.heightfield.requires_grad_(False)
    shape.heightfield.grad = None
    torch.cuda.empty_cache()

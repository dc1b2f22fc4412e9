#!/usr/bin/env python3
"""Time sky lighting with HIP events: the fused forward (hf_sky_lighting), its adjoint and tangent, and the composition
that gives the same image without it -- torch directions, si.spawn_ray, ray_test(coherent=False) once per direction,
a torch reduction -- on two scenes:
    a 2048^2 sine field under a 2048 x 2048 x 1 wavefront, 8 directions per sample;
    the 4096^2 bench field under the bench wavefront (1024 x 1024 x 64), 4 directions per sample.
usage: python scripts/sky_times.py [--warmup 2 --iters 5 --out profiles/sky/times.jsonl --stats profiles/sky/kernel_stats.txt]
       [--scenes 0 1] [--stats-only]
One JSON line per measurement (mean / min ms over the timed calls; the composition's image is compared with the fused
one first).  --stats: registers, LDS, private segment and occupancy of the hf_sky_* kernels, read from the metadata of
the library that ran (compiles nothing; --stats-only needs no device)."""
import argparse, json, math, os, sys
from regs import kernel_stats, occupancy_line
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--scenes", type=int, nargs="*", default=[0, 1])
ap.add_argument("--out", default=None)
ap.add_argument("--stats", default=None)
ap.add_argument("--stats-only", action="store_true")
a = ap.parse_args()
SCENES = [dict(grid=2048, film=2048, spp=1, K=8), dict(grid=4096, film=1024, spp=64, K=4)]
SEED, L, ALBEDO = 3, 1.0, 0.8


import hf_amd  # noqa: E402
if a.stats or a.stats_only:
    text = "\n".join(map(occupancy_line, kernel_stats(hf_amd.build.LIB_PATH, "hf_sky")))
    print(text)
    if a.stats:
        os.makedirs(os.path.dirname(os.path.abspath(a.stats)), exist_ok=True)
        open(a.stats, "w").write("hf_sky_* kernels of libhf.so (code-object metadata; occupancy from the VGPR count)\n" + text + "\n")
if a.stats_only:
    sys.exit(0)

import torch  # noqa: E402
assert torch.cuda.is_available(), "sky_times.py measures on a HIP device; there is none"
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


def report(kind, scene, mean, mn, **extra):
    rec = dict(kind=kind, **scene, ms_mean=round(mean, 4), ms_min=round(mn, 4), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n"); out_f.flush()


def composition(shape, si, ray, keys, K, spp):
    """the image of hf_sky_lighting from what the library offered before it: one materialised ray wavefront, one
    incoherent any-hit launch and one byte of visibility per direction"""
    n = len(ray)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    sn = si.sh_frame.n
    el = si.is_valid() & (-(sn * ray.d).sum(0) > 0)
    acc = torch.zeros(n, device=dev)
    for k in range(K):
        r0, r1 = hf_amd.workload.tea32(torch.full_like(ids, keys[k]), ids)
        sx = (r0 >> 9).to(torch.float32) * (1.0 / (1 << 23)); sy = (r1 >> 9).to(torch.float32) * (1.0 / (1 << 23))
        z = 1.0 - 2.0 * sy
        r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
        w = torch.stack([r * torch.cos(2.0 * math.pi * sx), r * torch.sin(2.0 * math.pi * sx), z])
        co = (sn * w).sum(0)
        tr = el & (co > 0)
        hit = shape.ray_test(si.spawn_ray(w), active=tr, coherent=False)
        acc += torch.where(tr & ~hit, co, torch.zeros_like(co))
    return (acc * (4.0 * ALBEDO * L / K)).reshape(-1, spp).mean(1)


for s in a.scenes:
    scene = SCENES[s]
    N, film, spp, K = scene["grid"], scene["film"], scene["spp"], scene["K"]
    shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(N, N, device=dev), max_height=0.5)
    rays = hf_amd.workload.ortho_rays(film, film, spp, dev)
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    n = len(ray)
    keys = [int(hf_amd.workload.tea32(torch.tensor([SEED]), torch.tensor([k]))[0]) for k in range(K)]
    kw = dict(radiance=L, albedo=ALBEDO, spp=spp, num_rays=K, seed=SEED)
    with torch.no_grad():
        img, vis = hf_amd.sky_lighting(shape, si, ray, return_visibility=True, **kw)
        ref = composition(shape, si, ray, keys, K, spp)
    # (the composition draws its directions with torch's float32 cos / sin: a grazing ray's answer, or the sign of a cosine
    # that is zero to rounding, can differ from the kernel's, and one direction is 1 / K of a sample's value)
    diff = float((img - ref).abs().max())
    differing = int(((img - ref).abs() > 1e-4).sum())
    traced = int(sum(int(((vis >> k) & 1).sum()) for k in range(K)))
    info = dict(samples=n, hits=int(si.is_valid().sum()), visible_directions=traced, image_max=float(img.max()),
                max_abs_diff_fused_vs_composition=diff, pixels_differing_by_more_than_1e_4=differing)
    print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
    assert differing <= 1e-4 * img.numel(), "the composition and the fused kernel disagree"
    with torch.no_grad():
        # alternate the two forwards so that both see the same machine
        f_mean, f_min = timed(lambda: hf_amd.sky_lighting(shape, si, ray, **kw))
        c_mean, c_min = timed(lambda: composition(shape, si, ray, keys, K, spp))
        f2_mean, f2_min = timed(lambda: hf_amd.sky_lighting(shape, si, ray, **kw))
    report("fused_forward", scene, f_mean, f_min, **info)
    report("composition_forward", scene, c_mean, c_min)
    report("fused_forward_again", scene, f2_mean, f2_min)
    # adjoint and tangent: the C entries on the saved visibility words (what the autograd Function calls)
    import ctypes as C
    from hf_amd import _capi
    lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    p3 = lambda x: C.byref((C.c_void_p * 3)(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(3)]))
    sn, dd, tt = si.sh_frame.n.detach().contiguous(), ray.d.contiguous(), si.t.detach().contiguous()
    gi = torch.randn(n // spp, device=dev); gn = torch.empty_like(sn); dimg = torch.empty(n // spp, device=dev)
    dn = torch.randn_like(sn)
    adj = lambda: _capi.check(lib.hf_sky_lighting_adjoint(n, spp, p3(sn), p3(dd), tt.data_ptr(), None, K, SEED, None, L, ALBEDO,
                                                          vis.data_ptr(), gi.data_ptr(), p3(gn), None, stream))
    tan = lambda: _capi.check(lib.hf_sky_lighting_tangent(n, spp, p3(sn), p3(dd), tt.data_ptr(), None, K, SEED, None, L, ALBEDO,
                                                          vis.data_ptr(), p3(dn), None, dimg.data_ptr(), stream))
    report("adjoint", scene, *timed(adj))
    report("tangent", scene, *timed(tan))
    del shape, rays, ray, si, img, vis, ref, sn, dd, tt, gi, gn, dimg, dn
    torch.cuda.empty_cache()

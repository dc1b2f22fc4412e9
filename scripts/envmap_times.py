#!/usr/bin/env python3
"""Time environment-map lighting with HIP events: the fused forward (hf_envmap_lighting), its adjoint (with and without
the texel gradient), its tangent and the table build, and the composition that gives the same image without the fused
kernel -- torch draws from the same table, si.spawn_ray, ray_test(coherent=False) once per direction, a torch
reduction -- on the two scenes of scripts/sky_times.py under a 257 x 128 map:
    a 2048^2 sine field under a 2048 x 2048 x 1 wavefront, 8 directions per sample;
    the 4096^2 bench field under the bench wavefront (1024 x 1024 x 64), 4 directions per sample.
usage: python scripts/envmap_times.py [--warmup 2 --iters 5 --out profiles/envmap_lighting/times.jsonl
       --stats profiles/envmap_lighting/kernel_stats.txt] [--scenes 0 1] [--stats-only]
One JSON line per measurement (mean / min ms over the timed calls; the composition's image is compared with the fused
one first; the fused forward is timed before and after the composition).  --stats: registers, LDS, private segment and
occupancy of the hf_envmap_* kernels, read from the metadata of the library that ran (compiles nothing; --stats-only
needs no device)."""
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
SEED, ALBEDO, MAP_W, MAP_H, DEFENSIVE = 3, 0.8, 257, 128, 0.1


import hf_amd  # noqa: E402
if a.stats or a.stats_only:
    text = "\n".join(map(occupancy_line, kernel_stats(hf_amd.build.LIB_PATH, "hf_envmap")))
    print(text)
    if a.stats:
        os.makedirs(os.path.dirname(os.path.abspath(a.stats)), exist_ok=True)
        open(a.stats, "w").write("hf_envmap_* kernels of libhf.so (code-object metadata; occupancy from the VGPR count)\n" + text + "\n")
if a.stats_only:
    sys.exit(0)

import torch  # noqa: E402
assert torch.cuda.is_available(), "envmap_times.py measures on a HIP device; there is none"
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
    rec = dict(kind=kind, **scene, map=[MAP_W, MAP_H], ms_mean=round(mean, 4), ms_min=round(mn, 4), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n"); out_f.flush()


def sky_map():
    """[MAP_H, MAP_W - 1]: an overcast gradient and a sun of a few texels"""
    th = math.pi * torch.arange(MAP_H, device=dev)[:, None] / (MAP_H - 1)
    ph = 2.0 * math.pi * (torch.arange(MAP_W - 1, device=dev)[None, :] + 0.5) / (MAP_W - 1)
    m = torch.clamp(0.3 + 0.7 * torch.cos(th), min=0.02) * (1.0 + 0.3 * torch.cos(ph))
    return (m + 200.0 * torch.exp(-(((th - 0.9) / 0.05) ** 2 + ((ph - 2.0) / 0.05) ** 2))).to(torch.float32).contiguous()


def composition(shape, si, ray, env, keys, K, spp):
    """the image of hf_envmap_lighting from what the library offered before it: torch draws from the same table, one
    materialised ray wavefront, one incoherent any-hit launch and one byte of visibility per direction"""
    n = len(ray)
    W, H = env.resolution
    data, table = env.full().detach(), env.table()
    sigma, mbar, u = table[0], table[1], table[2]
    M = table[4:4 + H - 1].contiguous(); Cc = table[4 + H - 1:].reshape(H - 1, W - 1)
    rmax = float(Cc[:, -1].max())
    flat = (Cc.double() + 2.0 * rmax * torch.arange(H - 1, device=dev, dtype=torch.float64)[:, None]).reshape(-1).contiguous()
    p = data.clamp(min=0.0)
    mc = 0.25 * ((p[:-1, :-1] + p[:-1, 1:]) + (p[1:, :-1] + p[1:, 1:]))
    rs = torch.sin(math.pi * (torch.arange(H - 1, device=dev, dtype=torch.float64) + 0.5) / (H - 1)).float()
    wcell = rs[:, None] * ((1.0 - u) * mc + u * mbar)
    R = env.to_world.to(dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    sn = si.sh_frame.n
    el = si.is_valid() & (-(sn * ray.d).sum(0) > 0)
    acc = torch.zeros(n, device=dev)
    top = 1.0 - 2.0 ** -24
    for k in range(K):
        r0, r1 = hf_amd.workload.tea32(torch.full_like(ids, keys[k]), ids)
        sx = (r0 >> 9).to(torch.float32) * (1.0 / (1 << 23)); sy = (r1 >> 9).to(torch.float32) * (1.0 / (1 << 23))
        y = sy * sigma
        cy = torch.searchsorted(M, y).clamp(max=H - 2)
        rowsum = Cc[cy, W - 2]
        fy = ((y - torch.where(cy > 0, M[(cy - 1).clamp(min=0)], torch.zeros_like(y))) / rowsum).clamp(0.0, top)
        x = sx * rowsum
        cx = (torch.searchsorted(flat, x.double() + 2.0 * rmax * cy.double()) - cy * (W - 1)).clamp(0, W - 2)
        wc = wcell[cy, cx]
        fx = ((x - torch.where(cx > 0, Cc[cy, (cx - 1).clamp(min=0)], torch.zeros_like(x))) / wc).clamp(0.0, top)
        th = math.pi * (cy + fy) / (H - 1); ph = 2.0 * math.pi * (cx + (fx + 0.5)) / (W - 1)
        st = torch.sin(th)
        w = R @ torch.stack([st * torch.sin(ph), torch.cos(th), -st * torch.cos(ph)])
        Lk = (1 - fy) * ((1 - fx) * data[cy, cx] + fx * data[cy, cx + 1]) + fy * ((1 - fx) * data[cy + 1, cx] + fx * data[cy + 1, cx + 1])
        Ek = Lk * (2.0 * math.pi ** 2) * st * sigma / (wc * ((W - 1) * (H - 1)))
        co = (sn * w).sum(0)
        tr = el & (wc > 0) & (co > 0)
        hit = shape.ray_test(si.spawn_ray(w), active=tr, coherent=False)
        acc += torch.where(tr & ~hit, co * Ek, torch.zeros_like(co))
    return (acc * (ALBEDO / (math.pi * K))).reshape(-1, spp).mean(1)


for s in a.scenes:
    scene = SCENES[s]
    N, film, spp, K = scene["grid"], scene["film"], scene["spp"], scene["K"]
    shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(N, N, device=dev), max_height=0.5)
    rays = hf_amd.workload.ortho_rays(film, film, spp, dev)
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    n = len(ray)
    env = hf_amd.Envmap(sky_map(), defensive=DEFENSIVE)
    keys = [int(hf_amd.workload.tea32(torch.tensor([SEED]), torch.tensor([k]))[0]) for k in range(K)]
    kw = dict(albedo=ALBEDO, spp=spp, num_rays=K, seed=SEED)
    with torch.no_grad():
        img, vis = hf_amd.envmap_lighting(shape, si, ray, env, return_visibility=True, **kw)
        ref = composition(shape, si, ray, env, keys, K, spp)
    # (the composition draws with torch's float32 sin / cos: a draw on a cell border, a grazing ray's answer or the sign of
    # a cosine that is zero to rounding can differ from the kernel's, and one direction is 1 / K of a sample's value)
    diff = float((img - ref).abs().max())
    differing = int(((img - ref).abs() > 1e-3 * float(img.max())).sum())
    traced = int(sum(int(((vis >> k) & 1).sum()) for k in range(K)))
    info = dict(samples=n, hits=int(si.is_valid().sum()), visible_directions=traced, image_max=float(img.max()),
                image_mean=float(img.mean()), max_abs_diff_fused_vs_composition=diff,
                pixels_differing_by_more_than_1e_3_of_max=differing)
    print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
    assert differing <= 1e-3 * img.numel(), "the composition and the fused kernel disagree"
    with torch.no_grad():
        # alternate the two forwards so that both see the same machine
        f_mean, f_min = timed(lambda: hf_amd.envmap_lighting(shape, si, ray, env, **kw))
        c_mean, c_min = timed(lambda: composition(shape, si, ray, env, keys, K, spp))
        f2_mean, f2_min = timed(lambda: hf_amd.envmap_lighting(shape, si, ray, env, **kw))
        s_mean, s_min = timed(lambda: hf_amd.sky_lighting(shape, si, ray, radiance=1.0, **kw))
    report("fused_forward", scene, f_mean, f_min, **info)
    report("composition_forward", scene, c_mean, c_min)
    report("fused_forward_again", scene, f2_mean, f2_min)
    report("sky_forward_same_wavefront", scene, s_mean, s_min)
    # adjoint, tangent and the table build: the C entries on the saved visibility words (what the autograd Function calls)
    import ctypes as C
    from hf_amd import _capi
    lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
    p3 = lambda x: C.byref((C.c_void_p * 3)(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(3)]))
    sn, dd, tt = si.sh_frame.n.detach().contiguous(), ray.d.contiguous(), si.t.detach().contiguous()
    gi = torch.randn(n // spp, device=dev); gn = torch.empty_like(sn); dimg = torch.empty(n // spp, device=dev)
    dn = torch.randn_like(sn)
    dat, table, rot = env.full().detach().contiguous(), env.table(), C.byref(env._rot)
    gd = torch.zeros_like(dat); ddat = torch.randn_like(dat); table2 = torch.empty_like(table)
    head = (n, spp, p3(sn), p3(dd), tt.data_ptr(), None, K, SEED, None, MAP_W, MAP_H, dat.data_ptr(), table.data_ptr(), rot, ALBEDO,
            vis.data_ptr())
    adj = lambda g: (lambda: _capi.check(lib.hf_envmap_lighting_adjoint(*head, gi.data_ptr(), p3(gn), None, g, stream)))
    tan = lambda d: (lambda: _capi.check(lib.hf_envmap_lighting_tangent(*head, p3(dn), None, d, dimg.data_ptr(), stream)))
    report("adjoint_sh_n", scene, *timed(adj(None)))
    report("adjoint_sh_n_and_texels", scene, *timed(adj(gd.data_ptr())))
    report("tangent_sh_n", scene, *timed(tan(None)))
    report("tangent_sh_n_and_texels", scene, *timed(tan(ddat.data_ptr())))
    report("table_build", scene, *timed(lambda: _capi.check(lib.hf_envmap_build_table(MAP_W, MAP_H, dat.data_ptr(), DEFENSIVE,
                                                                                        table2.data_ptr(), stream))))
    del shape, rays, ray, si, img, vis, ref, sn, dd, tt, gi, gn, dimg, dn
    torch.cuda.empty_cache()

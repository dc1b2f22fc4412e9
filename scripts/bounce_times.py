#!/usr/bin/env python3
"""Time bounce lighting with HIP events: the fused forward (hf_bounce_lighting), its adjoint and tangent, and the
composition that gives the same image without it -- torch directions, si.spawn_ray, ray_intersect(coherent=False), one
ray_test per light, direct_lighting(spp=1, vis=...) at the hits, a torch reduction -- on two scenes:
    a 2048^2 sine field under a 2048 x 2048 x 1 wavefront, 4 directions per sample, 2 lights;
    the 4096^2 bench field under the bench wavefront (1024 x 1024 x 64), 2 directions per sample, 2 lights.
usage: python scripts/bounce_times.py [--warmup 2 --iters 5 --out profiles/bounce_lighting/times.jsonl
       --stats profiles/bounce_lighting/kernel_stats.txt] [--scenes 0 1] [--stats-only] [--forward-only] [--limit 300]
Every scene is measured by a child process of its own under a time limit (--limit seconds); the first child that
fails or runs out of time ends the script.  One JSON line per measurement (mean / min ms over the timed calls; the
composition's image is compared with the fused one first, and the fused forward is timed before and after the
composition).  --stats: registers, LDS, private segment and occupancy of the hf_bounce_* kernels, read from the
metadata of the library that ran (HF_LIB or the in-tree build; compiles nothing; --stats-only needs no device)."""
import argparse, json, math, os, subprocess, sys
from regs import kernel_stats, occupancy_line
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--scenes", type=int, nargs="*", default=[0, 1])
ap.add_argument("--out", default=None)
ap.add_argument("--stats", default=None)
ap.add_argument("--stats-only", action="store_true")
ap.add_argument("--forward-only", action="store_true", help="the fused forward alone (A/B of library variants)")
ap.add_argument("--limit", type=int, default=300, help="seconds a scene's child process may take")
ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
a = ap.parse_args()
SCENES = [dict(grid=2048, film=2048, spp=1, K=4), dict(grid=4096, film=1024, spp=64, K=2)]
SEED, ALBEDO = 3, 0.8
LIGHTS = [[0.3, 0.2, 0.9, 1.0], [-0.5, 0.4, 0.6, 0.7]]


if a.child is None:
    # ---- the parent: touches no device; one child per scene, each under its own time limit ----
    import hf_amd  # noqa: E402
    lib_path = os.environ.get("HF_LIB") or hf_amd.build.LIB_PATH
    if a.stats or a.stats_only:
        text = "\n".join(map(occupancy_line, kernel_stats(lib_path, "hf_bounce")))
        print(text)
        if a.stats:
            os.makedirs(os.path.dirname(os.path.abspath(a.stats)), exist_ok=True)
            open(a.stats, "w").write("hf_bounce_* kernels of " + os.path.basename(lib_path) +
                                     " (code-object metadata; occupancy from the VGPR count)\n" + text + "\n")
    if a.stats_only:
        sys.exit(0)
    out_f = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out_f = open(a.out, "w")
    for s in a.scenes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(s), "--warmup", str(a.warmup), "--iters", str(a.iters)]
        if a.forward_only:
            cmd.append("--forward-only")
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"scene {s}: no result within {a.limit} s; stopping")
        sys.stdout.write(r.stdout); sys.stdout.flush()
        if out_f:
            out_f.write(r.stdout); out_f.flush()
        if r.returncode != 0:
            sys.exit(f"scene {s}: the measurement failed (exit status {r.returncode}); stopping")
    sys.exit(0)

# ---- a child: one scene ----
import torch  # noqa: E402
import hf_amd  # noqa: E402
assert torch.cuda.is_available(), "bounce_times.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)


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
    print(json.dumps(dict(kind=kind, **scene, ms_mean=round(mean, 4), ms_min=round(mn, 4), **extra)), flush=True)


def composition(shape, si, ray, lights, keys, K, spp):
    """the image of hf_bounce_lighting from what the library offered before it: per direction a materialised ray
    wavefront, an incoherent closest-hit launch with its surface interactions, a shadow wavefront and an any-hit
    launch per light, the direct-lighting kernel at the hits"""
    n = len(ray)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    sn = si.sh_frame.n
    el = si.is_valid() & (-(sn * ray.d).sum(0) > 0)
    fs, ft = hf_amd.shape._coordinate_system(sn)
    acc = torch.zeros((len(lights), n), device=dev)
    for k in range(K):
        r0, r1 = hf_amd.workload.tea32(torch.full_like(ids, keys[k]), ids)
        x = 2.0 * ((r0 >> 9).to(torch.float32) * (1.0 / (1 << 23))) - 1.0
        y = 2.0 * ((r1 >> 9).to(torch.float32) * (1.0 / (1 << 23))) - 1.0
        q13 = x.abs() < y.abs()
        r, rp = torch.where(q13, y, x), torch.where(q13, x, y)
        phi = torch.where(r != 0, (0.25 * math.pi) * rp / r, torch.zeros_like(r))
        phi = torch.where(q13, 0.5 * math.pi - phi, phi)
        px, py = r * torch.cos(phi), r * torch.sin(phi)
        z = torch.sqrt((1.0 - r.abs()) * (1.0 + r.abs()))
        w = fs * px + ft * py + sn * z
        tr = el & (z > 0)
        bray = si.spawn_ray(w)
        si2 = shape.ray_intersect(bray, hf_amd.RayFlags.All, active=tr, coherent=False)
        front = si2.is_valid() & (-(si2.n * w).sum(0) > 0)
        vis = torch.stack([~shape.ray_test(si2.spawn_ray(l[:3].to(dev)), active=front & ((si2.n * l[:3, None].to(dev)).sum(0) > 0),
                                           coherent=False) for l in lights]).to(torch.uint8)
        acc += hf_amd.direct_lighting(si2, bray, lights, albedo=ALBEDO, spp=1, vis=vis)
    return (acc * (ALBEDO / K)).reshape(len(lights), -1, spp).mean(2)


scene = SCENES[a.child]
N, film, spp, K = scene["grid"], scene["film"], scene["spp"], scene["K"]
lights = torch.tensor(LIGHTS)
lights[:, :3] /= lights[:, :3].norm(dim=1, keepdim=True)
shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(N, N, device=dev), max_height=0.5)
rays = hf_amd.workload.ortho_rays(film, film, spp, dev)
ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
with torch.no_grad():
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
n = len(ray)
kw = dict(albedo=ALBEDO, spp=spp, num_rays=K, seed=SEED)
if a.forward_only:
    with torch.no_grad():
        report("fused_forward", scene, *timed(lambda: hf_amd.bounce_lighting(shape, si, ray, lights, **kw)),
               lib=os.path.basename(os.environ.get("HF_LIB") or hf_amd.build.LIB_PATH))
    sys.exit(0)
keys = [int(hf_amd.workload.tea32(torch.tensor([SEED]), torch.tensor([k]))[0]) for k in range(K)]
with torch.no_grad():
    img, prim, lit = hf_amd.bounce_lighting(shape, si, ray, lights, return_records=True, **kw)
    ref = composition(shape, si, ray, lights, keys, K, spp)
# (the composition draws its directions with torch's float32 cos / sin: a grazing ray's answer, or the sign of a cosine
# that is zero to rounding, can differ from the kernel's, and one direction is 1 / K of a sample's value)
diff = float((img - ref).abs().max())
differing = int(((img - ref).abs() > 1e-4).sum())
info = dict(samples=n, hits=int(si.is_valid().sum()), bounce_hits=int((prim != -1).sum()),
            lit=[int(((lit >> l) & 1).sum()) for l in range(len(lights))], image_max=float(img.max()),
            max_abs_diff_fused_vs_composition=diff, pixels_differing_by_more_than_1e_4=differing)
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert differing <= 1e-4 * img.numel(), "the composition and the fused kernel disagree"
with torch.no_grad():
    # the fused forward before and after the composition, so that both see the same machine
    f_mean, f_min = timed(lambda: hf_amd.bounce_lighting(shape, si, ray, lights, **kw))
    c_mean, c_min = timed(lambda: composition(shape, si, ray, lights, keys, K, spp))
    f2_mean, f2_min = timed(lambda: hf_amd.bounce_lighting(shape, si, ray, lights, **kw))
report("fused_forward", scene, f_mean, f_min, **info)
report("composition_forward", scene, c_mean, c_min)
report("fused_forward_again", scene, f2_mean, f2_min)
# adjoint and tangent: the C entries on the saved record (what the autograd Function calls)
import ctypes as C  # noqa: E402
from hf_amd import _capi  # noqa: E402
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
p3 = lambda x: C.byref((C.c_void_p * 3)(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(3)]))
Lc = (_capi.hf_dir_light_t * len(lights))()
for j, row in enumerate(lights.tolist()):
    Lc[j].to_light[0], Lc[j].to_light[1], Lc[j].to_light[2], Lc[j].irradiance = row
sn, dd, tt = si.sh_frame.n.detach().contiguous(), ray.d.contiguous(), si.t.detach().contiguous()
npix = n // spp
gi = torch.randn(len(lights) * npix, device=dev); gn = torch.empty_like(sn); dimg = torch.empty(len(lights) * npix, device=dev)
dn = torch.randn_like(sn); gh = shape._zero_heights(); dh = torch.randn_like(gh)
head = (shape._h, n, spp, p3(sn), p3(dd), tt.data_ptr(), None, K, SEED, None, len(lights), Lc, ALBEDO, prim.data_ptr(),
        lit.data_ptr(), n)
adj = lambda: _capi.check(lib.hf_bounce_lighting_adjoint(*head, gi.data_ptr(), p3(gn), None, gh.data_ptr(), stream))
adj_n = lambda: _capi.check(lib.hf_bounce_lighting_adjoint(*head, gi.data_ptr(), p3(gn), None, None, stream))
tan = lambda: _capi.check(lib.hf_bounce_lighting_tangent(*head, p3(dn), None, dh.data_ptr(), dimg.data_ptr(), stream))
report("adjoint", scene, *timed(adj))
report("adjoint_without_heights", scene, *timed(adj_n))
report("tangent", scene, *timed(tan))

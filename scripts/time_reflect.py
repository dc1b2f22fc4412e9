#!/usr/bin/env python3
"""Time the reflection row with HIP events on the benchmark's wavefront (the 4096^2 sine field under 1024 x 1024 x 64 =
67.1 M samples; an ideal mirror, eta 0, under map_gradient-like 33 x 17 texels):
    the fused launch (hf_reflect_lighting: image, value and visibility);
    hf_envmap_lighting with num_rays = 1 on the same wavefront: that launch also does one any-hit walk per sample (its
      device code is the parent commit's, instruction for instruction: profiles/reflect/registers.txt);
    the two-call sequence hf_reflect_rays + hf_ray_test with the incoherent hint (ray_test(coherent=False));
    the adjoint (with and without grad_data) and the tangent on the visibility the forward wrote.
usage: python scripts/time_reflect.py [--warmup 2 --iters 10 --out profiles/reflect/times.jsonl] [--grid 4096 --film 1024 --spp 64]
One JSON line per measurement (median / min / mean ms over the timed calls).  The fused visibility is compared with the
two-call answer first.  A record, not a pass criterion."""
import argparse, ctypes as C, json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ETA = 0.0

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_reflect.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, eta=ETA, map="33x17")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def report(kind, ms, **extra):
    rec = dict(kind=kind, **scene, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4),
               ms_mean=round(sum(ms) / len(ms), 4), iters=len(ms), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n"); out_f.flush()


shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(a.grid, a.grid, device=dev), max_height=0.5)
rays = hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)
ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
with torch.no_grad():
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
n = len(ray)
th = math.pi * torch.arange(17, device=dev, dtype=torch.float32)[:, None] / 16
ph = 2.0 * math.pi * (torch.arange(32, device=dev, dtype=torch.float32)[None, :] + 0.5) / 32
env = hf_amd.Envmap((0.6 + 0.4 * torch.cos(ph) * torch.sin(th) + 0.3 * torch.cos(th)).contiguous())
with torch.no_grad():
    image, value, vis = hf_amd.reflection_lighting(shape, si, ray, env, eta=ETA, spp=a.spp, return_value=True, return_visibility=True)
    r = hf_amd.reflection_rays(si, ray)
    two = (r.maxt >= 0) & ~shape.ray_test(r, coherent=False)
same = bool(torch.equal(vis.bool(), two))
info = dict(samples=n, hits=int(si.is_valid().sum()), traced=int((r.maxt >= 0).sum()), visible=int(vis.sum()),
            fused_equals_two_call=same)
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the two-call sequence disagree"
del two

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
dat, table = env.full().detach().contiguous(), env.table()
W, H = env.resolution
rot = C.byref(env._rot)
mid = (None, None, ETA, W, H, dat.data_ptr(), rot)
words = torch.empty(n, dtype=torch.int32, device=dev)


def fused():
    _capi.check(lib.hf_reflect_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), *mid,
                                        image.data_ptr(), value.data_ptr(), vis.data_ptr(), stream))


def envmap_one_ray():
    _capi.check(lib.hf_envmap_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, 1, 0, None,
                                       W, H, dat.data_ptr(), table.data_ptr(), rot, 1.0, image.data_ptr(), words.data_ptr(), stream))


def two_call():
    _capi.check(lib.hf_reflect_rays(n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, rows(r.o), rows(r.d),
                                    r.maxt.data_ptr(), stream))
    shape.ray_test(r, coherent=False)


with torch.no_grad():
    # alternate so that the launches see the same machine
    f1 = timed(fused)
    e1 = timed(envmap_one_ray)
    t2 = timed(two_call)
    f2 = timed(fused)
    e2 = timed(envmap_one_ray)
    fused()                                         # (image and vis are the reflection row's again)
report("fused_forward", f1, **info)
report("envmap_lighting_num_rays_1", e1)
report("rays_plus_ray_test_incoherent_hint", t2)
report("fused_forward_again", f2)
report("envmap_lighting_num_rays_1_again", e2)
del words, r
head = (n, a.spp, rows(sn), rows(dd), tt.data_ptr(), *mid, vis.data_ptr())
gi, gv = torch.randn(n // a.spp, device=dev), torch.randn(n, device=dev)
g_n, g_w, g_d = torch.empty_like(sn), torch.empty(n, device=dev), torch.zeros_like(dat)
report("adjoint", timed(lambda: _capi.check(lib.hf_reflect_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(g_n), g_w.data_ptr(),
                                                                            None, stream))))
report("adjoint_with_grad_data", timed(lambda: _capi.check(lib.hf_reflect_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(g_n),
                                                                                           g_w.data_ptr(), g_d.data_ptr(), stream))))
del g_n, g_w
dn, dimg = torch.randn_like(sn), torch.empty(n // a.spp, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_reflect_lighting_tangent(*head, rows(dn), gv.data_ptr(), None, dimg.data_ptr(),
                                                                            value.data_ptr(), stream))))

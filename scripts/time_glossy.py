#!/usr/bin/env python3
"""Time the glossy row with HIP events on the benchmark's wavefront (the 4096^2 sine field under 1024 x 1024 x 64 =
67.1 M samples; alpha 0.3, eta 0, a smooth 33 x 17 map), 2 warm-ups and the median of 10:
    the fused launch hf_glossy_lighting (image, value and visibility word) at num_rays K = 1, 4, 8;
    the K-fold two-call sequence hf_glossy_rays + hf_ray_test with the incoherent hint (ray_test(coherent=False));
    hf_envmap_lighting at the same K (its device code is the parent commit's: profiles/glossy/registers.txt) and
    hf_reflect_lighting (one any-hit walk per sample) on the same wavefront;
    the adjoint (with and without grad_data) and the tangent at K = 4 on the words the forward wrote.
usage: python scripts/time_glossy.py [--warmup 2 --iters 10 --out profiles/glossy/times.jsonl] [--grid 4096 --film 1024 --spp 64]
One JSON line per measurement (median / min / mean ms over the timed calls).  Bit k of the fused word is compared with
the two-call answer first, for every k < 8.  A record, not a pass criterion."""
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
ETA, ALPHA, SEED, KS = 0.0, 0.3, 0, (1, 4, 8)

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_glossy.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, eta=ETA, alpha=ALPHA, map="33x17")


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
alpha = torch.full((n,), ALPHA, device=dev)
with torch.no_grad():
    image, value, words = hf_amd.glossy_lighting(shape, si, ray, env, alpha, eta=ETA, spp=a.spp, num_rays=max(KS), seed=SEED,
                                                 return_value=True, return_visibility=True)
    same, traced, visible = True, 0, 0
    for k in range(max(KS)):
        r = hf_amd.glossy_rays(si, ray, alpha, k, seed=SEED)
        two = (r.maxt >= 0) & ~shape.ray_test(r, coherent=False)
        same = same and bool(torch.equal(((words >> k) & 1).bool(), two))
        traced += int((r.maxt >= 0).sum()); visible += int(two.sum())
        del two
info = dict(samples=n, hits=int(si.is_valid().sum()), traced=traced, visible=visible, fused_equals_two_call=same)
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the two-call sequence disagree"

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
dat, table = env.full().detach().contiguous(), env.table()
W, H = env.resolution
rot = C.byref(env._rot)
wordsu = torch.empty(n, dtype=torch.int32, device=dev)
vis8 = torch.empty(n, dtype=torch.uint8, device=dev)
mid = lambda K: (None, None, alpha.data_ptr(), ETA, K, SEED, None, W, H, dat.data_ptr(), rot)


def fused(K):
    return lambda: _capi.check(lib.hf_glossy_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), *mid(K),
                                                      image.data_ptr(), value.data_ptr(), words.data_ptr(), stream))


def envmap(K):
    return lambda: _capi.check(lib.hf_envmap_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, K, SEED,
                                                      None, W, H, dat.data_ptr(), table.data_ptr(), rot, 1.0, image.data_ptr(),
                                                      wordsu.data_ptr(), stream))


def reflect():
    _capi.check(lib.hf_reflect_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, None, ETA, W, H,
                                        dat.data_ptr(), rot, image.data_ptr(), value.data_ptr(), vis8.data_ptr(), stream))


def two_call(K):
    def run():
        for k in range(K):
            _capi.check(lib.hf_glossy_rays(n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, alpha.data_ptr(), k, SEED, None,
                                           rows(r.o), rows(r.d), r.maxt.data_ptr(), None, stream))
            shape.ray_test(r, coherent=False)
    return run


with torch.no_grad():
    for K in KS:                                    # alternate so that the launches see the same machine
        f1 = timed(fused(K)); e1 = timed(envmap(K)); t2 = timed(two_call(K)); f2 = timed(fused(K))
        report("fused_forward", f1, num_rays=K, **(info if K == KS[0] else {}))
        report("envmap_lighting", e1, num_rays=K)
        report("rays_plus_ray_test_incoherent_hint", t2, num_rays=K)
        report("fused_forward_again", f2, num_rays=K)
    report("reflect_lighting", timed(reflect))
    fused(4)()                                      # (image and words are K = 4's again)
del wordsu, vis8, r
K = 4
head = (n, a.spp, rows(sn), rows(dd), tt.data_ptr(), *mid(K), words.data_ptr())
gi, gv = torch.randn(n // a.spp, device=dev), torch.randn(n, device=dev)
g_n, g_w, g_a, g_d = torch.empty_like(sn), torch.empty(n, device=dev), torch.empty(n, device=dev), torch.zeros_like(dat)
report("adjoint", timed(lambda: _capi.check(lib.hf_glossy_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(g_n), g_w.data_ptr(),
                                                                           g_a.data_ptr(), None, stream))), num_rays=K)
report("adjoint_with_grad_data", timed(lambda: _capi.check(lib.hf_glossy_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(g_n),
                                                                                          g_w.data_ptr(), g_a.data_ptr(), g_d.data_ptr(),
                                                                                          stream))), num_rays=K)
del g_n, g_w
dn, dimg = torch.randn_like(sn), torch.empty(n // a.spp, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_glossy_lighting_tangent(*head, rows(dn), gv.data_ptr(), g_a.data_ptr(), None,
                                                                           dimg.data_ptr(), value.data_ptr(), stream))), num_rays=K)

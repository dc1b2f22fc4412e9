#!/usr/bin/env python3
"""Time the area-light row with HIP events on a 2048 x 2048 x 4 spp orthographic wavefront (16.8 M samples) over the 4096^2
sine field, the lamp `above` of tests/rect_ref.py, K = 8 points per sample:
    the fused launch (hf_rect_lighting: image, vis_bits), without and with a 64 x 64 texture;
    the K-fold sequence it replaces, as far as the visibility word: per point hf_rect_rays + hf_ray_test and a torch
    reduction of the hit bytes into the word (the shading sum is NOT in it: a lower bound of the sequence);
    the adjoint (hf_rect_lighting_adjoint: grad_sh_n, grad_p, grad_weight) without and with grad_tex;
    the tangent.
usage: python scripts/time_rect.py [--warmup 3 --iters 20 --out profiles/rect/times.jsonl] [--grid 4096 --film 2048 --spp 4]
One JSON line per measurement (median / min / mean ms over the timed calls; the compared pair alternates so that both see
the same machine).  The fused visibility word is compared with the sequence's first."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=2048)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
K, SEED, TEXELS = 8, 5, 64

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_rect.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, num_rays=K)


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
n, npix = len(ray), len(ray) // a.spp
c = (torch.arange(TEXELS, device=dev, dtype=torch.float32) + 0.5) / TEXELS
tex = (0.6 + 0.25 * torch.sin(9.0 * c)[None, :] + 0.15 * torch.cos(7.0 * c)[:, None]).contiguous()
lamp = hf_amd.RectLight((0.2, -0.1, 1.1), (0.0, 0.2, 0.0), (0.3, 0.0, 0.05), 10.0)
S = lamp._struct()

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
image, vis = torch.empty(npix, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
ro, rd, rm = torch.empty(3, n, device=dev), torch.empty(3, n, device=dev), torch.empty(n, device=dev)
hit = torch.empty(n, dtype=torch.uint8, device=dev)
R = _capi.hf_rays_t(rows(ro), rows(rd), rm.data_ptr())
mid = lambda t: (None, K, SEED, None, S, TEXELS if t else 0, TEXELS if t else 0, tex.data_ptr() if t else None, 0.8)


def fused(t=False):
    _capi.check(lib.hf_rect_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), *mid(t),
                                     image.data_ptr(), vis.data_ptr(), stream))


def sequence():
    words = torch.zeros(n, dtype=torch.int32, device=dev)
    for k in range(K):
        _capi.check(lib.hf_rect_rays(n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), k, SEED, None, S, rows(ro), rows(rd),
                                     rm.data_ptr(), stream))
        _capi.check(lib.hf_ray_test(shape._h, n, C.byref(R), None, hit.data_ptr(), stream))
        words |= ((rm >= 0) & (hit == 0)).to(torch.int32) << k
    return words


with torch.no_grad():
    fused()
    same = bool(torch.equal(vis, sequence()))
    bits = (vis[:, None] >> torch.arange(K, device=dev, dtype=torch.int32)[None]) & 1
info = dict(samples=n, hits=int(si.is_valid().sum()), visible_draws=int(bits.sum()), vis_equals_sequence=same)
del bits
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the K-fold sequence disagree"

with torch.no_grad():
    f1 = timed(fused)
    s1 = timed(sequence)
    f2 = timed(fused)
    s2 = timed(sequence)
    ft = timed(lambda: fused(True))
report("fused_forward", f1, **info)
report("rays_plus_ray_test_plus_torch_visibility_only", s1)
report("fused_forward_again", f2)
report("rays_plus_ray_test_plus_torch_visibility_only_again", s2)
report("fused_forward_textured", ft, texture=TEXELS)
del ro, rd, rm, hit

fused()
gimg = torch.randn(npix, device=dev)
g_n, g_p, g_w, g_t = torch.empty_like(sn), torch.empty_like(sn), torch.empty(n, device=dev), torch.zeros(TEXELS, TEXELS, device=dev)
head = (n, a.spp, rows(pp), rows(sn), rows(dd), tt.data_ptr())
report("adjoint", timed(lambda: _capi.check(lib.hf_rect_lighting_adjoint(
    *head, *mid(False), vis.data_ptr(), gimg.data_ptr(), rows(g_n), rows(g_p), g_w.data_ptr(), None, stream))))
report("adjoint_textured_without_grad_tex", timed(lambda: _capi.check(lib.hf_rect_lighting_adjoint(
    *head, *mid(True), vis.data_ptr(), gimg.data_ptr(), rows(g_n), rows(g_p), g_w.data_ptr(), None, stream))), texture=TEXELS)
report("adjoint_textured_with_grad_tex", timed(lambda: _capi.check(lib.hf_rect_lighting_adjoint(
    *head, *mid(True), vis.data_ptr(), gimg.data_ptr(), rows(g_n), rows(g_p), g_w.data_ptr(), g_t.data_ptr(), stream))), texture=TEXELS)
del g_n, g_p, g_w
dn, dp = torch.randn_like(sn), torch.randn_like(sn)
dimg = torch.empty(npix, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_rect_lighting_tangent(
    *head, *mid(False), vis.data_ptr(), rows(dn), rows(dp), None, None, dimg.data_ptr(), stream))))

#!/usr/bin/env python3
"""Time the directional row with HIP events on scripts/time_spot.py's scene -- a 2048 x 2048 x 4 spp orthographic wavefront
(16.8 M samples) over the 4096^2 sine field -- under the first K lights of the rig of tests/directional_ref.py:
    the fused launch (hf_directional_lighting: K images, K value rows, vis) at K = 4 (the size of the rig of
    examples/inverse_heights.py) and K = 8;
    the same images by the sequence it replaces (examples/inverse_heights.py --shadows): per light si.spawn_ray(l) in
    torch + shape.ray_test, then ONE hf_direct_lighting_weighted (K images) given the K visibility rows;
    the K launch against K single-light launches;
    the adjoint (grad_sh_n, grad_weight) without and with grad_lights (the K x 4 reduced numbers), and the tangent, at K = 8.
usage: python scripts/time_directional.py [--warmup 2 --iters 10 --out profiles/directional/times.jsonl]
                                          [--grid 4096 --film 2048 --spp 4]
One JSON line per measurement (median / min / max / mean ms over the timed calls; the compared pair alternates in one
process so that both see the same machine).  The fused visibility bits are compared with hf_directional_rays +
hf_ray_test first, and the torch sequence's visibility rows with them."""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=2048)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.warmup >= 2 and a.iters >= 5, "the protocol: 2 warm-ups, at least 5 timed calls"
ALBEDO = 0.8

import numpy as np  # noqa: E402
import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
import directional_ref as D  # noqa: E402
assert torch.cuda.is_available(), "time_directional.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp)


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
    rec = dict(kind=kind, **scene, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
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
ref = D.rig()
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))


def structs(ks):
    S = (_capi.hf_directional_light_t * len(ks))()
    for j, k in enumerate(ks):
        S[j] = _capi.hf_directional_light_t((C.c_double * 3)(*ref[k].to_light.tolist()), ref[k].irradiance)
    return S


image, value = torch.empty(8, npix, device=dev), torch.empty(8, n, device=dev)
vis = torch.empty(n, dtype=torch.uint8, device=dev)
vis1 = torch.empty(n, dtype=torch.uint8, device=dev)


def fused(ks, with_value=True, out=None):
    _capi.check(lib.hf_directional_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, len(ks),
                                            structs(ks), ALBEDO, image.data_ptr(), value.data_ptr() if with_value else None,
                                            (out if out is not None else vis).data_ptr(), stream))


si_d = hf_amd.SurfaceInteraction3f()
si_d.p, si_d.n, si_d.t = pp, gn, tt
si_d.sh_frame = hf_amd.Frame3f(None, None, sn)
# the [K, 4] table direct_lighting takes: unit directions, float32
table = torch.tensor(np.stack([np.append(D.unit(L)[0], L.irradiance) for L in ref]), dtype=torch.float32)


def sequence(ks):
    """examples/inverse_heights.py --shadows: per light si.spawn_ray(l) in torch + one ray_test launch, then one
    hf_direct_lighting_weighted given the K visibility rows: returns (the [K, npix] images, the [K, n] rows)"""
    lights = table[list(ks)]
    v = torch.stack([~shape.ray_test(si_d.spawn_ray(l[:3])) for l in lights]).to(torch.uint8)
    return hf_amd.direct_lighting(si_d, ray, lights, albedo=ALBEDO, spp=a.spp, vis=v), v


with torch.no_grad():
    fused(tuple(range(8)))
    byte, img8 = vis.clone(), image.clone()
    same = True
    for k in range(8):
        r = hf_amd.directional_rays(si_d, ray, hf_amd.DirectionalLight(ref[k].to_light, ref[k].irradiance))
        same = same and bool(torch.equal((byte >> k) & 1, ((r.maxt >= 0) & ~shape.ray_test(r)).to(torch.uint8)))
    del r
    simg, sv = sequence(tuple(range(8)))
    # (the torch rows mark every unoccluded sample; the fused bits only those that are eligible and face the light)
    differ = [int((((byte >> k) & 1).bool() & ~sv[k].bool()).sum()) for k in range(8)]
    diff = float((simg - img8).abs().max())
info = dict(samples=n, hits=int(si.is_valid().sum()), visible_bits=[int(((byte >> k) & 1).sum()) for k in range(8)],
            vis_equals_rays_plus_ray_test=same, fused_bits_the_torch_sequence_calls_occluded=differ,
            sequence_image_max_abs_diff=diff, image_max=float(img8.max()))
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and hf_directional_rays + hf_ray_test disagree"
del simg, sv

with torch.no_grad():
    for K in (4, 8):
        ks = tuple(range(K))
        f1 = timed(lambda: fused(ks))
        s1 = timed(lambda: sequence(ks))
        f2 = timed(lambda: fused(ks))
        s2 = timed(lambda: sequence(ks))
        report("fused_forward", f1, K=K, **(info if K == 8 else {}))
        report("torch_spawn_ray_plus_ray_test_per_light_plus_direct_lighting_weighted", s1, K=K)
        report("fused_forward_again", f2, K=K)
        report("torch_spawn_ray_plus_ray_test_per_light_plus_direct_lighting_weighted_again", s2, K=K)

        def singles():
            for k in ks:
                fused((k,), out=vis1)
        e1 = timed(singles)
        f3 = timed(lambda: fused(ks))
        e2 = timed(singles)
        report("K_launches_of_one", e1, K=K)
        report("fused_forward_third", f3, K=K)
        report("K_launches_of_one_again", e2, K=K)
    report("fused_forward_images_and_vis_only", timed(lambda: fused(tuple(range(8)), with_value=False)), K=8)
    fused(tuple(range(8)))
del value

S8 = structs(tuple(range(8)))
gimg = torch.randn(8, npix, device=dev)
g_n, g_w = torch.empty_like(sn), torch.empty(n, device=dev)
gl = torch.zeros(8, 4, device=dev)
ws = torch.empty(lib.hf_directional_workspace_floats(8), device=dev)
head = (n, a.spp, rows(sn), rows(dd), tt.data_ptr(), None, 8, S8, ALBEDO, vis.data_ptr())
report("adjoint_per_lane_outputs_only", timed(lambda: _capi.check(lib.hf_directional_lighting_adjoint(
    *head, gimg.data_ptr(), None, rows(g_n), g_w.data_ptr(), None, None, stream))), K=8)
report("adjoint_with_grad_lights", timed(lambda: _capi.check(lib.hf_directional_lighting_adjoint(
    *head, gimg.data_ptr(), None, rows(g_n), g_w.data_ptr(), gl.data_ptr(), ws.data_ptr(), stream))), K=8)
report("adjoint_grad_lights_only", timed(lambda: _capi.check(lib.hf_directional_lighting_adjoint(
    *head, gimg.data_ptr(), None, None, None, gl.data_ptr(), ws.data_ptr(), stream))), K=8)
del g_n, g_w
dn = torch.randn_like(sn)
dl = torch.randn(8, 4, device=dev)
dimg = torch.empty(8, npix, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_directional_lighting_tangent(
    *head, rows(dn), None, dl.data_ptr(), dimg.data_ptr(), None, stream))), K=8)

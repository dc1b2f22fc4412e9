#!/usr/bin/env python3
"""Time the projector row with HIP events on a 2048 x 2048 x 4 spp orthographic wavefront (16.8 M samples) over the 4096^2
sine field, the projector `above` of tests/projector_ref.py with a 64 x 32 texture:
    the fused launch (hf_projector_lighting: image, value, vis, uv);
    the composition available without it, GIVEN the visibility: hf_sensor_project on a film of TW x TH -> hf_bitmap_eval
    (Bitmap.eval) -> torch arithmetic for G = <sh_n, c - p> / ref.z^3 and the box film.  The shadow rays and their
    hf_ray_test are NOT in it: a lower bound of the sequence;
    hf_projector_rays + hf_ray_test, the part of the sequence the line above leaves out;
    the adjoint (grad_sh_n, grad_p, grad_weight and the 14 reduced numbers) without and with grad_tex;
    the tangent.
usage: python scripts/time_projector.py [--warmup 3 --iters 20 --out profiles/projector/times.jsonl] [--grid 4096 --film 2048 --spp 4]
One JSON line per measurement (median / min / mean ms over the timed calls; the compared pair alternates so that both see
the same machine).  The fused visibility is compared with the two-call sequence's first."""
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
TW, TH, FOV, SCALE, ALBEDO = 64, 32, 40.0, 1.5, 0.8

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_projector.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, texture=[TW, TH])


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
cx = (torch.arange(TW, device=dev, dtype=torch.float32) + 0.5) / TW
cy = (torch.arange(TH, device=dev, dtype=torch.float32) + 0.5) / TH
tex = (0.6 + 0.25 * torch.sin(9.0 * cx)[None, :] + 0.15 * torch.cos(7.0 * cy)[:, None]).contiguous()
to_world = hf_amd.workload.look_at((0.3, -0.2, 2.0), (0.0, 0.0, 0.25), (0.0, 1.0, 0.0))
proj = hf_amd.Projector(to_world, FOV, tex, scale=SCALE, wrap="repeat")
S = proj._struct(proj.to_world, FOV, SCALE)

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
image, value, vis, uv = torch.empty(npix, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), \
    torch.empty(2, n, device=dev)
mid = (None, S, TW, TH, tex.data_ptr(), _capi.HF_WRAP_REPEAT, ALBEDO)


def fused():
    _capi.check(lib.hf_projector_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), *mid,
                                          image.data_ptr(), value.data_ptr(), vis.data_ptr(), rows(uv), stream))


cam = hf_amd.PerspectiveCamera(to_world, FOV, film=(TW, TH), near_clip=1e-3, far_clip=1e4)
bitmap = hf_amd.Bitmap(tex, wrap="repeat")
A32 = torch.as_tensor(to_world, device=dev)[:3, :3].float()
c32 = torch.as_tensor(to_world, device=dev)[:3, 3].float()


def composition():
    """float32 torch arithmetic (the float64 of the kernel's shading term would cost the sequence more)"""
    pos, _, _ = cam.sample_direction(pp)
    I = bitmap.eval(pos)
    u = c32[:, None] - pp
    z = -(A32[:, 2:3] * u).sum(0)                       # ref.z = <A e_z, p - c> for the scale-free to_world
    val = torch.where(vis.bool(), (ALBEDO * SCALE) * I * (sn * u).sum(0) / (z * z * z), torch.zeros_like(z))
    return val.reshape(-1, a.spp).mean(1), val


ro, rd, rm = torch.empty(3, n, device=dev), torch.empty(3, n, device=dev), torch.empty(n, device=dev)
hit = torch.empty(n, dtype=torch.uint8, device=dev)
R = _capi.hf_rays_t(rows(ro), rows(rd), rm.data_ptr())


def two_calls():
    _capi.check(lib.hf_projector_rays(n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), S, TW, TH, rows(ro), rows(rd),
                                      rm.data_ptr(), stream))
    _capi.check(lib.hf_ray_test(shape._h, n, C.byref(R), None, hit.data_ptr(), stream))
    return (rm >= 0) & (hit == 0)


with torch.no_grad():
    fused()
    same = bool(torch.equal(vis.bool(), two_calls()))
    cimg, _ = composition()
    diff = float((cimg - image).abs().max())
info = dict(samples=n, hits=int(si.is_valid().sum()), visible=int(vis.sum()), vis_equals_sequence=same,
            composition_image_max_abs_diff=diff, image_max=float(image.max()))
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the two-call sequence disagree"

with torch.no_grad():
    f1 = timed(fused)
    c1 = timed(composition)
    f2 = timed(fused)
    c2 = timed(composition)
    r1 = timed(two_calls)
report("fused_forward", f1, **info)
report("sensor_project_plus_bitmap_eval_plus_torch_given_vis", c1)
report("fused_forward_again", f2)
report("sensor_project_plus_bitmap_eval_plus_torch_given_vis_again", c2)
report("projector_rays_plus_ray_test", r1)
del ro, rd, rm, hit

gimg = torch.randn(npix, device=dev)
g_n, g_p, g_w, g_t = torch.empty_like(sn), torch.empty_like(sn), torch.empty(n, device=dev), torch.zeros(TH, TW, device=dev)
g12, gf, gs = torch.zeros(12, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
ws = torch.empty(lib.hf_projector_workspace_floats(), device=dev)
head = (n, a.spp, rows(pp), rows(sn), rows(dd), tt.data_ptr())
report("adjoint_without_grad_tex", timed(lambda: _capi.check(lib.hf_projector_lighting_adjoint(
    *head, *mid, vis.data_ptr(), gimg.data_ptr(), None, rows(g_n), rows(g_p), g_w.data_ptr(), None, g12.data_ptr(), gf.data_ptr(),
    gs.data_ptr(), ws.data_ptr(), stream))))
report("adjoint_with_grad_tex", timed(lambda: _capi.check(lib.hf_projector_lighting_adjoint(
    *head, *mid, vis.data_ptr(), gimg.data_ptr(), None, rows(g_n), rows(g_p), g_w.data_ptr(), g_t.data_ptr(), g12.data_ptr(),
    gf.data_ptr(), gs.data_ptr(), ws.data_ptr(), stream))))
report("adjoint_per_lane_outputs_only", timed(lambda: _capi.check(lib.hf_projector_lighting_adjoint(
    *head, *mid, vis.data_ptr(), gimg.data_ptr(), None, rows(g_n), rows(g_p), g_w.data_ptr(), None, None, None, None, None, stream))))
del g_n, g_p, g_w
dn, dp = torch.randn_like(sn), torch.randn_like(sn)
d12, d1 = torch.randn(12, device=dev), torch.randn(1, device=dev)
dimg = torch.empty(npix, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_projector_lighting_tangent(
    *head, *mid, vis.data_ptr(), rows(dn), rows(dp), None, None, d12.data_ptr(), d1.data_ptr(), d1.data_ptr(), dimg.data_ptr(), None,
    stream))))

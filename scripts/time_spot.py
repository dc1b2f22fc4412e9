#!/usr/bin/env python3
"""Time the spot row with HIP events on a 2048 x 2048 x 4 spp orthographic wavefront (16.8 M samples) over the 4096^2 sine
field (the projector row's timing scene), under the first K lights of the rig of tests/spot_ref.py:
    the fused launch (hf_spot_lighting: K images, K value rows, vis) at K = 1, 4 and 8;
    the same images by the sequence it replaces: K x (hf_spot_rays + hf_ray_test), the falloff in float32 torch, and one
    hf_point_lighting (K images) given the K visibility rows, times the falloff's film;
    the K = 8 launch against eight K = 1 launches;
    the adjoint (grad_sh_n, grad_p, grad_weight) without and with grad_lights (the K x 15 reduced numbers), and the tangent,
    at K = 8.
usage: python scripts/time_spot.py [--warmup 3 --iters 20 --out profiles/spot/times.jsonl] [--grid 4096 --film 2048 --spp 4]
One JSON line per measurement (median / min / mean ms over the timed calls; the compared pair alternates so that both see
the same machine).  The fused visibility bits are compared with the two-call sequence's first."""
import argparse, ctypes as C, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=2048)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ALBEDO = 0.8

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
import spot_ref as P  # noqa: E402
assert torch.cuda.is_available(), "time_spot.py measures on a HIP device; there is none"
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
ref = P.rig()
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))


def structs(ks):
    S = (_capi.hf_spot_light_t * len(ks))()
    for j, k in enumerate(ks):
        L = ref[k]
        S[j] = _capi.hf_spot_light_t((C.c_double * 12)(*L.to_world.reshape(-1).tolist()), L.intensity, L.cutoff, L.beam)
    return S


image, value = torch.empty(8, npix, device=dev), torch.empty(8, n, device=dev)
vis = torch.empty(n, dtype=torch.uint8, device=dev)
vis1 = torch.empty(n, dtype=torch.uint8, device=dev)


def fused(ks, with_value=True, out=None):
    _capi.check(lib.hf_spot_lighting(shape._h, n, a.spp, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, len(ks), structs(ks),
                                     ALBEDO, image.data_ptr(), value.data_ptr() if with_value else None, (out if out is not None else vis).data_ptr(),
                                     stream))


ro, rd, rm = torch.empty(3, n, device=dev), torch.empty(3, n, device=dev), torch.empty(n, device=dev)
hit = torch.empty(n, dtype=torch.uint8, device=dev)
R = _capi.hf_rays_t(rows(ro), rows(rd), rm.data_ptr())
si_d = hf_amd.SurfaceInteraction3f()
si_d.p, si_d.n, si_d.t = pp, gn, tt
si_d.sh_frame = hf_amd.Frame3f(None, None, sn)


def falloff32(L):
    """falloff_curve in float32 torch from the float32 points"""
    A = torch.as_tensor(L.to_world[:, :3], device=dev, dtype=torch.float32)
    c = torch.as_tensor(L.to_world[:, 3], device=dev, dtype=torch.float32)
    q = A.T @ (pp - c[:, None])                              # (scale-free: the inverse is the transpose)
    th = torch.atan2(torch.hypot(q[0], q[1]), q[2])
    cut, beam = math.radians(L.cutoff), math.radians(L.beam)
    if L.cutoff == L.beam:
        return (th < cut).float()
    return ((cut - th) / (cut - beam)).clamp(0.0, 1.0)


def sequence(ks):
    """K x (hf_spot_rays + hf_ray_test), then hf_point_lighting given the visibility with the falloff as the weight of the
    film: returns (the [K, npix] images, the [K, n] visibility rows)"""
    S = structs(ks)
    v = torch.empty(len(ks), n, dtype=torch.uint8, device=dev)
    imgs = []
    for j, k in enumerate(ks):
        one = C.cast(C.byref(S, j * C.sizeof(_capi.hf_spot_light_t)), C.POINTER(_capi.hf_spot_light_t))
        _capi.check(lib.hf_spot_rays(n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), one, rows(ro), rows(rd), rm.data_ptr(), stream))
        _capi.check(lib.hf_ray_test(shape._h, n, C.byref(R), None, hit.data_ptr(), stream))
        v[j] = (rm >= 0) & (hit == 0)
    # hf_point_lighting has no per-sample weight: the falloff multiplies the samples, so the film is taken at spp 1 and
    # averaged in torch
    lights = torch.tensor([[*ref[k].to_world[:, 3], ref[k].intensity] for k in ks], dtype=torch.float32)
    per = hf_amd.point_lighting(si_d, ray, lights, albedo=ALBEDO, spp=1, vis=v)
    for j, k in enumerate(ks):
        imgs.append((per[j] * falloff32(ref[k])).reshape(-1, a.spp).mean(1))
    return torch.stack(imgs), v


with torch.no_grad():
    fused(tuple(range(8)))
    byte = vis.clone()
    img8 = image.clone()
    simg, sv = sequence(tuple(range(8)))
    same = all(bool(torch.equal(((byte >> k) & 1), sv[k])) for k in range(8))
    diff = float((simg - img8).abs().max())
info = dict(samples=n, hits=int(si.is_valid().sum()), visible_bits=[int(((byte >> k) & 1).sum()) for k in range(8)],
            vis_equals_sequence=same, sequence_image_max_abs_diff=diff, image_max=float(img8.max()))
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the two-call sequence disagree"
del simg, sv

with torch.no_grad():
    for K in (1, 4, 8):
        ks = tuple(range(K))
        f1 = timed(lambda: fused(ks))
        s1 = timed(lambda: sequence(ks))
        f2 = timed(lambda: fused(ks))
        s2 = timed(lambda: sequence(ks))
        report("fused_forward", f1, K=K, **(info if K == 8 else {}))
        report("rays_plus_ray_test_plus_point_lighting_plus_torch_falloff", s1, K=K)
        report("fused_forward_again", f2, K=K)
        report("rays_plus_ray_test_plus_point_lighting_plus_torch_falloff_again", s2, K=K)
    report("fused_forward_images_and_vis_only", timed(lambda: fused(tuple(range(8)), with_value=False)), K=8)

    def eight_singles():
        for k in range(8):
            fused((k,), out=vis1)
    e1 = timed(eight_singles)
    f3 = timed(lambda: fused(tuple(range(8))))
    e2 = timed(eight_singles)
    report("eight_launches_of_one", e1, K=8)
    report("fused_forward_third", f3, K=8)
    report("eight_launches_of_one_again", e2, K=8)
    fused(tuple(range(8)))
del ro, rd, rm, hit, value

S8 = structs(tuple(range(8)))
gimg = torch.randn(8, npix, device=dev)
g_n, g_p, g_w = torch.empty_like(sn), torch.empty_like(sn), torch.empty(n, device=dev)
gl = torch.zeros(8, 15, device=dev)
ws = torch.empty(lib.hf_spot_workspace_floats(8), device=dev)
head = (n, a.spp, rows(pp), rows(sn), rows(dd), tt.data_ptr(), None, 8, S8, ALBEDO, vis.data_ptr())
report("adjoint_per_lane_outputs_only", timed(lambda: _capi.check(lib.hf_spot_lighting_adjoint(
    *head, gimg.data_ptr(), None, rows(g_n), rows(g_p), g_w.data_ptr(), None, None, stream))), K=8)
report("adjoint_with_grad_lights", timed(lambda: _capi.check(lib.hf_spot_lighting_adjoint(
    *head, gimg.data_ptr(), None, rows(g_n), rows(g_p), g_w.data_ptr(), gl.data_ptr(), ws.data_ptr(), stream))), K=8)
report("adjoint_grad_lights_only", timed(lambda: _capi.check(lib.hf_spot_lighting_adjoint(
    *head, gimg.data_ptr(), None, None, None, None, gl.data_ptr(), ws.data_ptr(), stream))), K=8)
del g_n, g_p, g_w
dn, dp = torch.randn_like(sn), torch.randn_like(sn)
dl = torch.randn(8, 15, device=dev)
dimg = torch.empty(8, npix, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_spot_lighting_tangent(
    *head, rows(dn), rows(dp), None, dl.data_ptr(), dimg.data_ptr(), None, stream))), K=8)

#!/usr/bin/env python3
"""Time the specular row with HIP events on scripts/time_directional.py's scene -- a 2048 x 2048 x 4 spp orthographic
wavefront (16.8 M samples) over the 4096^2 sine field -- under the first K lights of the rig of tests/directional_ref.py,
K = 4 and K = 8, a per-sample roughness row over [0.05, 0.6], eta 1.5, the visibility byte of hf_directional_lighting:
    the fused forward (hf_specular_lighting: K images and K value rows) against the same arithmetic written with torch
    on the device (float32, [K, n] tensors, one where() for the masks, a mean for the film);
    the fused adjoint (grad_sh_n, grad_weight, grad_alpha, and with the K x 4 reduced numbers) against torch's forward +
    backward of that text (autograd needs its own forward; the fused adjoint forms the lobe again too);
    the fused tangent against torch.func.jvp of that text.
usage: python scripts/time_specular.py [--warmup 2 --iters 10 --out profiles/specular/times.jsonl]
                                       [--grid 4096 --film 2048 --spp 4]
One JSON line per measurement (median / min / max / mean ms over the timed calls; the compared pair alternates in one
process so that both see the same machine).  The torch text's values are compared with the fused ones first."""
import argparse, ctypes as C, json, math, os, statistics, sys
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
ETA = 1.5

import numpy as np  # noqa: E402
import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
import directional_ref as D  # noqa: E402
assert torch.cuda.is_available(), "time_specular.py measures on a HIP device; there is none"
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
ref = D.rig()
with torch.no_grad():
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    _, byte = hf_amd.directional_lighting(shape, si, ray, [hf_amd.DirectionalLight(L.to_light, L.irradiance) for L in ref],
                                          spp=a.spp, return_visibility=True)
n, npix = len(ray), len(ray) // a.spp
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
sn, dd = si.sh_frame.n.detach().contiguous(), ray.d.detach().contiguous()
del si, rays
alpha = 0.05 + 0.55 * torch.rand(n, device=dev, generator=torch.Generator(dev).manual_seed(3))
weight = 0.5 + torch.rand(n, device=dev, generator=torch.Generator(dev).manual_seed(4))


def structs(K):
    S = (_capi.hf_directional_light_t * K)()
    for k in range(K):
        S[k] = _capi.hf_directional_light_t((C.c_double * 3)(*ref[k].to_light.tolist()), ref[k].irradiance)
    return S


def lobe(sn, w, al, l, E, vis):
    """the header's value of every sample under every light in float32 torch: [K, n]"""
    wi = -dd
    ci = (sn * wi).sum(0)
    co = l @ sn
    ok = vis & (ci > 0)[None] & (co > 0)
    ci, co = ci.clamp_min(1e-6), co.clamp_min(1e-6)        # (masked lanes: finite, then dropped)
    m = wi[None] + l[:, :, None]
    M = m.norm(dim=1)
    h = m / M[:, None]
    ch, u = (h * sn[None]).sum(1), (h * wi[None]).sum(1)
    cta = (1 - (1 - u * u) / (ETA * ETA)).clamp_min(0).sqrt()
    a_s, a_p = (u - ETA * cta) / (u + ETA * cta), (cta - ETA * u) / (cta + ETA * u)
    F = 0.5 * (a_s * a_s + a_p * a_p)
    a2 = al.clamp_min(1e-4) ** 2
    g1 = lambda c: 2 / (1 + (1 + a2 * (1 - c * c).clamp_min(0) / (c * c)).sqrt())
    q = (1 - ch * ch).clamp_min(0) / a2 + ch * ch
    val = w * E[:, None] * F * g1(ci) * g1(co) / (math.pi * a2 * q * q * 4 * ci)
    return torch.where(ok, val, torch.zeros((), device=dev))


def film(v):
    return v.reshape(v.shape[0], npix, a.spp).mean(2)


for K in (4, 8):
    S = structs(K)
    vis_k = torch.stack([((byte >> k) & 1).bool() for k in range(K)])
    l = torch.tensor(np.stack([D.unit(ref[k])[0] for k in range(K)]), dtype=torch.float32, device=dev)
    E = torch.tensor([ref[k].irradiance for k in range(K)], dtype=torch.float32, device=dev)
    image, value = torch.empty(K, npix, device=dev), torch.empty(K, n, device=dev)
    head = (n, a.spp, rows(sn), rows(dd), weight.data_ptr(), alpha.data_ptr(), ETA, K, S, byte.data_ptr())
    fused = lambda: _capi.check(lib.hf_specular_lighting(*head, image.data_ptr(), value.data_ptr(), stream))

    def torch_forward():
        with torch.no_grad():
            v = lobe(sn, weight, alpha, l, E, vis_k)
            return film(v), v
    fused()
    ti, tv = torch_forward()
    info = dict(samples=n, lit=[int(v.sum()) for v in vis_k], value_max=float(value.max()),
                torch_value_max_abs_diff=float((tv - value).abs().max()), torch_image_max_abs_diff=float((ti - image).abs().max()))
    print(json.dumps(dict(kind="check", K=K, **scene, **info)), flush=True)
    del ti, tv
    f1 = timed(fused); t1 = timed(torch_forward); f2 = timed(fused); t2 = timed(torch_forward)
    report("fused_forward", f1, K=K, **info)
    report("torch_forward", t1, K=K)
    report("fused_forward_again", f2, K=K)
    report("torch_forward_again", t2, K=K)
    del value

    gimg = torch.randn(K, npix, device=dev)
    g_n, g_w, g_a = torch.empty_like(sn), torch.empty(n, device=dev), torch.empty(n, device=dev)
    gl = torch.zeros(K, 4, device=dev)
    ws = torch.empty(lib.hf_specular_workspace_floats(K), device=dev)
    adj = lambda lights: _capi.check(lib.hf_specular_lighting_adjoint(
        *head, gimg.data_ptr(), None, rows(g_n), g_w.data_ptr(), g_a.data_ptr(), gl.data_ptr() if lights else None,
        ws.data_ptr() if lights else None, stream))

    def torch_backward(lights):
        leaves = [x.detach().requires_grad_(True) for x in ((sn, weight, alpha, l, E) if lights else (sn, weight, alpha))]
        v = lobe(*leaves, *(() if lights else (l, E)), vis_k)
        return torch.autograd.grad((film(v) * gimg).sum(), leaves)
    for lights in (False, True):
        tag = "_with_grad_lights" if lights else "_per_lane_outputs_only"
        f1 = timed(lambda: adj(lights)); t1 = timed(lambda: torch_backward(lights))
        f2 = timed(lambda: adj(lights)); t2 = timed(lambda: torch_backward(lights))
        report("fused_adjoint" + tag, f1, K=K)
        report("torch_forward_plus_backward" + tag, t1, K=K)
        report("fused_adjoint" + tag + "_again", f2, K=K)
        report("torch_forward_plus_backward" + tag + "_again", t2, K=K)
    del g_n, g_w, g_a

    dn, da = torch.randn_like(sn), 0.05 * torch.randn(n, device=dev)
    dl = torch.randn(K, 4, device=dev)
    dimg = torch.empty(K, npix, device=dev)
    tan = lambda: _capi.check(lib.hf_specular_lighting_tangent(*head, rows(dn), None, da.data_ptr(), dl.data_ptr(), dimg.data_ptr(),
                                                               None, stream))
    # (the tangent of l through the normalisation, as the kernel forms it from the tangent of to_light)
    inv = torch.tensor([1.0 / float(D.unit(ref[k])[1]) for k in range(K)], dtype=torch.float32, device=dev)
    dlk = (dl[:, :3] - l * (l * dl[:, :3]).sum(1, keepdim=True)) * inv[:, None]

    def torch_jvp():
        with torch.no_grad():
            return torch.func.jvp(lambda s, al, ll, EE: film(lobe(s, weight, al, ll, EE, vis_k)), (sn, alpha, l, E),
                                  (dn, da, dlk, dl[:, 3].contiguous()))[1]
    tan()
    tj = torch_jvp()
    print(json.dumps(dict(kind="check_tangent", K=K, dimage_max=float(dimg.abs().max()),
                          torch_dimage_max_abs_diff=float((tj - dimg).abs().max()))), flush=True)
    del tj
    f1 = timed(tan); t1 = timed(torch_jvp); f2 = timed(tan); t2 = timed(torch_jvp)
    report("fused_tangent", f1, K=K)
    report("torch_func_jvp", t1, K=K)
    report("fused_tangent_again", f2, K=K)
    report("torch_func_jvp_again", t2, K=K)
    del dn, da, dimg, image, gimg
    torch.cuda.empty_cache()

#!/usr/bin/env python3
"""Time the refraction view with HIP events on the wavefront scripts/time_caustic.py uses (the 4096^2 sine field under
1024 x 1024 x 64 = 67.1 M samples; eta 1.33, a receiver plane at z = -0.5 carrying a 1024 x 1024 texture, sigma_t = 0: the
sequence it replaces has no absorption):
    the fused launch (hf_refract_lighting: image, value, vis);
    the three-step sequence it replaces: hf_caustic_lighting (pos, value, vis), hf_bitmap_eval(pos), then the product
    with eta_ti^2 and the box film in torch;
    the fused adjoint (hf_refract_lighting_adjoint: grad_sh_n, grad_p, grad_tex from grad_image);
    the adjoint of the sequence: the film's and the product's transposes in torch, hf_bitmap_eval_adjoint (grad_pos,
    grad_tex), hf_caustic_adjoint (grad_sh_n, grad_p);
    the fused tangent.
usage: python scripts/time_refract.py [--warmup 2 --iters 10 --out profiles/refract/times.jsonl] [--grid 4096 --film 1024 --spp 64]
One JSON line per measurement (median / min / mean ms over the timed calls).  The fused outputs are compared with the
sequence's first."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()
ETA, Z = 1.33, -0.5

import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_refract.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, eta=ETA, receiver_z=Z, sigma_t=0.0, texture=a.film)


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
rcv = hf_amd.Receiver.plane_z(Z, (-1.0, 1.0), (-1.0, 1.0), a.film, a.film)
c = (torch.arange(a.film, device=dev, dtype=torch.float32) + 0.5) / a.film
tex = (0.6 + 0.25 * torch.sin(9.0 * c)[None, :] + 0.15 * torch.cos(7.0 * c)[:, None]).contiguous()
TW = TH = a.film

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
S = rcv._struct()
head = (n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None)
mid = (rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None, None, ETA, 0.0, S, TW, TH, tex.data_ptr(), 0)
# eta_ti^2 of every sample (a few rays enter the field from the side and meet the surface from below: c_i < 0), formed
# once, outside the timed sequences: it does not change from call to call
eta32 = torch.tensor(ETA, dtype=torch.float32, device=dev)
e2 = torch.where(-(sn * dd).sum(0) >= 0, 1.0 / eta32, eta32) ** 2
image, value, vis = torch.empty(npix, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
pos, cval, cvis, L = torch.empty(2, n, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, device=dev)


def fused():
    _capi.check(lib.hf_refract_lighting(shape._h, n, a.spp, *mid, image.data_ptr(), value.data_ptr(), vis.data_ptr(), None, stream))


def sequence():
    _capi.check(lib.hf_caustic_lighting(shape._h, *head, None, ETA, 1.0, S, rows(pos), cval.data_ptr(), cvis.data_ptr(), stream))
    _capi.check(lib.hf_bitmap_eval(n, rows(pos), cvis.data_ptr(), TW, TH, tex.data_ptr(), 0, L.data_ptr(), None, stream))
    return ((cval * e2) * L).view(npix, a.spp).mean(1)


with torch.no_grad():
    fused()
    img2 = sequence()
    same_vis = bool(torch.equal(vis, cvis))
    diff = float((image - img2).abs().max() / img2.abs().max())
info = dict(samples=n, hits=int(si.is_valid().sum()), lit=int(vis.sum()), vis_equals_caustic=same_vis, image_rel_diff=diff)
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same_vis and diff <= 1e-5, "the fused kernel and the three-step sequence disagree"
del img2

with torch.no_grad():
    # alternate so that the sequences see the same machine
    f1 = timed(fused)
    s1 = timed(sequence)
    f2 = timed(fused)
    s2 = timed(sequence)
report("fused_forward", f1, **info)
report("caustic_plus_bitmap_plus_torch_forward", s1)
report("fused_forward_again", f2)
report("caustic_plus_bitmap_plus_torch_forward_again", s2)

gimg = torch.randn(npix, device=dev)
g_n, g_p, g_t = torch.empty_like(sn), torch.empty_like(sn), torch.zeros(TH, TW, device=dev)
gpos = torch.empty(2, n, device=dev)


def fused_adjoint():
    _capi.check(lib.hf_refract_lighting_adjoint(n, a.spp, *mid, vis.data_ptr(), gimg.data_ptr(), None, rows(g_n), rows(g_p), None,
                                                g_t.data_ptr(), stream))


def sequence_adjoint():
    g = (gimg * (1.0 / a.spp)).repeat_interleave(a.spp)
    gL, gc = (g * e2) * cval, (g * e2) * L
    _capi.check(lib.hf_bitmap_eval_adjoint(n, rows(pos), cvis.data_ptr(), TW, TH, tex.data_ptr(), 0, gL.data_ptr(), rows(gpos),
                                           g_t.data_ptr(), stream))
    _capi.check(lib.hf_caustic_adjoint(*head, None, ETA, 1.0, S, cvis.data_ptr(), rows(gpos), gc.data_ptr(), rows(g_n), rows(g_p),
                                       None, stream))


with torch.no_grad():
    fused_adjoint()
    ref_n = g_n.clone()
    sequence_adjoint()
    adj_diff = float((g_n - ref_n).norm() / ref_n.norm())
    del ref_n
    print(json.dumps(dict(kind="check_adjoint", **scene, grad_sh_n_rel_diff=adj_diff)), flush=True)
    assert adj_diff <= 1e-4, "the fused adjoint and the sequence's disagree"
    a1 = timed(fused_adjoint)
    b1 = timed(sequence_adjoint)
    a2 = timed(fused_adjoint)
    b2 = timed(sequence_adjoint)
report("fused_adjoint", a1)
report("torch_plus_bitmap_adjoint_plus_caustic_adjoint", b1)
report("fused_adjoint_again", a2)
report("torch_plus_bitmap_adjoint_plus_caustic_adjoint_again", b2)
# (what the texel atomics cost: most landings of this grazing camera lie outside the texture and clamp onto its border)
report("fused_adjoint_without_grad_tex", timed(lambda: _capi.check(lib.hf_refract_lighting_adjoint(
    n, a.spp, *mid, vis.data_ptr(), gimg.data_ptr(), None, rows(g_n), rows(g_p), None, None, stream))))
del g_n, g_p, gpos
dn, dp = torch.randn_like(sn), torch.randn_like(sn)
dimg = torch.empty(npix, device=dev)
report("fused_tangent", timed(lambda: _capi.check(lib.hf_refract_lighting_tangent(n, a.spp, *mid, vis.data_ptr(), rows(dn), rows(dp), None,
                                                                                  None, dimg.data_ptr(), None, stream))))

#!/usr/bin/env python3
"""Time the caustic row with HIP events on the benchmark's wavefront (the 4096^2 sine field under 1024 x 1024 x 64 =
67.1 M samples, used as light samples; eta 1.33, a receiver plane at z = -0.5):
    the fused launch (hf_caustic_lighting);
    the two-call sequence hf_caustic_rays + hf_ray_test with the incoherent hint (ray_test(coherent=False));
    the same sequence without the hint;
    the adjoint and the tangent (hf_caustic_adjoint, hf_caustic_tangent) on the visibility the forward wrote.
The two-call sequences walk with hf_trace_kernel, which this row does not touch: they are the yardstick.
usage: python scripts/time_caustic.py [--warmup 2 --iters 10 --out profiles/caustic/times.jsonl] [--grid 4096 --film 1024 --spp 64]
One JSON line per measurement (median / min / mean ms over the timed calls).  The fused visibility is compared with the
two-call answer first."""
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
assert torch.cuda.is_available(), "time_caustic.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, eta=ETA, receiver_z=Z)


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
rcv = hf_amd.Receiver.plane_z(Z, (-1.0, 1.0), (-1.0, 1.0), a.film, a.film)
with torch.no_grad():
    pos, value, vis = hf_amd.caustic_lighting(shape, si, ray, rcv, eta=ETA, return_visibility=True)
    r = hf_amd.caustic_rays(si, ray, rcv, ETA)
    two = (r.maxt >= 0) & ~shape.ray_test(r, coherent=False)
same = bool(torch.equal(vis.bool(), two))
info = dict(samples=n, hits=int(si.is_valid().sum()), traced=int((r.maxt >= 0).sum()), deposited=int(vis.sum()),
            fused_equals_two_call=same)
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert same, "the fused kernel and the two-call sequence disagree"
del two

lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
pp, gn, sn, dd, tt = (x.detach().contiguous() for x in (si.p, si.n, si.sh_frame.n, ray.d, si.t))
S = rcv._struct()
head = (n, rows(pp), rows(gn), rows(sn), rows(dd), tt.data_ptr(), None)
hit = torch.empty(n, dtype=torch.bool, device=dev)


def fused():
    _capi.check(lib.hf_caustic_lighting(shape._h, *head, None, ETA, 1.0, S, rows(pos), value.data_ptr(), vis.data_ptr(), stream))


def two_call(coherent):
    def go():
        _capi.check(lib.hf_caustic_rays(*head, ETA, S, rows(r.o), rows(r.d), r.maxt.data_ptr(), stream))
        shape.ray_test(r, coherent=coherent)
    return go


with torch.no_grad():
    # alternate so that the sequences see the same machine
    f1 = timed(fused)
    t_inc = timed(two_call(False))
    t_def = timed(two_call(None))
    f2 = timed(fused)
report("fused_forward", f1, **info)
report("rays_plus_ray_test_incoherent_hint", t_inc)
report("rays_plus_ray_test_no_hint", t_def)
report("fused_forward_again", f2)
gpos, gv = torch.randn(2, n, device=dev), torch.randn(n, device=dev)
g_n, g_p, g_w = torch.empty_like(sn), torch.empty_like(sn), torch.empty(n, device=dev)
report("adjoint", timed(lambda: _capi.check(lib.hf_caustic_adjoint(*head, None, ETA, 1.0, S, vis.data_ptr(), rows(gpos), gv.data_ptr(),
                                                                   rows(g_n), rows(g_p), g_w.data_ptr(), stream))))
del g_n, g_p, g_w
dn, dp = torch.randn_like(sn), torch.randn_like(sn)
dpos, dval = torch.empty(2, n, device=dev), torch.empty(n, device=dev)
report("tangent", timed(lambda: _capi.check(lib.hf_caustic_tangent(*head, None, ETA, 1.0, S, vis.data_ptr(), rows(dn), rows(dp), gv.data_ptr(),
                                                                   rows(dpos), dval.data_ptr(), stream))))

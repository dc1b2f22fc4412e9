#!/usr/bin/env python3
"""Time hf_adjoint_transform against hf_adjoint_rows on the bench wavefront (4096^2 sine field, 1024^2 x 64 spp =
67.1 M rays) with bench.py's upstream rows (t and p), with HIP events: per round and variant 5 warm-up launches, then
20 timed ones (median and min in ms).  Variants: hf_adjoint_rows, hf_adjoint_transform with grad_heights, and without.
usage: python scripts/prof_transform_grad.py [--out profiles/transform_grad/times_run.json]
Under rocprofv3 --kernel-trace --stats for the per-kernel split (profiles/transform_grad/kernel_stats.txt)."""
import argparse, ctypes as C, json, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi
from hf_amd.shape import _DIFF_ROWS, _fill, _rows
dev = torch.device("cuda", 0)
N = 4096
shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(N, N, device=dev), max_height=0.5,
                           differentiable_to_world=True)
rays = hf_amd.workload.ortho_rays(1024, 1024, 64, dev)
R = rays.shape[1]
t = torch.empty(R, device=dev); uv = torch.empty((2, R), device=dev); prim = torch.empty(R, dtype=torch.int32, device=dev)
si = torch.empty((18, R), device=dev); gsi = torch.zeros((18, R), device=dev)
lib = _capi.lib(); stream = torch.cuda.current_stream(dev).cuda_stream
r_s = shape._rays_struct(rays[0:3], rays[3:6], rays[6]); pi_s = shape._pi_struct(t, uv, prim)
si_s = _fill(_capi.hf_si_t(), _DIFF_ROWS, _rows(si, R)); g_s = _fill(_capi.hf_si_grad_t(), _DIFF_ROWS, _rows(gsi, R))
flags = int(hf_amd.RayFlags.All)
_capi.check(lib.hf_ray_intersect(shape._h, R, C.byref(r_s), flags, None, C.byref(pi_s), C.byref(si_s), stream))
hit = torch.isfinite(t)
gsi[0] = hit.float(); gsi[1:4] = si[4:7] * hit
grad = torch.zeros((N, N), device=dev); band = torch.tensor([N, 0], dtype=torch.int32, device=dev)
gtw = torch.zeros(12, device=dev)
def plain():
    _capi.check(lib.hf_adjoint_rows(shape._h, R, C.byref(r_s), C.byref(pi_s), flags, None, C.byref(g_s), grad.data_ptr(),
                                    None, None, band.data_ptr(), stream))
def xform():
    _capi.check(lib.hf_adjoint_transform(shape._h, R, C.byref(r_s), C.byref(pi_s), flags, None, C.byref(g_s), grad.data_ptr(),
                                         None, None, band.data_ptr(), gtw.data_ptr(), stream))
def xonly():
    _capi.check(lib.hf_adjoint_transform(shape._h, R, C.byref(r_s), C.byref(pi_s), flags, None, C.byref(g_s), None,
                                         None, None, None, gtw.data_ptr(), stream))
res = {}
for rnd in range(3):
    for name, fn in (("hf_adjoint_rows", plain), ("hf_adjoint_transform", xform), ("hf_adjoint_transform_no_heights", xonly)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
        ms.sort()
        res.setdefault(name, []).append({"median_ms": ms[len(ms) // 2], "min_ms": ms[0]})
print(json.dumps({"rays": R, "hits": int(hit.sum()), "grad_to_world": gtw.tolist(), "rounds": res}))
if args.out:
    open(args.out, "w").write(json.dumps(res, indent=1) + "\n")

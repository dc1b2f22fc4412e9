#!/usr/bin/env python3
"""Time hf_tangent (forward mode of the surface interaction) on the bench workload with HIP events.
usage: python scripts/prof_tangent.py [--grid 4096 --film 1024 --spp 64 --warmup 5 --iters 20] [kinds...]
kinds: h (height tangent only), hr (heights + ray tangents d_o, d_d), si (hf_compute_surface_interaction, for comparison)
One JSON line per kind: mean / min ms over the timed launches, the byte count of DESIGN 4.6 and its fraction of 8 TB/s."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hf_amd
from hf_amd import _capi
from hf_amd.shape import _AUX_ROWS, _DIFF_ROWS, _fill, _rows

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("kinds", nargs="*", default=["h", "hr", "si"])
a = ap.parse_args()
dev = torch.device("cuda", 0)
N, R = a.grid, a.film * a.film * a.spp
lib = _capi.lib()
shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(N, N, device=dev), max_height=0.5)
rays = hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)
ray = hf_amd.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
del rays
pi = shape.ray_intersect_preliminary(ray)
hits = int(pi.is_valid().sum())
rs = shape._rays_struct(ray.o, ray.d, ray.maxt)
ps = shape._pi_struct(pi.t, pi.prim_uv, pi.prim_index)
out = torch.empty((18, R), dtype=torch.float32, device=dev)
ts = _fill(_capi.hf_si_tangent_t(), _DIFF_ROWS, _rows(out, R))
aux = torch.empty((10, R), dtype=torch.float32, device=dev)
sio = _fill(_fill(_capi.hf_si_t(), _DIFF_ROWS, _rows(out, R)), _AUX_ROWS, _rows(aux, R))
g = torch.Generator(device=dev); g.manual_seed(0)
dh = torch.randn((N, N), device=dev, generator=g)
dod = torch.randn((6, R), device=dev, generator=g)
dop = (C.c_void_p * 3)(*_rows(dod, R)[0:3]); ddp = (C.c_void_p * 3)(*_rows(dod, R)[3:6])
stream = torch.cuda.current_stream(dev).cuda_stream
flags = int(hf_amd.RayFlags.All)


def launch(kind):
    if kind == "si":
        return lib.hf_compute_surface_interaction(shape._h, R, C.byref(rs), C.byref(ps), flags, None, C.byref(sio), stream)
    return lib.hf_tangent(shape._h, R, C.byref(rs), C.byref(ps), flags, None, dh.data_ptr(),
                          C.byref(dop) if kind == "hr" else None, C.byref(ddp) if kind == "hr" else None, C.byref(ts), stream)


def nbytes(kind):
    """a hit reads pi (16 B) + o, d (24 B) [+ d_o, d_d (24 B)] and writes 72 B; a miss reads pi.t and writes
    72 B; the two textures (heights, height tangent) are read once"""
    miss = R - hits
    if kind == "si":   # hf_si_kernel as launched here: hits read 40 B, misses pi.t + d (16 B); 28 rows written (112 B)
        return hits * (40 + 112) + miss * (16 + 112) + 4 * N * N
    return hits * (16 + 24 + (24 if kind == "hr" else 0) + 72) + miss * (4 + 72) + 2 * 4 * N * N


for kind in a.kinds:
    for _ in range(a.warmup):
        _capi.check(launch(kind))
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record(); _capi.check(launch(kind)); e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    mean = sum(ms) / len(ms)
    b = nbytes(kind)
    print(json.dumps({"kind": kind, "rays": R, "hits": hits, "hit_fraction": round(hits / R, 4), "ms_mean": round(mean, 4),
                      "ms_min": round(min(ms), 4), "bytes": b, "GB_per_s": round(b / mean / 1e6, 1),
                      "fraction_of_8TBps": round(b / (mean * 1e-3) / 8e12, 3)}), flush=True)

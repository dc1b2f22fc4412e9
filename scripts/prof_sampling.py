#!/usr/bin/env python3
"""Time area sampling on the bench field with HIP events: the table rebuild (hf_set_heights with the table enabled, minus
hf_set_heights without it), hf_sample_position (flat and smooth shading), hf_sample_position_adjoint and _tangent.
usage: python scripts/prof_sampling.py [--grid 4096 --warmup 5 --iters 20 --out profiles/area_sampling/times.jsonl]
       [--samples 16777216 67108864]
One JSON line per measurement: mean / min ms over the timed launches and the byte count of DESIGN 4.8."""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hf_amd
from hf_amd import _capi
from hf_amd.shape import _rows

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--samples", type=int, nargs="*", default=[1 << 24, 1 << 26])
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.grid
M = 2 * (N - 1) * (N - 1)
lib = _capi.lib()
h = hf_amd.workload.sine_heights(N, N, device=dev)
shape = hf_amd.Heightfield(heightfield=h, max_height=0.5)
stream = torch.cuda.current_stream(dev).cuda_stream
out_f = open(a.out, "w") if a.out else None


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return sum(ms) / len(ms), min(ms)


def report(kind, mean, mn, nbytes, **extra):
    rec = dict(kind=kind, grid=N, ms_mean=round(mean, 4), ms_min=round(mn, 4), bytes=nbytes,
               GB_per_s=round(nbytes / mean / 1e6, 1), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n")


hd = shape.heightfield.detach()
set_h = lambda: _capi.check(lib.hf_set_heights(shape._h, hd.data_ptr(), stream))
base, base_min = timed(set_h)
shape.ensure_pmf_built()
full, full_min = timed(set_h)
# the rebuild reads the heights twice (both passes) and writes the CDF (+ the coarse table, 1/64 of it)
report("rebuild", full - base, full_min - base_min, 2 * 4 * N * N + 4 * M + 4 * M // 64,
       set_heights_ms=round(base, 4), set_heights_with_table_ms=round(full, 4))

for smooth in (False, True):
    shape.set_face_normals(not smooth)
    for n in a.samples:
        smp = torch.rand((2, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        buf = torch.empty((11, n), device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        rows = _rows(buf, n)
        ps = _capi.hf_position_sample_t()
        for k in range(3):
            ps.p[k], ps.n[k] = rows[k], rows[3 + k]
        ps.uv[0], ps.uv[1], ps.pdf = rows[6], rows[7], rows[8]
        ps.prim_index = prim.data_ptr()
        ps.b[0], ps.b[1] = rows[9], rows[10]
        sp = (C.c_void_p * 2)(*_rows(smp, n))
        fwd = lambda: _capi.check(lib.hf_sample_position(shape._h, n, C.byref(sp), None, C.byref(ps), stream))
        mean, mn = timed(fwd)
        # 8 B of samples in, 48 B out (11 rows + prim); CDF segment + heights (+ vertex normals) gathered per sample
        report("sample_position", mean, mn, n * (8 + 48), samples=n, smooth=smooth)
        grad = torch.zeros((N, N), device=dev)
        g = torch.randn((6, n), device=dev)
        gp, gn = (C.c_void_p * 3)(*_rows(g, n)[0:3]), (C.c_void_p * 3)(*_rows(g, n)[3:6])
        bp = (C.c_void_p * 2)(rows[9], rows[10])
        adj = lambda: _capi.check(lib.hf_sample_position_adjoint(shape._h, n, prim.data_ptr(), C.byref(bp), None,
                                                                 C.byref(gp), C.byref(gn), grad.data_ptr(), stream))
        mean, mn = timed(adj)
        report("adjoint", mean, mn, n * (4 + 8 + 24), samples=n, smooth=smooth)
        dh = torch.randn((N, N), device=dev)
        dpn = torch.empty((6, n), device=dev)
        dp, dn = (C.c_void_p * 3)(*_rows(dpn, n)[0:3]), (C.c_void_p * 3)(*_rows(dpn, n)[3:6])
        tan = lambda: _capi.check(lib.hf_sample_position_tangent(shape._h, n, prim.data_ptr(), C.byref(bp), None,
                                                                 dh.data_ptr(), C.byref(dp), C.byref(dn), stream))
        mean, mn = timed(tan)
        report("tangent", mean, mn, n * (4 + 8 + 24), samples=n, smooth=smooth)
        del smp, buf, prim, grad, g, dh, dpn
        torch.cuda.empty_cache()

#!/usr/bin/env python3
"""Time eval_parameterization on the bench field with HIP events: hf_eval_parameterization (RayFlags::All, flat and smooth
shading), hf_eval_parameterization_adjoint and _tangent, for uniform random uv and a coherent raster of uv.
usage: python scripts/prof_parameterization.py [--grid 4096 --warmup 5 --iters 20 --out profiles/parameterization/times.jsonl]
       [--queries 16777216 67108864]
One JSON line per measurement: mean / min ms over the timed launches, the bytes the launch must move and the
fraction of the 8 TB/s roofline that is."""
import argparse, ctypes as C, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hf_amd
from hf_amd import _capi
from hf_amd.shape import _AUX_ROWS, _DIFF_ROWS, _fill, _rows, hf_si_grad_t, hf_si_t, hf_si_tangent_t

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--queries", type=int, nargs="*", default=[1 << 24, 1 << 26])
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
N = a.grid
ROOFLINE = 8e12
ALL = 0x2 | 0x4 | 0x8
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
               GB_per_s=round(nbytes / mean / 1e6, 1), roofline_ms=round(nbytes / ROOFLINE * 1e3, 4),
               roofline_fraction=round(nbytes / ROOFLINE * 1e3 / mn, 3), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n")


def queries(n, mode):
    if mode == "random":
        return torch.rand((2, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    r = int(math.isqrt(n))                 # a raster of r x (n / r) pixel centres, row by row (camera-like coherence)
    i = torch.arange(n, device=dev)
    return torch.stack([((i % r).float() + 0.5) / r, ((i // r).float() + 0.5) / (n // r)]).contiguous()


for smooth in (False, True):
    shape.set_face_normals(not smooth)
    vn = 48 if smooth else 0               # three 16-byte vertex normals gathered per query
    for n in a.queries:
        for mode in ("random", "raster"):
            uv = queries(n, mode)
            uvp = (C.c_void_p * 2)(*_rows(uv, n))
            buf = torch.empty((28, n), device=dev)
            prim = torch.empty(n, dtype=torch.int32, device=dev)
            out = _fill(_fill(hf_si_t(), _DIFF_ROWS, _rows(buf[:18], n)), _AUX_ROWS, _rows(buf[18:], n))
            fwd = lambda: _capi.check(lib.hf_eval_parameterization(shape._h, n, C.byref(uvp), ALL, None, C.byref(out),
                                                                   prim.data_ptr(), stream))
            mean, mn = timed(fwd)
            # 8 B of uv in; 27 rows (all but boundary_test) + prim_index out = 112 B; 3 heights gathered (+ normals)
            report("forward", mean, mn, n * (8 + 112 + 12 + vn), queries=n, uv=mode, smooth=smooth)
            del buf
            grad = torch.zeros((N, N), device=dev)
            g = torch.randn((18, n), device=dev)
            gs = _fill(hf_si_grad_t(), _DIFF_ROWS, _rows(g, n))
            adj = lambda: _capi.check(lib.hf_eval_parameterization_adjoint(shape._h, n, C.byref(uvp), ALL, None,
                                                                           C.byref(gs), grad.data_ptr(), None, stream))
            mean, mn = timed(adj)
            # 8 B of uv, 15 upstream rows (p, n, sh_n, dp_du, dp_dv) in; 3 heights (+ normals) gathered; the scatter
            # (12 B per query before the LDS tile folds it) counted once
            report("adjoint", mean, mn, n * (8 + 60 + 12 + vn + 12), queries=n, uv=mode, smooth=smooth)
            del g
            dh = torch.randn((N, N), device=dev)
            tbuf = torch.empty((18, n), device=dev)
            ts = _fill(hf_si_tangent_t(), _DIFF_ROWS, _rows(tbuf, n))
            tan = lambda: _capi.check(lib.hf_eval_parameterization_tangent(shape._h, n, C.byref(uvp), ALL, None,
                                                                           dh.data_ptr(), None, C.byref(ts), stream))
            mean, mn = timed(tan)
            # 8 B of uv in, 18 rows out; 3 heights and 3 height tangents (+ normals) gathered
            report("tangent", mean, mn, n * (8 + 72 + 24 + vn), queries=n, uv=mode, smooth=smooth)
            del uv, prim, grad, dh, tbuf
            torch.cuda.empty_cache()

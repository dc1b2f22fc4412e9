#!/usr/bin/env python3
"""Time the sensor with HIP events.
On the benchmark's wavefront (1024 x 1024 x 64 spp = 67.1 M samples):
    hf_sensor_rays for both sensor types, with and without out_pos (36 / 28 bytes of stores per ray), in BOTH store
    variants (HF_SENSOR_STORE = dword: one sample per lane; wide: four per lane, 16-byte stores), alternated, and their
    outputs compared bit for bit;
    a device-to-device copy of the same number of bytes, timed in the same call and alternated with the kernel: the
    yardstick of a store-bound kernel (a copy also READS its bytes, so it moves twice what the kernel does);
    workload.ortho_rays on the device, what the orthographic type replaces as a camera.
On a 2048 x 2048 x 4 spp wavefront (16.8 M samples):
    hf_sensor_rays_tangent, hf_sensor_rays_adjoint (both types), hf_sensor_project, its tangent and its adjoint.
usage: python scripts/time_sensor.py [--warmup 3 --iters 20 --out profiles/sensor/times.jsonl] [--film 1024 --spp 64]
One JSON line per measurement (median / min / mean ms over the timed calls)."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--film", type=int, default=1024)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--film2", type=int, default=2048, help="the film of the derivative and projection timings")
ap.add_argument("--spp2", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
assert torch.cuda.is_available(), "time_sensor.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")


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
    rec = dict(kind=kind, ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_mean=round(sum(ms) / len(ms), 4),
               iters=len(ms), **extra)
    print(json.dumps(rec), flush=True)
    if out_f:
        out_f.write(json.dumps(rec) + "\n"); out_f.flush()
    return rec["ms_median"]


lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
KW = dict(origin=(1.5, 1.5, 1.5), target=(0.0, 0.0, 0.125), up=(0.0, 0.0, 1.0))
cams = {"perspective": hf_amd.PerspectiveCamera.look_at(fov=35.0, film=(a.film, a.film), **KW),
        "orthographic": hf_amd.OrthographicCamera.look_at(scale=(1.6, 1.6, 1.0), film=(a.film, a.film), **KW)}

# ---- the wavefront of the benchmark ----
n = a.film * a.film * a.spp
scene = dict(film=a.film, spp=a.spp, samples=n)
buf = torch.empty((9, n), dtype=torch.float32, device=dev)
src = torch.randn((9, n), dtype=torch.float32, device=dev)
o, d, maxt, pos = buf[0:3], buf[3:6], buf[6], buf[7:9]
for name, cam in cams.items():
    S = cam._struct(cam.to_world, cam.fov)
    for with_pos in (True, False):
        k = 9 if with_pos else 7
        def kern(store):
            os.environ["HF_SENSOR_STORE"] = store         # the test hook of include/hf.h, read at every launch
            _capi.check(lib.hf_sensor_rays(S, n, 0, a.spp, 0, None, rows(o), rows(d), maxt.data_ptr(),
                                           rows(pos) if with_pos else None, stream))
        copy = lambda: buf[:k].copy_(src[:k])
        kern("dword"); ref = buf[:k].clone(); kern("wide")
        same = bool(torch.equal(ref.view(torch.int32), buf[:k].view(torch.int32)))
        del ref
        dw, wd, cp = [], [], []
        for _ in range(2):                                # dword, wide and the copy alternate: all see the same machine
            dw += timed(lambda: kern("dword")); wd += timed(lambda: kern("wide")); cp += timed(copy)
        tag = f"{name}" + ("_with_pos" if with_pos else "")
        td = report(f"sensor_rays_{tag}", dw, **scene, bytes_stored=4 * k * n, store_variant="dword: one sample per lane, 4-byte stores")
        tw = report(f"sensor_rays_{tag}", wd, **scene, bytes_stored=4 * k * n, store_variant="wide: four samples per lane, 16-byte stores",
                    same_bytes_as_dword=same)
        tc = report(f"device_copy_{4 * k}_bytes_per_ray", cp, **scene, bytes_copied=4 * k * n)
        report(f"ratio_to_copy_{tag}", [td / tc], **scene, store_variant="dword")
        report(f"ratio_to_copy_{tag}", [tw / tc], **scene, store_variant="wide")
os.environ.pop("HF_SENSOR_STORE", None)
with torch.no_grad():
    want = hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)
    S = cams["orthographic"]._struct(cams["orthographic"].to_world, None)
    _capi.check(lib.hf_sensor_rays(S, n, 0, a.spp, 0, None, rows(o), rows(d), maxt.data_ptr(), None, stream))
    same = dict(d_bitwise=bool(torch.equal(d, want[3:6])), maxt_bitwise=bool(torch.equal(maxt, want[6])),
                o_max_abs_difference=float((o - want[0:3]).abs().max()))
    del want
    report("workload_ortho_rays_on_device", timed(lambda: hf_amd.workload.ortho_rays(a.film, a.film, a.spp, dev)), **scene, **same)
del buf, src, o, d, maxt, pos
torch.cuda.empty_cache()

# ---- derivatives and the way back ----
n = a.film2 * a.film2 * a.spp2
scene = dict(film=a.film2, spp=a.spp2, samples=n)
dtw, dfov = torch.randn(12, device=dev) * 0.1, torch.full((1,), 0.5, device=dev)
ro, rd, go, gd, gp = (torch.randn((3, n), device=dev) for _ in range(5))
uv, guv = torch.empty((2, n), device=dev), torch.randn((2, n), device=dev)
w, gw = torch.empty(n, device=dev), torch.randn(n, device=dev)
valid = torch.empty(n, dtype=torch.uint8, device=dev)
g12, gf = torch.zeros(12, device=dev), torch.zeros(1, device=dev)
ws = torch.empty(lib.hf_sensor_workspace_floats(), dtype=torch.float32, device=dev)
for name in cams:
    cam = type(cams[name]).look_at(film=(a.film2, a.film2), **KW, **(dict(fov=35.0) if name == "perspective" else dict(scale=(1.6, 1.6, 1.0))))
    S = cam._struct(cam.to_world, cam.fov)
    head = (S, n, 0, a.spp2, 0, None)
    report(f"sensor_rays_tangent_{name}", timed(lambda: _capi.check(lib.hf_sensor_rays_tangent(
        *head, dtw.data_ptr(), dfov.data_ptr(), rows(ro), rows(rd), stream))), **scene)
    report(f"sensor_rays_adjoint_{name}", timed(lambda: _capi.check(lib.hf_sensor_rays_adjoint(
        *head, rows(go), rows(gd), g12.data_ptr(), gf.data_ptr(), ws.data_ptr(), stream))), **scene)
    if name == "perspective":
        mt = torch.empty(n, device=dev)
        _capi.check(lib.hf_sensor_rays(*head, rows(ro), rows(rd), mt.data_ptr(), None, stream))
        p = (ro + rd * 1.5).contiguous()
        del mt
        report("sensor_project", timed(lambda: _capi.check(lib.hf_sensor_project(
            S, n, rows(p), None, rows(uv), valid.data_ptr(), w.data_ptr(), stream))), **scene, valid=int(valid.sum()))
        report("sensor_project_tangent", timed(lambda: _capi.check(lib.hf_sensor_project_tangent(
            S, n, rows(p), None, rows(go), dtw.data_ptr(), dfov.data_ptr(), rows(uv), w.data_ptr(), stream))), **scene)
        report("sensor_project_adjoint", timed(lambda: _capi.check(lib.hf_sensor_project_adjoint(
            S, n, rows(p), None, rows(guv), gw.data_ptr(), rows(gp), g12.data_ptr(), gf.data_ptr(), ws.data_ptr(), stream))), **scene)
assert np.isfinite(float(g12.sum()))

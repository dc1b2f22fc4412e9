#!/usr/bin/env python3
"""Time the thin lens with HIP events, in the manner of scripts/time_sensor.py.
On the benchmark's wavefront (1024 x 1024 x 64 spp = 67.1 M samples), with out_pos (36 bytes of stores per ray),
alternated in one process so that all see the same machine:
    hf_thinlens_rays in BOTH store variants (HF_SENSOR_STORE = dword: one sample per lane; wide: four per lane, 16-byte
    stores), their outputs compared bit for bit;
    hf_sensor_rays of the perspective type in both variants: what the lens adds is one TEA draw and the disk;
    a device-to-device copy of the same number of bytes: the yardstick of a store-bound kernel (a copy also READS its
    bytes, so it moves twice what the kernel does).
On a 2048 x 2048 x 4 spp wavefront (16.8 M samples):
    hf_thinlens_rays_tangent, hf_thinlens_rays_adjoint, hf_thinlens_project, its tangent and its adjoint.
usage: python scripts/time_thinlens.py [--warmup 3 --iters 20 --out profiles/thinlens/times.jsonl] [--film 1024 --spp 64]
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
assert torch.cuda.is_available(), "time_thinlens.py measures on a HIP device; there is none"
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
LENS = dict(aperture_radius=0.05, focus_distance=2.0)


def cameras(film):
    lens = hf_amd.ThinLensCamera.look_at(fov=35.0, film=(film, film), **LENS, **KW)
    pin = hf_amd.PerspectiveCamera.look_at(fov=35.0, film=(film, film), **KW)
    return (lens._lens_struct(lens.to_world, lens.fov, lens.aperture_radius, lens.focus_distance), pin._struct(pin.to_world, pin.fov))


# ---- the wavefront of the benchmark ----
n = a.film * a.film * a.spp
scene = dict(film=a.film, spp=a.spp, samples=n, **LENS)
buf = torch.empty((9, n), dtype=torch.float32, device=dev)
src = torch.randn((9, n), dtype=torch.float32, device=dev)
o, d, maxt, pos = buf[0:3], buf[3:6], buf[6], buf[7:9]
L, S = cameras(a.film)


def kern(entry, st, store):
    os.environ["HF_SENSOR_STORE"] = store         # the test hook of include/hf.h, read at every launch
    _capi.check(entry(st, n, 0, a.spp, 0, None, rows(o), rows(d), maxt.data_ptr(), rows(pos), stream))


copy = lambda: buf.copy_(src)
kern(lib.hf_thinlens_rays, L, "dword"); ref = buf.clone(); kern(lib.hf_thinlens_rays, L, "wide")
same = bool(torch.equal(ref.view(torch.int32), buf.view(torch.int32)))
del ref
t = {k: [] for k in ("lens_dword", "lens_wide", "pin_dword", "pin_wide", "copy")}
for _ in range(2):                                # the five alternate: all see the same machine
    t["lens_dword"] += timed(lambda: kern(lib.hf_thinlens_rays, L, "dword"))
    t["pin_dword"] += timed(lambda: kern(lib.hf_sensor_rays, S, "dword"))
    t["lens_wide"] += timed(lambda: kern(lib.hf_thinlens_rays, L, "wide"))
    t["pin_wide"] += timed(lambda: kern(lib.hf_sensor_rays, S, "wide"))
    t["copy"] += timed(copy)
os.environ.pop("HF_SENSOR_STORE", None)
DW, WD = "dword: one sample per lane, 4-byte stores", "wide: four samples per lane, 16-byte stores"
m = {"lens_dword": report("thinlens_rays_with_pos", t["lens_dword"], **scene, bytes_stored=36 * n, store_variant=DW),
     "lens_wide": report("thinlens_rays_with_pos", t["lens_wide"], **scene, bytes_stored=36 * n, store_variant=WD, same_bytes_as_dword=same),
     "pin_dword": report("sensor_rays_perspective_with_pos", t["pin_dword"], **scene, bytes_stored=36 * n, store_variant=DW),
     "pin_wide": report("sensor_rays_perspective_with_pos", t["pin_wide"], **scene, bytes_stored=36 * n, store_variant=WD),
     "copy": report("device_copy_36_bytes_per_ray", t["copy"], **scene, bytes_copied=36 * n)}
for v in ("dword", "wide"):
    report("ratio_thinlens_to_perspective", [m[f"lens_{v}"] / m[f"pin_{v}"]], **scene, store_variant=v)
    report("ratio_thinlens_to_copy", [m[f"lens_{v}"] / m["copy"]], **scene, store_variant=v)
del buf, src, o, d, maxt, pos
torch.cuda.empty_cache()

# ---- derivatives and the way back ----
n = a.film2 * a.film2 * a.spp2
scene = dict(film=a.film2, spp=a.spp2, samples=n, **LENS)
dtw = torch.randn(12, device=dev) * 0.1
dfov, dr, dfo = (torch.full((1,), v, device=dev) for v in (0.5, 0.1, -0.2))
ro, rd, go, gd, gp = (torch.randn((3, n), device=dev) for _ in range(5))
uv, guv = torch.empty((2, n), device=dev), torch.randn((2, n), device=dev)
w, gw = torch.empty(n, device=dev), torch.randn(n, device=dev)
valid = torch.empty(n, dtype=torch.uint8, device=dev)
g = torch.zeros(15, device=dev)
gptr = [g.data_ptr() + 4 * k for k in (0, 12, 13, 14)]
ws = torch.empty(lib.hf_thinlens_workspace_floats(), dtype=torch.float32, device=dev)
L, _ = cameras(a.film2)
head = (L, n, 0, a.spp2, 0, None)
report("thinlens_rays_tangent", timed(lambda: _capi.check(lib.hf_thinlens_rays_tangent(
    *head, dtw.data_ptr(), dfov.data_ptr(), dr.data_ptr(), dfo.data_ptr(), rows(ro), rows(rd), stream))), **scene)
report("thinlens_rays_adjoint", timed(lambda: _capi.check(lib.hf_thinlens_rays_adjoint(
    *head, rows(go), rows(gd), *gptr, ws.data_ptr(), stream))), **scene)
mt = torch.empty(n, device=dev)
_capi.check(lib.hf_thinlens_rays(*head, rows(ro), rows(rd), mt.data_ptr(), None, stream))
p = (ro + rd * 1.5).contiguous()
del mt
phead = (L, n, 0, 0, None, rows(p), None)
report("thinlens_project", timed(lambda: _capi.check(lib.hf_thinlens_project(
    *phead, rows(uv), valid.data_ptr(), w.data_ptr(), stream))), **scene, valid=int(valid.sum()))
report("thinlens_project_tangent", timed(lambda: _capi.check(lib.hf_thinlens_project_tangent(
    *phead, rows(go), dtw.data_ptr(), dfov.data_ptr(), dr.data_ptr(), dfo.data_ptr(), rows(uv), w.data_ptr(), stream))), **scene)
report("thinlens_project_adjoint", timed(lambda: _capi.check(lib.hf_thinlens_project_adjoint(
    *phead, rows(guv), gw.data_ptr(), rows(gp), *gptr, ws.data_ptr(), stream))), **scene)
assert np.isfinite(float(g.sum()))

#!/usr/bin/env python3
"""Time the bump map with HIP events on scripts/time_normalmap.py's scene and protocol -- a 2048 x 2048 x 4 spp
orthographic wavefront (16.8 M samples) over the 4096^2 sine field -- with a 1024^2 relief (tests/bumpmap_ref.texture):
    the fused forward (hf_bumpmap_eval: N and the mask), the fused tangent (all five tangents) and the fused adjoint without
    grad_tex (grad_uv, grad_sh_n, grad_dp_du, grad_dp_dv) and with it (four float atomics per run of samples more), through
    the C ABI;
    the only way a user had before: the same map written in plain torch -- four gathers of the texels, the slopes, the
    projected tangents and the cross product over [n] rows --, its autograd backward (all five inputs attached) and its
    forward-mode tangent;
    forward + backward through the public class (BumpMap.normal) against forward + backward of the torch map.
usage: python scripts/time_bumpmap.py [--warmup 2 --iters 10 --out profiles/bumpmap/times.jsonl]
                                      [--grid 4096 --film 2048 --spp 4 --tex 1024] [--plain-lib libhf_plain.so]
--plain-lib: the same library built with -DHF_BUMPMAP_MERGE=0 (the adjoint's texel scatter without the wave-level merge of
lanes that share a cell); its adjoint with grad_tex is timed alternately with this one's.
One JSON line per measurement (median / min / max / mean ms over the timed calls; the compared pair alternates in one
process so that both see the same machine).  The fused N is compared with the torch map's first."""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--film", type=int, default=2048)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--tex", type=int, default=1024)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--out", default=None)
ap.add_argument("--plain-lib", default=None, help="a build of libhf.so with -DHF_BUMPMAP_MERGE=0: its adjoint is timed against this one's")
a = ap.parse_args()
assert a.warmup >= 2 and a.iters >= 5, "the protocol: 2 warm-ups, at least 5 timed calls"

import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
import bumpmap_ref as R  # noqa: E402
assert torch.cuda.is_available(), "time_bumpmap.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, tex=a.tex, scale=a.scale)
WRAP = "repeat"


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
n = len(ray)
uv, sn, ng, du, dv = (x.detach().contiguous() for x in (si.uv, si.sh_frame.n, si.n, si.dp_du, si.dp_dv))
act = si.is_valid().to(torch.uint8).contiguous()
hit = act.bool()
del si, rays, ray, shape
tex = torch.from_numpy(R.texture(a.tex, a.tex)).to(dev)
TW = TH = a.tex
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
head = (n, rows(uv), rows(sn), rows(ng), rows(du), rows(dv), act.data_ptr(), TW, TH, tex.data_ptr(), _capi.HF_WRAP_REPEAT, a.scale)


def gathers(data, uv_, b, u, v):
    """what the fused forward replaces: the map in plain torch (repeat wrap), four gathers and the frame algebra over rows"""
    qx, qy = uv_[0] * float(TW) - 0.5, uv_[1] * float(TH) - 0.5
    x0, y0 = torch.floor(qx.detach()), torch.floor(qy.detach())
    fx, fy = qx - x0, qy - y0
    ix0, iy0 = torch.remainder(x0.long(), TW), torch.remainder(y0.long(), TH)
    ix1, iy1 = torch.remainder(ix0 + 1, TW), torch.remainder(iy0 + 1, TH)
    flat = data.reshape(-1)
    v00, v10, v01, v11 = flat[iy0 * TW + ix0], flat[iy0 * TW + ix1], flat[iy1 * TW + ix0], flat[iy1 * TW + ix1]
    Lx = (1.0 - fy) * (v10 - v00) + fy * (v11 - v01)
    Ly = (1.0 - fx) * (v01 - v00) + fx * (v11 - v10)
    gx, gy = a.scale * TW * Lx, a.scale * TH * Ly
    Pu = u + b * (gx - (b * u).sum(0)).unsqueeze(0)
    Pv = v + b * (gy - (b * v).sum(0)).unsqueeze(0)
    c = torch.linalg.cross(Pu, Pv, dim=0)
    sigma = torch.where((ng * c.detach()).sum(0) < 0, -1.0, 1.0)
    Nn = c * (sigma / torch.linalg.vector_norm(c, dim=0)).unsqueeze(0)
    return torch.where(hit.unsqueeze(0), Nn, b)


N, mask = torch.empty_like(sn), torch.empty(n, dtype=torch.uint8, device=dev)
fused_forward = lambda: _capi.check(lib.hf_bumpmap_eval(*head, rows(N), mask.data_ptr(), stream))
with torch.no_grad():
    fused_forward()
    ref = gathers(tex, uv, sn, du, dv)
    diff = (N - ref)[:, hit & mask.bool()].abs()
    info = dict(samples=n, hits=int(hit.sum()), perturbed=int(mask.sum()),
                fused_against_torch_max_abs_diff=float(diff.max()), fused_against_torch_share_above_1e_5=float((diff.amax(0) > 1e-5).float().mean()))
    del ref, diff
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert info["perturbed"] == info["hits"], "a hit sample passed through"

# ---- forward
with torch.no_grad():
    f1 = timed(fused_forward)
    s1 = timed(lambda: gathers(tex, uv, sn, du, dv))
    f2 = timed(fused_forward)
    s2 = timed(lambda: gathers(tex, uv, sn, du, dv))
report("fused_forward", f1, **info)
report("torch_gathers_forward", s1)
report("fused_forward_again", f2)
report("torch_gathers_forward_again", s2)

# ---- adjoint: the C entry without and with grad_tex
gout = torch.randn(3, n, device=dev)
gtex, guv, gn, gpu, gpv = torch.zeros_like(tex), torch.empty_like(uv), torch.empty_like(sn), torch.empty_like(du), torch.empty_like(dv)
adj = lambda with_tex: _capi.check(lib.hf_bumpmap_eval_adjoint(*head, rows(gout), gtex.data_ptr() if with_tex else None, rows(guv),
                                                               rows(gn), rows(gpu), rows(gpv), stream))
a1 = timed(lambda: adj(False))
b1 = timed(lambda: adj(True))
a2 = timed(lambda: adj(False))
b2 = timed(lambda: adj(True))
c1 = timed(lambda: _capi.check(lib.hf_bumpmap_eval_adjoint(*head, rows(gout), gtex.data_ptr(), None, None, None, None, stream)))
report("fused_adjoint_without_grad_tex", a1)
report("fused_adjoint_with_grad_tex", b1)
report("fused_adjoint_without_grad_tex_again", a2)
report("fused_adjoint_with_grad_tex_again", b2)
report("fused_adjoint_grad_tex_only", c1)
if a.plain_lib:
    # the adjoint's texel scatter without the wave-level merge of lanes that share a cell: the same library built with
    # -DHF_BUMPMAP_MERGE=0, loaded beside this one; the two alternate
    plain = C.CDLL(a.plain_lib).hf_bumpmap_eval_adjoint
    plain.restype, plain.argtypes = _capi.SYMBOLS["hf_bumpmap_eval_adjoint"]
    adj_plain = lambda: _capi.check(plain(*head, rows(gout), gtex.data_ptr(), rows(guv), rows(gn), rows(gpu), rows(gpv), stream))
    gtex.zero_(); adj(True); merged = gtex.clone()
    gtex.zero_(); adj_plain()
    rel = float(torch.linalg.vector_norm(merged.double() - gtex.double()) / torch.linalg.vector_norm(gtex.double()))
    del merged
    m1 = timed(lambda: adj(True))
    p1 = timed(adj_plain)
    m2 = timed(lambda: adj(True))
    p2 = timed(adj_plain)
    report("fused_adjoint_with_grad_tex_merged_runs", m1, grad_tex_relative_l2_between_the_two=rel)
    report("fused_adjoint_with_grad_tex_plain_scatter", p1)
    report("fused_adjoint_with_grad_tex_merged_runs_again", m2)
    report("fused_adjoint_with_grad_tex_plain_scatter_again", p2)
del gtex, guv, gn, gpu, gpv


def leaves(with_tex=True):
    return [x.detach().clone().requires_grad_(k > 0 or with_tex) for k, x in enumerate((tex, uv, sn, du, dv))]


def step_torch(with_tex=True):
    (gathers(*leaves(with_tex)) * gout).sum().backward()


def step_fused(with_tex=True):
    d, u_, b, p, q_ = leaves(with_tex)
    q = hf_amd.SurfaceInteraction3f()
    q.uv, q.n, q.dp_du, q.dp_dv, q.sh_frame = u_, ng, p, q_, hf_amd.Frame3f(None, None, b)
    (hf_amd.BumpMap(d, scale=a.scale, wrap=WRAP).normal(q, active=act) * gout).sum().backward()


for with_tex in (True, False):
    tag = "" if with_tex else "_texels_detached"
    p1 = timed(lambda: step_fused(with_tex))
    q1 = timed(lambda: step_torch(with_tex))
    p2 = timed(lambda: step_fused(with_tex))
    q2 = timed(lambda: step_torch(with_tex))
    report("class_forward_plus_backward" + tag, p1)
    report("torch_gathers_forward_plus_autograd_backward" + tag, q1)
    report("class_forward_plus_backward_again" + tag, p2)
    report("torch_gathers_forward_plus_autograd_backward_again" + tag, q2)
# (what both sides pay besides the map: five clones, the product with gout, its sum and its backward)
report("leaves_product_sum_backward_alone", timed(lambda: (leaves()[2] * gout).sum().backward()))

# ---- tangent
dtex, duv, dn = torch.randn_like(tex), 0.01 * torch.randn_like(uv), torch.randn_like(sn)
dpu, dpv = torch.randn_like(du), torch.randn_like(dv)
dN = torch.empty_like(sn)
fused_tangent = lambda: _capi.check(lib.hf_bumpmap_eval_tangent(*head, dtex.data_ptr(), rows(duv), rows(dn), rows(dpu), rows(dpv),
                                                                rows(dN), stream))


def torch_tangent():
    with fwAD.dual_level():
        x = [fwAD.make_dual(p, t) for p, t in ((tex, dtex), (uv, duv), (sn, dn), (du, dpu), (dv, dpv))]
        return fwAD.unpack_dual(gathers(*x)).tangent


t1 = timed(fused_tangent)
u1 = timed(torch_tangent)
t2 = timed(fused_tangent)
u2 = timed(torch_tangent)
report("fused_tangent", t1)
report("torch_gathers_forward_mode_tangent", u1)
report("fused_tangent_again", t2)
report("torch_gathers_forward_mode_tangent_again", u2)

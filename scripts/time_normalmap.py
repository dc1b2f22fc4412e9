#!/usr/bin/env python3
"""Time the normal map with HIP events on scripts/time_spot.py's scene -- a 2048 x 2048 x 4 spp orthographic wavefront
(16.8 M samples) over the 4096^2 sine field -- with a 1024^2 map (tests/normalmap_ref.texture's field of tilted normals):
    the fused forward (hf_normalmap_eval: N and the mask), the fused tangent (all four tangents) and the fused adjoint
    without grad_tex (grad_uv, grad_sh_n, grad_dp_du) and with it (twelve float atomics per sample more), through the C ABI;
    the sequence they replace, built only from what the library had before: three Bitmap.eval launches on the planes +
    the frame algebra in torch over [3, n] rows, its autograd backward (all four inputs attached) and its forward-mode
    tangent;
    forward + backward through the public class (NormalMap.normal) against forward + backward of the sequence.
usage: python scripts/time_normalmap.py [--warmup 2 --iters 10 --out profiles/normalmap/times.jsonl]
                                        [--grid 4096 --film 2048 --spp 4 --tex 1024] [--plain-lib libhf_plain.so]
--plain-lib: the same library built with -DHF_NORMALMAP_MERGE=0 (the adjoint's texel scatter without the wave-level merge of
lanes that share a cell); its adjoint with grad_tex is timed alternately with this one's.
One JSON line per measurement (median / min / max / mean ms over the timed calls; the compared pair alternates in one
process so that both see the same machine).  The fused N is compared with the sequence's first."""
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
ap.add_argument("--out", default=None)
ap.add_argument("--plain-lib", default=None, help="a build of libhf.so with -DHF_NORMALMAP_MERGE=0: its adjoint is timed against this one's")
a = ap.parse_args()
assert a.warmup >= 2 and a.iters >= 5, "the protocol: 2 warm-ups, at least 5 timed calls"

import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402
import hf_amd  # noqa: E402
from hf_amd import _capi  # noqa: E402
import normalmap_ref as R  # noqa: E402
assert torch.cuda.is_available(), "time_normalmap.py measures on a HIP device; there is none"
dev = torch.device("cuda", 0)
out_f = None
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_f = open(a.out, "w")
scene = dict(grid=a.grid, film=a.film, spp=a.spp, tex=a.tex)
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
uv, sn, du = (x.detach().contiguous() for x in (si.uv, si.sh_frame.n, si.dp_du))
act = si.is_valid().to(torch.uint8).contiguous()
del si, rays, ray, shape
tex = torch.from_numpy(R.texture(a.tex, a.tex)).to(dev)
TW = TH = a.tex
lib, stream = _capi.lib(), torch.cuda.current_stream(dev).cuda_stream
rows = lambda x: (C.c_void_p * x.shape[0])(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(x.shape[0])])
head = (n, rows(uv), rows(sn), rows(du), act.data_ptr(), TW, TH, tex.data_ptr(), _capi.HF_WRAP_REPEAT)


def sequence(data, uv_, b, u):
    """what the fused forward replaces: three Bitmap.eval launches + the frame algebra in torch"""
    pos = torch.stack([uv_[0] * float(TW), uv_[1] * float(TH)])
    c = torch.stack([hf_amd.Bitmap(data[k], wrap=WRAP).eval(pos, active=act) for k in range(3)])
    mt = 2.0 * c - 1.0
    m = mt / torch.linalg.vector_norm(mt, dim=0, keepdim=True)
    a_ = u - b * (b * u).sum(0, keepdim=True)
    s0 = a_ / torch.linalg.vector_norm(a_, dim=0, keepdim=True)
    t0 = torch.linalg.cross(b, s0, dim=0)
    return s0 * m[0:1] + t0 * m[1:2] + b * m[2:3]


N, mask = torch.empty_like(sn), torch.empty(n, dtype=torch.uint8, device=dev)
fused_forward = lambda: _capi.check(lib.hf_normalmap_eval(*head, rows(N), mask.data_ptr(), stream))
with torch.no_grad():
    fused_forward()
    ref = sequence(tex, uv, sn, du)
    hit = act.bool()
    info = dict(samples=n, hits=int(hit.sum()), perturbed=int(mask.sum()),
                fused_against_sequence_max_abs_diff=float((N - ref)[:, hit & mask.bool()].abs().max()))
    del ref
print(json.dumps(dict(kind="check", **scene, **info)), flush=True)
assert info["perturbed"] == info["hits"], "a hit sample passed through"

# ---- forward
with torch.no_grad():
    f1 = timed(fused_forward)
    s1 = timed(lambda: sequence(tex, uv, sn, du))
    f2 = timed(fused_forward)
    s2 = timed(lambda: sequence(tex, uv, sn, du))
report("fused_forward", f1, **info)
report("three_bitmap_eval_plus_torch_frame_algebra_forward", s1)
report("fused_forward_again", f2)
report("three_bitmap_eval_plus_torch_frame_algebra_forward_again", s2)

# ---- adjoint: the C entry without and with grad_tex, and forward + backward through autograd on both sides
gout = torch.randn(3, n, device=dev)
gtex, guv, gn, gp = torch.zeros_like(tex), torch.empty_like(uv), torch.empty_like(sn), torch.empty_like(du)
adj = lambda with_tex: _capi.check(lib.hf_normalmap_eval_adjoint(*head, rows(gout), gtex.data_ptr() if with_tex else None, rows(guv),
                                                                 rows(gn), rows(gp), stream))
a1 = timed(lambda: adj(False))
b1 = timed(lambda: adj(True))
a2 = timed(lambda: adj(False))
b2 = timed(lambda: adj(True))
c1 = timed(lambda: _capi.check(lib.hf_normalmap_eval_adjoint(*head, rows(gout), gtex.data_ptr(), None, None, None, stream)))
report("fused_adjoint_without_grad_tex", a1)
report("fused_adjoint_with_grad_tex", b1)
report("fused_adjoint_without_grad_tex_again", a2)
report("fused_adjoint_with_grad_tex_again", b2)
report("fused_adjoint_grad_tex_only", c1)
if a.plain_lib:
    # the adjoint's texel scatter without the wave-level merge of lanes that share a cell: the same library built with
    # -DHF_NORMALMAP_MERGE=0, loaded beside this one; the two alternate
    plain = C.CDLL(a.plain_lib).hf_normalmap_eval_adjoint
    plain.restype, plain.argtypes = _capi.SYMBOLS["hf_normalmap_eval_adjoint"]
    adj_plain = lambda: _capi.check(plain(*head, rows(gout), gtex.data_ptr(), rows(guv), rows(gn), rows(gp), stream))
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
del gtex, guv, gn, gp


def leaves(with_tex=True):
    return [v.detach().clone().requires_grad_(k > 0 or with_tex) for k, v in enumerate((tex, uv, sn, du))]


def step_sequence(with_tex=True):
    x = leaves(with_tex)
    (sequence(*x) * gout).sum().backward()


def step_fused(with_tex=True):
    d, u_, b, p = leaves(with_tex)
    q = hf_amd.SurfaceInteraction3f()
    q.uv, q.dp_du, q.sh_frame = u_, p, hf_amd.Frame3f(None, None, b)
    (hf_amd.NormalMap(d, wrap=WRAP).normal(q, active=act) * gout).sum().backward()


for with_tex in (True, False):
    tag = "" if with_tex else "_texels_detached"
    p1 = timed(lambda: step_fused(with_tex))
    q1 = timed(lambda: step_sequence(with_tex))
    p2 = timed(lambda: step_fused(with_tex))
    q2 = timed(lambda: step_sequence(with_tex))
    report("class_forward_plus_backward" + tag, p1)
    report("sequence_forward_plus_autograd_backward" + tag, q1)
    report("class_forward_plus_backward_again" + tag, p2)
    report("sequence_forward_plus_autograd_backward_again" + tag, q2)
# (what both sides pay besides the map: four clones, the product with gout, its sum and its backward)
report("leaves_product_sum_backward_alone", timed(lambda: (leaves()[2] * gout).sum().backward()))

# ---- tangent
dtex, duv, dn, dp = torch.randn_like(tex), 0.01 * torch.randn_like(uv), torch.randn_like(sn), torch.randn_like(du)
dN = torch.empty_like(sn)
fused_tangent = lambda: _capi.check(lib.hf_normalmap_eval_tangent(*head, dtex.data_ptr(), rows(duv), rows(dn), rows(dp), rows(dN), stream))


def sequence_tangent():
    with fwAD.dual_level():
        x = [fwAD.make_dual(v, t) for v, t in ((tex, dtex), (uv, duv), (sn, dn), (du, dp))]
        return fwAD.unpack_dual(sequence(*x)).tangent


t1 = timed(fused_tangent)
u1 = timed(sequence_tangent)
t2 = timed(fused_tangent)
u2 = timed(sequence_tangent)
report("fused_tangent", t1)
report("sequence_forward_mode_tangent", u1)
report("fused_tangent_again", t2)
report("sequence_forward_mode_tangent_again", u2)

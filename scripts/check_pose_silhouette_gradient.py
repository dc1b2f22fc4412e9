#!/usr/bin/env python3
"""The gradient table of DESIGN 4.13 for examples/inverse_pose.py --silhouette: d(pixel loss)/d(tx, ty, yaw) at the
example's start pose by central differences and by autograd in three forms --
  attached: no silhouette term (hf_adjoint_transform alone);
  fixed:    primary rays through reparameterize_ray, samples times the determinant, film positions held fixed;
  moving:   the example's form: the samples are also splatted at the film position of the reparameterised ray.
--native-film: every film is the library's (hf_amd.film_gaussian(..., weight=det)) instead of the example's splat().
usage: python scripts/check_pose_silhouette_gradient.py [--film 64 --spp 16 --aux 16 --kappa 2e4 --native-film --out FILE]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch
import hf_amd
import inverse_pose as ip

ap = argparse.ArgumentParser()
ap.add_argument("--film", type=int, default=64)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--aux", type=int, default=16)
ap.add_argument("--kappa", type=float, default=2e4)
ap.add_argument("--half", type=float, default=1.3)
ap.add_argument("--native-film", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
NF = a.native_film
dev = "cuda"
shape = hf_amd.Heightfield(heightfield=ip.field(device=dev), max_height=0.5, differentiable_to_world=True)
ray, pos = ip.pinhole(a.film, a.spp, dev, a.half)


def set_pose(p):
    shape.to_world = ip.pose_matrix(p)
    shape.parameters_changed(["to_world"])


with torch.no_grad():
    set_pose(torch.tensor(ip.TARGET, dtype=torch.float64))
    target = ip.render_silhouette(shape, ray, pos, a.film, a.half, reparam=False, native_film=NF)


def loss_of(p, mode):
    set_pose(p)
    if mode == "attached":
        img = ip.render_silhouette(shape, ray, pos, a.film, a.half, reparam=False, native_film=NF)
    elif mode == "moving":
        img = ip.render_silhouette(shape, ray, pos, a.film, a.half, a.aux, a.kappa, reparam=True, native_film=NF)
    else:
        d, det = hf_amd.reparameterize_ray(shape, ray, num_rays=a.aux, kappa=a.kappa, exponent=3.0)
        img = ip.film_of(ip.render(shape, hf_amd.Ray3f(ray.o, d, ray.maxt)) * det, det, pos, a.film, NF)
    return ((img - target) ** 2).mean()


lines = [f"{'native film (hf_film_splat_weighted): ' if NF else ''}film {a.film} spp {a.spp} aux {a.aux} kappa {a.kappa:g} half {a.half}: d(loss)/d(tx, ty, yaw) at {ip.START}"]
p0 = torch.tensor(ip.START, dtype=torch.float64)
for eps in (0.004, 0.008):
    fd = []
    for j in range(3):
        e = torch.zeros(3, dtype=torch.float64); e[j] = eps
        with torch.no_grad():
            fd.append(float(loss_of(p0 + e, "attached") - loss_of(p0 - e, "attached")) / (2 * eps))
    lines.append(f"central differences, step {eps}: " + "  ".join(f"{v:+.4e}" for v in fd))
for mode in ("attached", "fixed", "moving"):
    p = p0.clone().requires_grad_(True)
    loss_of(p, mode).backward()
    lines.append(f"{mode:9s}" + "  ".join(f"{float(v):+.4e}" for v in p.grad))
print("\n".join(lines))
if a.out:
    open(a.out, "w").write("\n".join(lines) + "\n")

#!/usr/bin/env python3
"""Pose recovery through the transform derivatives: Adam on a translation (tx, ty) and a yaw of a known 256^2 field,
starting from a perturbed pose, against renders of the target pose.

    to_world(tx, ty, yaw) = [[cos yaw, -sin yaw, 0, tx], [sin yaw, cos yaw, 0, ty], [0, 0, 1, 0]]
    image = world height of the visible point of every primary ray (orthographic, looking straight down)
    loss  = mean |image(pose) - image(target)|^2

The heightfield is created with differentiable_to_world=True; the pose's 3x4 matrix, built by torch from the three
parameters, is set as shape.to_world and takes effect at parameters_changed(["to_world"]); loss.backward() reaches the
parameters through hf_adjoint_transform.  The camera sees the interior of the field only, so every ray hits and the
image has no silhouette (the attached gradient is the whole derivative).

--silhouette looks at the whole field on a background of height 0 through a pinhole, so the image has a silhouette that
moves with the pose, and adds the discontinuity term the way prb_reparam.py:317-366 does for the camera ray: the
primary rays go through hf_amd.reparameterize_ray (identity in primal mode; --aux auxiliary rays per ray), the
intersection is differentiated with respect to the reparameterised direction as well, every sample is multiplied by the
determinant, AND the sample is splatted at the film position of the reparameterised ray with a smooth reconstruction
filter (splat(): a radial Gaussian in torch, differentiable in the positions; --native-film: the library's film,
hf_amd.film_gaussian(vals * det, pos', film, film, weight=det), the separable filter of ImageBlock with its own adjoint
and tangent kernels).  The loss is then on the PIXELS.  Both are needed: the reparameterisation is a change of variables of the pixel integral,
so it holds for a loss on integrals, not on single samples, and only when the filter follows the warped ray -- with
samples kept in fixed pixels (a box film) the term div(f V) integrates to the flux of f V through the pixel edges,
which for a translating shape is as large as the interior gradient.  The backward reaches to_world
through hf_reparam_backward_full.

    python examples/inverse_pose.py [--steps 150 --film 64 --spp 4 --silhouette --aux 8 --native-film]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

TARGET = (0.0, 0.0, 0.0)            # tx, ty, yaw (radians)
START = (0.08, -0.06, math.radians(6.0))


def field(n=256, device="cuda"):
    """three Gaussian bumps of different sizes on a tilted plane: no symmetry, so the pose is identifiable"""
    u = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=device)
    X, Y = u[None, :], u[:, None]
    h = 0.3 + 0.1 * X - 0.05 * Y
    for cx, cy, r, a in ((-0.3, 0.2, 0.35, 0.5), (0.35, 0.1, 0.25, 0.35), (0.0, -0.35, 0.3, -0.3)):
        h = h + a * torch.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2 * r * r))
    return h.to(torch.float32)


def pose_matrix(p):
    """3x4 to_world of the pose p = (tx, ty, yaw), differentiable in p"""
    tx, ty, yaw = p[0], p[1], p[2]
    c, s = torch.cos(yaw), torch.sin(yaw)
    one, z = torch.ones_like(tx), torch.zeros_like(tx)
    return torch.stack([torch.stack([c, -s, z, tx]), torch.stack([s, c, z, ty]), torch.stack([z, z, one, z])])


def camera(film, spp, device):
    """orthographic rays looking down on the central +-0.55 of the field"""
    return hf_amd.workload.ortho_rays(film, film, spp, device, origin=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0),
                                      up=(0.0, 1.0, 0.0), scale=(0.55, 0.55, 1.0))


def render(shape, ray):
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    return torch.where(si.is_valid(), si.p[2], torch.zeros_like(si.t))


EYE = 3.0   # height of the pinhole of the silhouette view above the plane z = 0


def film_position(d, film, half):
    """film position (pixel units) of the direction d [3, n] through the pinhole (0, 0, EYE) that looks down on the
    square |x|, |y| <= half of the plane z = 0: differentiable in d"""
    s = -EYE / d[2]
    return torch.stack([(d[0] * s / half + 1.0) * (0.5 * film), (1.0 - d[1] * s / half) * (0.5 * film)])


def pinhole(film, spp, device, half):
    """(rays, film positions) of a perspective sensor: the warp of reparameterize_ray is one of the ray DIRECTION at a
    fixed origin, which is a change of variables of the pixel integral for a pinhole (for an orthographic sensor the
    integral is over the origins, and a direction does not name a film position)"""
    pos = hf_amd.workload.film_positions(film, film, spp, device)
    x = (pos[0] / (0.5 * film) - 1.0) * half
    y = (1.0 - pos[1] / (0.5 * film)) * half
    d = torch.stack([x, y, torch.full_like(x, -EYE)])
    d = d / d.norm(dim=0)
    o = torch.zeros_like(d); o[2] = EYE
    return hf_amd.Ray3f(o.contiguous(), d.contiguous()), pos


def splat(values, weights, pos, film, stddev=0.5, radius=2):
    """Gaussian reconstruction filter (src/rfilters/gaussian.cpp: exp(-r^2 / 2 stddev^2) minus its value at the radius)
    of per-sample values at film positions pos [2, n] (pixel units, pixel i covers [i, i + 1)), normalised by the
    splatted weights: [film * film], differentiable in values, weights and pos"""
    base = torch.floor(pos.detach()).long()
    alpha, bias = -0.5 / (stddev * stddev), math.exp(-0.5 * radius * radius / (stddev * stddev))
    img = torch.zeros(film * film, dtype=values.dtype, device=values.device)
    wsum = torch.zeros_like(img)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            px, py = base[0] + dx, base[1] + dy
            inside = (px >= 0) & (px < film) & (py >= 0) & (py < film)
            r2 = (pos[0] - (px + 0.5)) ** 2 + (pos[1] - (py + 0.5)) ** 2
            w = torch.clamp(torch.exp(alpha * r2) - bias, min=0.0) * inside
            idx = py.clamp(0, film - 1) * film + px.clamp(0, film - 1)
            img = img.index_add(0, idx, w * values)
            wsum = wsum.index_add(0, idx, w * weights)
    return img / wsum.clamp_min(1e-12)


def film_of(values, weights, pos, film, native_film=False):
    """the film [film * film] of weighted samples: splat(), or the library's film (ImageBlock::put(pos, value, weight))"""
    if native_film:
        return hf_amd.film_gaussian(values[None], pos, film, film, weight=weights)[0]
    return splat(values, weights, pos, film)


def render_silhouette(shape, ray, pos, film, half, aux=8, kappa=2e4, reparam=True, native_film=False):
    """the film [film * film] of the silhouette view.  reparam: primary rays through reparameterize_ray, values times the
    determinant, splatted at the film position of the reparameterised ray (prb_reparam.py:317-366, common.py:229-262:
    the sensor's film position of o + d').  In primal mode d' = d: pos keeps the value, the position's derivative moves"""
    if not reparam:
        return film_of(render(shape, ray), torch.ones_like(ray.o[0]), pos, film, native_film)
    d, det = hf_amd.reparameterize_ray(shape, ray, num_rays=aux, kappa=kappa, exponent=3.0)
    vals = render(shape, hf_amd.Ray3f(ray.o, d, ray.maxt))
    return film_of(vals * det, det, pos + (film_position(d, film, half) - film_position(d.detach(), film, half)), film,
                   native_film)


def recover_silhouette(steps=150, film=64, spp=4, lr=0.01, device="cuda", log=None, aux=8, reparam=True, half=1.3,
                       native_film=False):
    """recover() on the view that contains the whole field: a loss on the pixels of the Gaussian film.  reparam=False
    leaves the discontinuity term out (the attached gradient alone), for comparison; native_film: the library's film
    instead of splat(), for the target as well"""
    h = field(device=device)
    shape = hf_amd.Heightfield(heightfield=h, max_height=0.5, differentiable_to_world=True)
    ray, pos = pinhole(film, spp, device, half)
    with torch.no_grad():
        shape.to_world = pose_matrix(torch.tensor(TARGET, dtype=torch.float64))
        shape.parameters_changed(["to_world"])
        target = render_silhouette(shape, ray, pos, film, half, reparam=False, native_film=native_film)
    p = torch.tensor(START, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr)
    losses = []
    for k in range(steps):
        opt.zero_grad()
        shape.to_world = pose_matrix(p)
        shape.parameters_changed(["to_world"])
        loss = ((render_silhouette(shape, ray, pos, film, half, aux, reparam=reparam, native_film=native_film)
                 - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log and (k % 10 == 0 or k == steps - 1):
            log(f"step {k:4d}  loss {losses[-1]:.3e}  tx {float(p[0]):+.5f}  ty {float(p[1]):+.5f}  "
                f"yaw {math.degrees(float(p[2])):+.4f} deg")
    return TARGET, START, tuple(float(v) for v in p.detach()), losses


def recover(steps=150, film=64, spp=4, lr=0.01, device="cuda", log=None):
    """returns (target pose, start pose, final pose, losses)"""
    h = field(device=device)
    shape = hf_amd.Heightfield(heightfield=h, max_height=0.5, differentiable_to_world=True)
    rays = camera(film, spp, device)
    ray = hf_amd.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    with torch.no_grad():
        shape.to_world = pose_matrix(torch.tensor(TARGET, dtype=torch.float64))
        shape.parameters_changed(["to_world"])
        target = render(shape, ray)
        assert bool(torch.isfinite(target).all())
    p = torch.tensor(START, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr)
    losses = []
    for k in range(steps):
        opt.zero_grad()
        shape.to_world = pose_matrix(p)
        shape.parameters_changed(["to_world"])
        img = render(shape, ray)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log and (k % 10 == 0 or k == steps - 1):
            log(f"step {k:4d}  loss {losses[-1]:.3e}  tx {float(p[0]):+.5f}  ty {float(p[1]):+.5f}  "
                f"yaw {math.degrees(float(p[2])):+.4f} deg")
    return TARGET, START, tuple(float(v) for v in p.detach()), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--film", type=int, default=64)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--silhouette", action="store_true", help="the whole field in view, reparameterised primary rays")
    ap.add_argument("--aux", type=int, default=8, help="auxiliary rays per primary ray of --silhouette")
    ap.add_argument("--native-film", action="store_true",
                    help="--silhouette: hf_amd.film_gaussian(..., weight=det) instead of the example's torch splat()")
    a = ap.parse_args()
    if a.silhouette:
        target, start, final, losses = recover_silhouette(a.steps, a.film, a.spp, a.lr, log=print, aux=a.aux,
                                                          native_film=a.native_film)
    else:
        target, start, final, losses = recover(a.steps, a.film, a.spp, a.lr, log=print)
    print(f"target {target}, start {start}, recovered {final}")


if __name__ == "__main__":
    main()

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

    python examples/inverse_pose.py [--steps 150 --film 64 --spp 4]
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
    a = ap.parse_args()
    target, start, final, losses = recover(a.steps, a.film, a.spp, a.lr, log=print)
    print(f"target {target}, start {start}, recovered {final}")


if __name__ == "__main__":
    main()

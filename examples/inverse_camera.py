#!/usr/bin/env python3
"""Camera recovery through the sensor's derivatives: Adam on the eye position (x, y), the yaw and the field of view of a
PerspectiveCamera that looks down on a known field, starting from a perturbed camera, against a render of the target one.

    to_world(ex, ey, yaw) = [Rz(yaw) look_down | (ex, ey, EYE)],   look_down = look_at((0, 0, EYE), (0, 0, 0), up = y)
    image = world height of the visible point of every primary ray
    loss  = mean |image(camera) - image(target)|^2

The pose's 3x4 matrix and the field of view are torch tensors built from the four parameters; cam.sample_rays() makes
the wavefront in one kernel (hf_sensor_rays) and loss.backward() reaches the parameters through shape.ray_intersect's
ray gradients and hf_sensor_rays_adjoint.  The camera sees the interior of the field only (inverse_pose.py's field), so
every ray hits and the image has no silhouette: the attached gradient is the whole derivative.  The eye's height is
known: over a field this flat it and the field of view scale the image alike, and one view does not tell them apart.

    python examples/inverse_camera.py [--steps 150 --film 64 --spp 4]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hf_amd  # noqa: E402
from inverse_pose import field  # noqa: E402

EYE = 3.0
TARGET = (0.0, 0.0, 0.0, 20.0)                          # eye x, eye y, yaw (radians), fov (degrees)
START = (0.06, -0.05, math.radians(5.0), 22.0)
LR = (0.004, 0.004, 0.005, 0.12)                        # per parameter: about a fifteenth of the start's error


def pose_matrix(p):
    """3x4 to_world of the camera p = (ex, ey, yaw, .), differentiable in p: a rotation about z after the look-down frame
    (left, up, dir) = (-x, y, -z)"""
    c, s = torch.cos(p[2]), torch.sin(p[2])
    z, one = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([torch.stack([-c, -s, z, p[0]]), torch.stack([-s, c, z, p[1]]), torch.stack([z, z, -one, EYE * one])])


def render(shape, cam, p, spp):
    cam.to_world, cam.fov = pose_matrix(p), p[3]
    ray, _, _ = cam.sample_rays(spp)
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    return si.p[2], si.is_valid()


def recover(steps=150, film=64, spp=4, device="cuda", log=None):
    """returns (target, start, final parameters, losses)"""
    shape = hf_amd.Heightfield(heightfield=field(device=device), max_height=0.5)
    cam = hf_amd.PerspectiveCamera(pose_matrix(torch.tensor(TARGET, dtype=torch.float64)), TARGET[3], film=(film, film))
    with torch.no_grad():
        target, hit = render(shape, cam, torch.tensor(TARGET, dtype=torch.float64), spp)
        assert bool(hit.all()), "the target view leaves the field"
    ps = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in START]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(ps, LR)])
    losses = []
    for k in range(steps):
        opt.zero_grad()
        img, _ = render(shape, cam, ps, spp)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log and (k % 10 == 0 or k == steps - 1):
            log(f"step {k:4d}  loss {losses[-1]:.3e}  eye ({float(ps[0]):+.5f}, {float(ps[1]):+.5f})  "
                f"yaw {math.degrees(float(ps[2])):+.4f} deg  fov {float(ps[3]):.4f} deg")
    return TARGET, START, tuple(float(q.detach()) for q in ps), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--film", type=int, default=64)
    ap.add_argument("--spp", type=int, default=4)
    a = ap.parse_args()
    target, start, final, losses = recover(a.steps, a.film, a.spp, log=print)
    print(f"target {target}, start {start}, recovered {final}")


if __name__ == "__main__":
    main()

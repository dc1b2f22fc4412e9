#!/usr/bin/env python3
"""Focus recovery through the thin lens's derivatives: Adam on the focus distance and the aperture radius of a
ThinLensCamera that looks down on a known terrain, against one render of the target lens.

    image = the terrain (smooth shading normals) under two directional lights, seen through the lens: every sample's ray
            leaves its own point of the aperture, a pixel is the mean of its samples (box film)
    loss  = mean |image(lens) - image(target)|^2

focus_distance and aperture_radius are torch scalars; cam.sample_rays() makes the wavefront in one kernel
(hf_thinlens_rays) and loss.backward() reaches them through direct_lighting, shape.ray_intersect's ray gradients and
hf_thinlens_rays_adjoint.  The target and the iterate draw the SAME samples (one seed: the same film jitter and the same
aperture points), so the loss is zero at the target and what is left is the lens alone.  The camera sees the interior of
the field only, so every ray hits and the image has no silhouette: the attached gradient is the whole derivative.  The
depth of the terrain varies over the view (2.6 to 3.0 below the eye), and the blur circle r |z / f - 1| of a point at
depth z tells the two parameters apart through that variation only: the radius is the slower of the two.

    python examples/inverse_focus.py [--steps 150 --size 64 --spp 8]
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

EYE, FOV, SEED = 3.0, 20.0, 7
TARGET = (2.0, 0.30)                                    # focus_distance, aperture_radius
START = (2.5, 0.20)
LR = (0.02, 0.005)                                      # per parameter: about a twenty-fifth of the start's error
LIGHTS = torch.tensor([[0.5, 0.2, 0.84], [-0.4, -0.5, 0.77]])


def lights(device):
    return torch.cat([LIGHTS / LIGHTS.norm(dim=1, keepdim=True), torch.full((len(LIGHTS), 1), math.pi)], 1).to(device)


def render(shape, cam, p, spp, lamps):
    """[K, pixels]: the view through the lens p = (focus_distance, aperture_radius)"""
    cam.focus_distance, cam.aperture_radius = p[0], p[1]
    ray, _, _ = cam.sample_rays(spp, seed=SEED)
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    return hf_amd.direct_lighting(si, ray, lamps, albedo=1.0, spp=spp), si.is_valid()


def recover(steps=150, size=64, spp=8, device="cuda", log=None):
    """returns (target, start, final parameters, losses)"""
    shape = hf_amd.Heightfield(heightfield=field(device=device), max_height=0.5, face_normals=False)
    cam = hf_amd.ThinLensCamera.look_at((0.0, 0.0, EYE), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV, TARGET[1], TARGET[0],
                                        film=(size, size))
    lamps = lights(device)
    with torch.no_grad():
        target, hit = render(shape, cam, torch.tensor(TARGET, dtype=torch.float64), spp, lamps)
        assert bool(hit.all()), "the target view leaves the field"
    ps = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in START]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(ps, LR)])
    losses = []
    for k in range(steps):
        opt.zero_grad()
        img, _ = render(shape, cam, ps, spp, lamps)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():                           # the lens's domain: f > 0, r >= 0
            ps[0].clamp_(min=0.1)
            ps[1].clamp_(min=0.0)
        losses.append(float(loss.detach()))
        if log and (k % 10 == 0 or k == steps - 1):
            log(f"step {k:4d}  loss {losses[-1]:.3e}  focus_distance {float(ps[0].detach()):.4f}  aperture_radius {float(ps[1].detach()):.4f}")
    return TARGET, START, tuple(float(q.detach()) for q in ps), losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--spp", type=int, default=8)
    a = ap.parse_args()
    target, start, final, losses = recover(a.steps, a.size, a.spp, log=print)
    print(f"target {target}, start {start}, recovered {final}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Recover the density and the anisotropy of a haze over a known terrain from one image per light.

    python examples/inverse_fog.py [--steps 120 --size 64]

A homogeneous medium (the reference's `homogeneous` with the `hg` phase function) fills the space below z = 1.5 over a
known relief; two directional lights, a raking one and a high one, are switched on in turn and an orthographic camera
above the haze takes one image per light.  Every step:
    si = shape.ray_intersect(ray)                                       fused traversal + surface interaction
    fog = hf_amd.medium_lighting(shape, si, ray, rig, medium)           ONE fused HIP launch: 8 points per primary ray,
                                                                        their shadow rays through the haze ("god rays")
    value = hf_amd.directional_lighting(..., return_value=True)         the surface term with its cast shadows
    image = fog + film(value * hf_amd.medium_attenuation(...))          the surface seen and lit through the haze
    loss = mean((image - target)^2);  loss.backward()                   hf_medium_lighting_adjoint
torch's Adam runs on sigma_t and g through the kernel's reduced gradients (3 numbers of the medium, one per light) and
through the closed-form attenuation; the two lights see the phase function at two angles, which separates g from the
density.  The visibility of every point is held, as everywhere: the silhouette part of a moving shadow is hf_reparam_*'s."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
STEPS = 8                                     # points per primary ray
RIG = (((-1.0, -0.2, 0.35), 3.0), ((0.3, 0.2, 0.9), 3.0))      # (to_light, irradiance)
TARGET = (0.6, 0.5)                           # sigma_t, g
START = (0.3, 0.1)
TOP = (0.0, 0.0, 1.5)
ALBEDO = 0.8                                  # of the haze and of the surface


def run(size=64, steps=120, lr=0.02, device="cuda", verbose=True):
    """returns (the loss history, (sigma_t, g) at the start, at the end, the target)"""
    dev = torch.device(device)
    shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(size, size, device=dev), max_height=0.5)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=(1.8, 0.5, 2.25), target=(0.0, 0.0, 0.25),
                                      scale=(0.95, 0.95, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    rig = [hf_amd.DirectionalLight(v, E) for v, E in RIG]
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)         # the terrain is known: one intersection for every step
    with torch.no_grad():
        surface = hf_amd.directional_lighting(shape, si, ray, rig, albedo=ALBEDO, spp=SPP, return_value=True)[1]

    def render(sigma_t, g):
        medium = hf_amd.Medium(sigma_t, ALBEDO, g, top_origin=TOP)
        fog = hf_amd.medium_lighting(shape, si, ray, rig, medium, spp=SPP, num_steps=STEPS, seed=3)    # [2, size * size]
        seen = surface * hf_amd.medium_attenuation(si, ray, rig, medium)
        return fog + seen.reshape(len(rig), -1, SPP).mean(2)

    with torch.no_grad():
        targets = render(*(torch.tensor(x, dtype=torch.float64) for x in TARGET))
    sigma_t, g = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in START)
    opt = torch.optim.Adam([sigma_t, g], lr=lr)
    hist = []
    for step in range(steps):
        opt.zero_grad()
        loss = 1e3 * ((render(sigma_t, g) - targets) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose:
            print("step %4d  loss %.6e  sigma_t %.4f  g %.4f" % (step, hist[-1], float(sigma_t.detach()), float(g.detach())))
    end = (float(sigma_t.detach()), float(g.detach()))
    if verbose:
        print("sigma_t, g: %.4f, %.4f (start %.4f, %.4f; target %.4f, %.4f)" % (end + START + TARGET))
    return hist, START, end, TARGET


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.02)
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr)

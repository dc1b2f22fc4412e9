#!/usr/bin/env python3
"""Photometric stereo for a normal map: recover a per-texel normal field, finer than the height grid and independent of
it, from images under a rig of four directional lights.

    python examples/inverse_normalmap.py [--steps 200 --size 64]

A known terrain carries an unknown normal map (the reference's `normalmap` over a `bitmap`: texels 0.5 (m + 1), m the
normal in the tangent space of the surface).  An orthographic camera looks down at the terrain and takes one image per
light.  Every step:
    si = shape.ray_intersect(ray)                                      fused traversal + surface interaction
    si = normal_map.perturb(si)                                        ONE fused HIP launch: hf_normalmap_eval
    images = hf_amd.directional_lighting(shape, si, ray, rig)          ONE fused HIP launch, the shadow rays traced inside
    loss = mean((images - targets)^2);  loss.backward()                hf_directional_lighting_adjoint, then
                                                                       hf_normalmap_eval_adjoint: the texels' gradient
The texels start from NormalMap.flat (every normal the surface's own) and torch's Adam runs on them.  The error is the
mean angle between the decoded map and the true one over the texels the view sees.  The visibility is held, as
everywhere: the rows decide on <sh_n, l> with the perturbed normal, the shadow rays leave along the geometric one."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
# (to_light, irradiance): examples/inverse_sun.py's rig
RIG = torch.tensor([[0.5, 0.2, 0.84, 3.0], [-0.7, 0.3, 0.45, 3.5], [0.1, -0.8, 0.4, 2.5], [0.0, 0.0, 1.0, 3.14]], dtype=torch.float64)


def true_map(T, device):
    """[3, T, T] texels of a smooth field of normals tilted by up to about 25 degrees"""
    c = (torch.arange(T, device=device, dtype=torch.float32) + 0.5) / T
    y, x = torch.meshgrid(c, c, indexing="ij")
    m = torch.stack([0.45 * torch.sin(2 * math.pi * (x + 0.3 * y)), 0.45 * torch.cos(2 * math.pi * (1.5 * y - 0.2 * x)),
                     torch.ones_like(x)])
    return hf_amd.NormalMap.encode(m / m.norm(dim=0, keepdim=True)).contiguous()


def seen_texels(si, T):
    """[T, T] bool: the texels whose cell a hit sample's uv falls into"""
    hit = si.is_valid()
    ix = (si.uv[0][hit] * T).floor().clamp(0, T - 1).long()
    iy = (si.uv[1][hit] * T).floor().clamp(0, T - 1).long()
    seen = torch.zeros((T, T), dtype=torch.bool, device=si.uv.device)
    seen[iy, ix] = True
    return seen


def angle_error(nm, target, seen):
    """mean angle (radians) between the decoded maps over the texels `seen`"""
    with torch.no_grad():
        cos = (nm.decode() * target.decode()).sum(0).clamp(-1.0, 1.0)
        return float(torch.acos(cos)[seen].mean())


def run(size=64, steps=200, heights=None, lr=0.02, device="cuda", verbose=True):
    """returns (the loss history, the angular error at the start, the angular error at the end).  `heights`: the known
    terrain as a [H, W] tensor in [0, 1] (None: workload.sine_heights(size, size)); the film is size x size pixels of SPP
    samples, the map min(32, size // 2) texels a side"""
    dev = torch.device(device)
    h = hf_amd.workload.sine_heights(size, size, device=dev) if heights is None else heights.to(dev)
    shape = hf_amd.Heightfield(heightfield=h, max_height=0.5)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=(0.6, 0.35, 2.0), target=(0.0, 0.0, 0.25),
                                      scale=(0.95, 0.95, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    T = max(4, min(32, size // 2))
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)      # the terrain is known: one trace serves every step
    target = hf_amd.NormalMap(true_map(T, dev), wrap="clamp")
    seen = seen_texels(si, T)

    def render(nm):
        return hf_amd.directional_lighting(shape, nm.perturb(si), ray, RIG, albedo=0.8, spp=SPP)   # [4, size * size]

    with torch.no_grad():
        targets = render(target)
    nm = hf_amd.NormalMap.flat(T, T, device=dev, wrap="clamp")
    nm.data.requires_grad_(True)
    opt = torch.optim.Adam([nm.data], lr=lr)
    err0 = angle_error(nm, target, seen)
    hist = []
    for step in range(steps):
        opt.zero_grad()
        loss = len(RIG) * ((render(nm) - targets) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e  mean angle %.5f rad" % (step, hist[-1], angle_error(nm, target, seen)))
    err = angle_error(nm, target, seen)
    if verbose:
        print("mean angle between the maps over the %d texels seen: %.5f rad (start %.5f)" % (int(seen.sum()), err, err0))
    return hist, err0, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.02)
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr)

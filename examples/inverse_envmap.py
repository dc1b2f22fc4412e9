#!/usr/bin/env python3
"""Lighting as the unknown: recover the texels of an environment map from one rendered view of a known terrain.

    terrain (hf_amd.workload.sine_heights) and an orthographic view are given;
    image = envmap_lighting on the samples that hit the terrain (hf_envmap_lighting: the shadow rays drawn by importance
            sampling of the CURRENT map and traced inside the kernel)  +  Envmap.eval on the rays that miss it
            (the emitter seen directly: the si.emitter(scene).eval(si) term of direct_reparam.py:141);
    the target is rendered under a sun-plus-gradient map; Adam (torch.optim) runs on the texels from a grey map.
The sampling distribution follows the texels (Envmap rebuilds its table when they change); a defensive fraction keeps
texels that are dark in the current estimate reachable.

    python examples/inverse_envmap.py [--grid 64 --film 64 --steps 100]
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402


def target_map(width, height, device):
    """[height, width] (no seam column): an overcast gradient, brighter towards the zenith and towards one side, plus a
    low sun of a few texels"""
    th = math.pi * torch.arange(height, device=device)[:, None] / (height - 1)
    ph = 2.0 * math.pi * (torch.arange(width, device=device)[None, :] + 0.5) / width
    m = 0.5 + 0.4 * torch.cos(th) + 0.2 * torch.sin(th) * torch.cos(ph)
    m = torch.where(torch.cos(th) > -0.05, m, torch.full_like(m, 0.05))          # the ground below the horizon is dim
    sun = 20.0 * torch.exp(-(((th - 0.3 * math.pi) / 0.25) ** 2 + ((ph - 0.6 * math.pi) / 0.35) ** 2))
    return (m + sun).to(torch.float32)


def render(shape, si, ray, env, spp, num_rays, seed):
    """[pixels]: the terrain under the map, the map itself beside the terrain (box film, mean of the pixel's samples)"""
    lit = hf_amd.envmap_lighting(shape, si, ray, env, albedo=0.8, spp=spp, num_rays=num_rays, seed=seed)
    miss = ~si.is_valid()
    background = env.eval(ray.d, active=miss)
    return lit + background.reshape(-1, spp).mean(1)


def run(grid=64, film=64, map_size=(17, 9), spp=4, steps=100, lr=0.05, num_rays=8, defensive=0.25, device="cuda",
        verbose=True):
    """returns the loss history; run.texel_error: (initial, final) mean |texel - target| over the upper hemisphere"""
    dev = torch.device(device)
    shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(grid, grid, device=dev), max_height=0.5)
    # a view from the side that frames the terrain and the sky behind it
    rays = hf_amd.workload.ortho_rays(film, film, spp, dev, seed=1, origin=(2.2, 0.6, 1.1), target=(0.0, 0.0, 0.45),
                                      scale=(1.3, 1.3, 1.0))
    ray = hf_amd.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    W0, H = map_size[0] - 1, map_size[1]
    truth = target_map(W0, H, dev)
    with torch.no_grad():
        target = render(shape, si, ray, hf_amd.Envmap(truth, defensive=defensive), spp, 32, seed=99)
    data = torch.full((H, W0), 0.5, device=dev, requires_grad=True)
    env = hf_amd.Envmap(data, defensive=defensive)
    opt = torch.optim.Adam([data], lr=lr)
    upper = slice(0, H // 2 + 1)
    err0 = float((data.detach() - truth)[upper].abs().mean())
    hist = []
    for it in range(steps):
        opt.zero_grad()
        loss = ((render(shape, si, ray, env, spp, num_rays, seed=it) - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            data.clamp_(min=0.0)                                                 # radiance is not negative
        hist.append(float(loss.detach()))
        if verbose:
            print(f"step {it:4d}  loss {hist[-1]:.6f}", flush=True)
    run.texel_error = (err0, float((data.detach() - truth)[upper].abs().mean()))
    if verbose:
        print(f"mean |texel - target| above the horizon: {run.texel_error[0]:.4f} -> {run.texel_error[1]:.4f}")
    return hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--film", type=int, default=64)
    ap.add_argument("--map", type=int, nargs=2, default=(17, 9), metavar=("W", "H"), help="texels, the seam column included")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.05)
    a = ap.parse_args()
    run(a.grid, a.film, tuple(a.map), a.spp, a.steps, a.lr)

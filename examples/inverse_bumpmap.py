#!/usr/bin/env python3
"""Photometric stereo for a bump map: recover the texels of a relief finer than the height grid from images of a known
coarse terrain under a rig of four directional lights.

    python examples/inverse_bumpmap.py [--steps 200 --size 64]

A known terrain on a COARSE grid (a quarter of the film's resolution) carries an unknown relief on a finer texture (the
reference's `bumpmap` over a `bitmap`: one float per texel, whose slopes tilt the shading normal).  Unlike a normal map the
unknown is a surface by construction: whatever is recovered is integrable.  An orthographic camera looks down at the
terrain and takes one image per light.  Every step:
    si = shape.ray_intersect(ray)                                      fused traversal + surface interaction (once: known)
    si = bump_map.perturb(si)                                          ONE fused HIP launch: hf_bumpmap_eval
    images = hf_amd.directional_lighting(shape, si, ray, rig)          ONE fused HIP launch, the shadow rays traced inside
    loss = mean((images - targets)^2);  loss.backward()                hf_directional_lighting_adjoint, then
                                                                       hf_bumpmap_eval_adjoint: the texels' gradient
The texels start from BumpMap.flat and torch's Adam runs on them.  The images see only the relief's slopes, so it is
recovered up to a constant: the error is the RMS difference of the two reliefs, each with its mean over the texels the
view sees taken off, over the RMS of the true one.  The visibility is held, as everywhere: the rows decide on <sh_n, l>
with the perturbed normal, the shadow rays leave along the geometric one."""
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
AMPLITUDE = 0.03


def true_relief(T, device):
    """[T, T] texels of a smooth relief of two crossing waves: slopes of up to about a third of |dp_du| = 2"""
    c = (torch.arange(T, device=device, dtype=torch.float32) + 0.5) / T
    y, x = torch.meshgrid(c, c, indexing="ij")
    return (AMPLITUDE * (torch.sin(2 * math.pi * (2 * x + 0.5 * y)) + 0.7 * torch.cos(2 * math.pi * (1.5 * y - x)))).contiguous()


def seen_texels(si, T):
    """[T, T] bool: the texels whose cell a hit sample's uv falls into"""
    hit = si.is_valid()
    ix = (si.uv[0][hit] * T).floor().clamp(0, T - 1).long()
    iy = (si.uv[1][hit] * T).floor().clamp(0, T - 1).long()
    seen = torch.zeros((T, T), dtype=torch.bool, device=si.uv.device)
    seen[iy, ix] = True
    return seen


def relief_error(bm, target, seen):
    """RMS difference of the reliefs over the texels `seen`, their means taken off, over the RMS of the true one"""
    with torch.no_grad():
        a, b = bm.data[seen], target.data[seen]
        a, b = a - a.mean(), b - b.mean()
        return float((a - b).square().mean().sqrt() / b.square().mean().sqrt())


def run(size=64, steps=200, heights=None, lr=0.002, device="cuda", verbose=True):
    """returns (the loss history, the relief's error at the start, its error at the end).  `heights`: the known terrain as
    a [H, W] tensor in [0, 1] (None: workload.sine_heights on a grid of size // 4 a side); the film is size x size pixels of
    SPP samples, the relief min(32, size // 2) texels a side"""
    dev = torch.device(device)
    G = max(4, size // 4)
    h = hf_amd.workload.sine_heights(G, G, device=dev) if heights is None else heights.to(dev)
    shape = hf_amd.Heightfield(heightfield=h, max_height=0.5)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=(0.6, 0.35, 2.0), target=(0.0, 0.0, 0.25),
                                      scale=(0.95, 0.95, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    T = max(4, min(32, size // 2))
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)      # the terrain is known: one trace serves every step
    target = hf_amd.BumpMap(true_relief(T, dev), wrap="clamp")
    seen = seen_texels(si, T)

    def render(bm):
        return hf_amd.directional_lighting(shape, bm.perturb(si), ray, RIG, albedo=0.8, spp=SPP)   # [4, size * size]

    with torch.no_grad():
        targets = render(target)
    bm = hf_amd.BumpMap.flat(T, T, device=dev, wrap="clamp")
    bm.data.requires_grad_(True)
    opt = torch.optim.Adam([bm.data], lr=lr)
    err0 = relief_error(bm, target, seen)
    hist = []
    for step in range(steps):
        opt.zero_grad()
        loss = len(RIG) * ((render(bm) - targets) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e  relief error %.5f" % (step, hist[-1], relief_error(bm, target, seen)))
    err = relief_error(bm, target, seen)
    if verbose:
        print("relative RMS error of the relief over the %d texels seen: %.5f (start %.5f)" % (int(seen.sum()), err, err0))
    return hist, err0, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.002)
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr)

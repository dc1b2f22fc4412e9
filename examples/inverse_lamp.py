"""Inverse lamp: recover the texels of a light panel from one view of a known terrain lit by it.

    python examples/inverse_lamp.py --steps 100 --size 64

An orthographic camera looks down on a known heightfield under a rectangular light panel (the reference's `area` emitter
on a `rectangle`) whose emission is a texture.  The terrain is traced once; every step is
    hf_amd.rect_lighting(shape, si, ray, lamp)        fused HIP kernel: draw points of the panel, trace the soft shadows,
                                                      look the texture up at the draws, reduce to the image
    loss = mean((image - target)^2);  loss.backward() hf_rect_lighting_adjoint -> the texels (float atomics)
    torch.optim.Adam on the texels
The image is linear in the texels, so this is a least-squares problem whose matrix the terrain's shadows shape: a texel
shows in the image through the samples that see it.  The draws are the same from step to step (seed), as in the
reference's detached emitter sampling; the visibility does not depend on the texels."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP, NUM_RAYS = 4, 16
ORIGIN, TARGET = (0.3, 0.2, 2.0), (0.0, 0.0, 0.25)
CENTER, EX, EY, RADIANCE = (0.1, -0.1, 1.2), (0.0, 0.4, 0.0), (0.6, 0.0, 0.1), 8.0   # ex x ey looks down
TW, TH = 16, 8


def panel(device):
    """the known emission of the panel: 0.6 + 0.3 sin(2 pi 1.5 x + 0.4) + 0.1 cos(2 pi y), x, y in [0, 1]"""
    y = (torch.arange(TH, device=device, dtype=torch.float32) + 0.5) / TH
    x = (torch.arange(TW, device=device, dtype=torch.float32) + 0.5) / TW
    yy, xx = torch.meshgrid(y, x, indexing="ij")
    return (0.6 + 0.3 * torch.sin(2.0 * math.pi * 1.5 * xx + 0.4) + 0.1 * torch.cos(2.0 * math.pi * yy)).contiguous()


def run(size=64, steps=100, lr=0.05, device="cuda", verbose=True):
    """returns (the loss history, the relative L2 error of the recovered texels)"""
    dev = torch.device(device)
    shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(size, size, device=dev), max_height=0.5)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=ORIGIN, target=TARGET, scale=(0.8, 0.8, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    with torch.no_grad():
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)

    def render(texels):
        lamp = hf_amd.RectLight(CENTER, EX, EY, RADIANCE, texture=texels)
        return hf_amd.rect_lighting(shape, si, ray, lamp, albedo=0.8, spp=SPP, num_rays=NUM_RAYS, seed=3)

    truth = panel(dev)
    with torch.no_grad():
        target = render(truth)
    texels = torch.full_like(truth, 0.5).requires_grad_(True)
    opt = torch.optim.Adam([texels], lr=lr)
    hist = []
    for step in range(steps):
        opt.zero_grad()
        loss = ((render(texels) - target) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e" % (step, hist[-1]))
    err = float((texels.detach() - truth).norm() / truth.norm())
    if verbose:
        print("relative L2 error of the texels: %.4f" % err)
    return hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.05)
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr)

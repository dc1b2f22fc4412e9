#!/usr/bin/env python3
"""Photometric stereo with cast shadows under distant lights: calibrate a rig of four directional lights on a known
relief, or recover the relief under the known rig.

    python examples/inverse_sun.py [--steps 150 --size 64]             the rig: 4 directions and 4 irradiances
    python examples/inverse_sun.py --heights [--steps 100 --size 64]   the heights

Four directional lights (the reference's `directional` emitter) are switched on in turn; an orthographic camera looks
down at 30 degrees off vertical and takes one image per light.  Every step:
    si = shape.ray_intersect(ray)                                      fused traversal + surface interaction
    images = hf_amd.directional_lighting(shape, si, ray, rig)          ONE fused HIP launch: the four shadow rays and the
                                                                       four films, the sample's record read once
    loss = mean((images - targets)^2);  loss.backward()                hf_directional_lighting_adjoint
In the default mode the terrain is known and torch's Adam runs on the [4, 4] table of (to_light, irradiance) through the
kernel's reduced gradients (4 numbers per light); the gradient of a to_light is orthogonal to it, so its length drifts
only with Adam's own normalisation and the error is measured as an angle.  With --heights the rig is known and hf_amd.Adam
runs on the heights (an update + a rebuild of the acceleration data per step), the gradient arriving through sh_n and
hf_adjoint.  Visibility and the masks are held, as everywhere: the silhouette part of a moving shadow is hf_reparam_*'s.
examples/inverse_heights.py --shadows is the same loop with the shadow rays traced by the caller, one launch per light."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
# (to_light, irradiance): one high light, two low ones that cast long shadows, the zenith
RIG = torch.tensor([[0.5, 0.2, 0.84, 3.0], [-0.7, 0.3, 0.45, 3.5], [0.1, -0.8, 0.4, 2.5], [0.0, 0.0, 1.0, 3.14]], dtype=torch.float64)
# where the calibration starts: every direction off by about 5 degrees, every irradiance by 15 to 25 per cent
START = RIG + torch.tensor([[0.06, -0.05, 0.0, -0.6], [0.05, 0.06, 0.04, 0.7], [-0.06, 0.03, 0.05, -0.5], [0.07, -0.04, 0.0, 0.6]],
                           dtype=torch.float64)
RIG_LR = (0.006, 0.05)      # Adam's step for the components of to_light and for the irradiances


def rig_error(table):
    """mean angle between each to_light and the true one (radians) + mean |E - E*| / E*"""
    l = table[:, :3] / table[:, :3].norm(dim=1, keepdim=True)
    t = RIG[:, :3] / RIG[:, :3].norm(dim=1, keepdim=True)
    angle = torch.acos((l * t).sum(1).clamp(-1.0, 1.0)).mean()
    return float(angle + ((table[:, 3] - RIG[:, 3]).abs() / RIG[:, 3]).mean())


def centred_error(h, target):
    """mean |h - h*| after removing the mean offset: shading under distant lights observes the surface's slope, not its
    absolute height (examples/inverse_heights.py)"""
    d = h - target
    return float((d - d.mean()).abs().mean())


def run(size=64, steps=100, lr=None, heights=False, device="cuda", verbose=True):
    """returns (the loss history, the parameter error at the start, the parameter error at the end): rig_error of the
    table, or with heights centred_error of the heights"""
    dev = torch.device(device)
    target_h = hf_amd.workload.sine_heights(size, size, device=dev)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=(0.6, 0.35, 2.0), target=(0.0, 0.0, 0.25),
                                      scale=(0.95, 0.95, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])

    def render(shape, table):
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
        return hf_amd.directional_lighting(shape, si, ray, table, albedo=0.8, spp=SPP)     # [4, size * size]: one launch

    with torch.no_grad():
        targets = render(hf_amd.Heightfield(heightfield=target_h, max_height=0.5), RIG)
    hist = []
    if heights:
        table = RIG
        shape = hf_amd.Heightfield(heightfield=(0.5 + 0.6 * (target_h - 0.5)).contiguous(), max_height=0.5)
        shape.heightfield.requires_grad_(True)
        opt = hf_amd.Adam(shape, lr=lr or 0.004)
        error = lambda: centred_error(shape.heightfield.detach(), target_h)
    else:
        shape = hf_amd.Heightfield(heightfield=target_h, max_height=0.5)
        v = START[:, :3].clone().requires_grad_(True)
        E = START[:, 3].clone().requires_grad_(True)
        opt = torch.optim.Adam([{"params": [v], "lr": (lr or 1.0) * RIG_LR[0]}, {"params": [E], "lr": (lr or 1.0) * RIG_LR[1]}])
        error = lambda: rig_error(torch.cat([v.detach(), E.detach()[:, None]], 1))
    err0 = error()
    for step in range(steps):
        opt.zero_grad()
        images = render(shape, table if heights else torch.cat([v, E[:, None]], 1))
        loss = len(RIG) * ((images - targets) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e  error %.5f" % (step, hist[-1], error()))
    err = error()
    if verbose:
        if heights:
            print("mean |height - target| (offset removed): %.5f (start %.5f)" % (err, err0))
        else:
            print("mean angle + mean relative irradiance error: %.5f (start %.5f)" % (err, err0))
            print("to_light, irradiance:", torch.cat([v.detach(), E.detach()[:, None]], 1).tolist())
    return hist, err0, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--heights", action="store_true")
    a = ap.parse_args()
    run(size=a.size, steps=a.steps or (100 if a.heights else 150), lr=a.lr, heights=a.heights)

#!/usr/bin/env python3
"""Gloss from highlights: recover the roughness of a glossy relief under a rig of directional lights, or the roughness and
the relief together, from one image per light.

    python examples/inverse_highlight.py [--steps 120 --size 64]             the roughness alpha
    python examples/inverse_highlight.py --heights [--steps 120 --size 64]   alpha and the heights

Eight directional lights (the rig of tests/directional_ref.py) are switched on in turn; an orthographic camera looks down
at the relief and takes one image per light: a diffuse term plus the GGX highlight of a dielectric coating (eta 1.5).
Every step:
    si = shape.ray_intersect(ray)                                        fused traversal + surface interaction
    diffuse, vis = hf_amd.directional_lighting(shape, si, ray, rig, return_visibility=True)
                                                                         ONE launch: the eight shadow walks, the films
    gloss = hf_amd.specular_lighting(si, ray, rig, vis, alpha)           ONE launch, nothing traced: the byte is read
    loss = mean((diffuse + gloss - targets)^2);  loss.backward()         hf_specular_lighting_adjoint (+ the diffuse row's)
torch's Adam runs on the scalar alpha (the kernel hands back a per-sample row, torch reduces it); it starts from a wrong
roughness, more than twice the true one.  With --heights hf_amd.Adam also runs on the heights, which start flattened (an
update + a rebuild of the acceleration data per step); their gradient arrives through sh_n of both rows and hf_adjoint.
The two optimisers are staged: alpha is held for the first ALPHA_HOLD steps.  While the relief is far off, its misplaced
highlights are best explained by blur, and a free alpha first GROWS (0.45 -> 0.63 in 30 steps) before it comes back.
A diffuse-only fit of such images is biased by the highlights; here they are part of the model.  Visibility and the masks
are held, as everywhere."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
ETA = 1.5
ALBEDO = 0.8
ALPHA = 0.2                 # the roughness to find
ALPHA_START = 0.45          # where the fit starts
ALPHA_LR = 0.01             # torch's Adam on alpha
FLATTEN = 0.6               # --heights: the relief starts as 0.5 + FLATTEN (h* - 0.5), as in examples/inverse_sun.py
HEIGHT_LR = 0.004           # --heights: hf_amd.Adam on the heights, as in examples/inverse_sun.py
ALPHA_HOLD = 20             # --heights: alpha is held for the first steps, while the relief moves the highlights into place
# (to_light, irradiance): tests/directional_ref.py's RIG
RIG = torch.tensor([[0, 0, 1, 3.0], [0.3, 0.2, 0.9, 2.5], [1, 0.1, 0.25, 1.5], [-0.2, -1, 0.2, 2.0], [-1, 0.3, 0.08, 4.0],
                    [0.7, -0.7, 0.35, 1.0], [0.3, 0.1, -0.6, 0.5], [2, 1, 1.5, 3.5]], dtype=torch.float64)


def centred_error(h, target):
    """mean |h - h*| after removing the mean offset: shading under distant lights observes the surface's slope, not its
    absolute height (examples/inverse_heights.py)"""
    d = h - target
    return float((d - d.mean()).abs().mean())


def run(size=64, steps=120, lr=None, heights=False, device="cuda", verbose=True):
    """returns (the loss history, |alpha - alpha*| at the start and at the end, the centred height error at the start and
    at the end -- both 0 without heights)"""
    dev = torch.device(device)
    target_h = hf_amd.workload.sine_heights(size, size, device=dev)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=(0.6, 0.35, 2.0), target=(0.0, 0.0, 0.25),
                                      scale=(0.95, 0.95, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])

    def render(shape, alpha):
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
        diffuse, vis = hf_amd.directional_lighting(shape, si, ray, RIG, albedo=ALBEDO, spp=SPP, return_visibility=True)
        return diffuse + hf_amd.specular_lighting(si, ray, RIG, vis, alpha, eta=ETA, spp=SPP)   # [8, size * size]

    with torch.no_grad():
        targets = render(hf_amd.Heightfield(heightfield=target_h, max_height=0.5), ALPHA)
    alpha = torch.tensor(ALPHA_START, requires_grad=True)
    opt_a = torch.optim.Adam([alpha], lr=(lr or 1.0) * ALPHA_LR)
    if heights:
        shape = hf_amd.Heightfield(heightfield=(0.5 + FLATTEN * (target_h - 0.5)).contiguous(), max_height=0.5)
        shape.heightfield.requires_grad_(True)
        opt_h = hf_amd.Adam(shape, lr=(lr or 1.0) * HEIGHT_LR)
        h_error = lambda: centred_error(shape.heightfield.detach(), target_h)
    else:
        shape = hf_amd.Heightfield(heightfield=target_h, max_height=0.5)
        opt_h, h_error = None, lambda: 0.0
    a_error = lambda: abs(float(alpha.detach()) - ALPHA)
    err0, herr0 = a_error(), h_error()
    hist = []
    for step in range(steps):
        opt_a.zero_grad()
        if opt_h:
            opt_h.zero_grad()
        images = render(shape, alpha)
        loss = len(RIG) * ((images - targets) ** 2).mean()
        loss.backward()
        if not (heights and step < ALPHA_HOLD):
            opt_a.step()
        if opt_h:
            opt_h.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e  alpha %.4f  height error %.5f" % (step, hist[-1], float(alpha.detach()), h_error()))
    err, herr = a_error(), h_error()
    if verbose:
        print("|alpha - %.2f|: %.4f (start %.4f)" % (ALPHA, err, err0))
        if heights:
            print("mean |height - target| (offset removed): %.5f (start %.5f)" % (herr, herr0))
    return hist, err0, err, herr0, herr


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--heights", action="store_true")
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr, heights=a.heights)

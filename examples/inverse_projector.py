#!/usr/bin/env python3
"""Fringe profilometry: recover a relief from three structured-light images, or calibrate the projector on a known one.

    python examples/inverse_projector.py [--steps 100 --size 64]          the heights
    python examples/inverse_projector.py --pose [--steps 150 --size 64]   the projector's origin, yaw and field of view

A projector (the reference's `projector` emitter) stands beside the terrain and throws three sinusoidal fringe patterns,
phase-shifted by a third of a period, onto it; a PerspectiveCamera looks down.  The pattern position a surface point
receives depends on its height, so the three images constrain the heights directly and not only the slopes.  Every step:
    si = shape.ray_intersect(ray)                               fused traversal + surface interaction
    image_k = hf_amd.projector_lighting(shape, si, ray, proj_k)   fused HIP kernel: frustum mapping, fringe lookup, the
                                                                shadow ray to the pinhole, the film
    loss = sum_k mean((image_k - target_k)^2);  loss.backward()   hf_projector_lighting_adjoint -> si.p, sh_n -> hf_adjoint
    hf_amd.Adam on the heights (an update + a rebuild of the acceleration data per step)
With --pose the terrain is known and torch's Adam runs on the projector's origin (x, y, z), its yaw about the world's z
axis and its field of view, through the kernel's reduced gradients of to_world (12 numbers) and fov.  Visibility and the
masks are held, as everywhere: the silhouette part of a moving shadow is hf_reparam_*'s."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
EYE, LOOK = (0.15, -0.2, 2.6), (0.0, 0.0, 0.25)
ORIGIN, AIM, FOV = (1.6, 0.3, 1.5), (0.0, 0.0, 0.2), 42.0       # the projector: from the side, 43 degrees above the horizon
TW, TH, PERIODS = 64, 64, 6.0                                   # (the frustum's aspect is TW / TH: a square one)
POSE_START = (0.05, -0.04, 0.04, math.radians(2.0), 1.5)        # offsets of origin x, y, z, the yaw and the fov (degrees)
POSE_LR = (0.004, 0.004, 0.004, 0.003, 0.1)


def fringes(device):
    """three [TH, TW] patterns 0.5 + 0.5 cos(2 pi PERIODS x + 2 pi k / 3): vertical fringes, constant along y"""
    x = (torch.arange(TW, device=device, dtype=torch.float32) + 0.5) / TW
    return [(0.5 + 0.5 * torch.cos(2.0 * math.pi * (PERIODS * x + k / 3.0)))[None, :].expand(TH, TW).contiguous() for k in range(3)]


def pose_matrix(q):
    """3x4 to_world of the projector moved by q = (dx, dy, dz, yaw, .): a rotation about the world's z axis through the
    base origin after the base look-at frame, differentiable in q"""
    base = torch.as_tensor(hf_amd.workload.look_at(ORIGIN, AIM, (0.0, 0.0, 1.0)), dtype=torch.float64)[:3]
    c, s = torch.cos(q[3]), torch.sin(q[3])
    z, one = torch.zeros_like(c), torch.ones_like(c)
    R = torch.stack([torch.stack([c, -s, z]), torch.stack([s, c, z]), torch.stack([z, z, one])])
    return torch.cat([R @ base[:, :3], (base[:, 3] + torch.stack([q[0], q[1], q[2]]))[:, None]], dim=1)


def run(size=64, steps=100, lr=None, pose=False, device="cuda", verbose=True):
    """returns (the loss history, the final error: mean |height - target| in units of max_height, or with pose the largest
    |parameter - target| relative to the start's)"""
    dev = torch.device(device)
    target_h = hf_amd.workload.sine_heights(size, size, device=dev)
    cam = hf_amd.PerspectiveCamera.look_at(EYE, LOOK, (0.0, 1.0, 0.0), 30.0, film=(size, size))
    ray, _, _ = cam.sample_rays(SPP, seed=1, device=dev)
    patterns = fringes(dev)

    def render(shape, to_world, fov):
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
        return [hf_amd.projector_lighting(shape, si, ray, hf_amd.Projector(to_world, fov, tex, scale=4.0, wrap="clamp"),
                                          albedo=0.8, spp=SPP) for tex in patterns]

    zero = torch.zeros(5, dtype=torch.float64)
    with torch.no_grad():
        targets = render(hf_amd.Heightfield(heightfield=target_h, max_height=0.5), pose_matrix(zero), FOV)
    hist = []
    if pose:
        shape = hf_amd.Heightfield(heightfield=target_h, max_height=0.5)
        qs = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in POSE_START]
        opt = torch.optim.Adam([{"params": [q], "lr": (lr or 1.0) * r} for q, r in zip(qs, POSE_LR)])
    else:
        shape = hf_amd.Heightfield(heightfield=(0.5 + 0.6 * (target_h - 0.5)).contiguous(), max_height=0.5)
        shape.heightfield.requires_grad_(True)
        opt = hf_amd.Adam(shape, lr=lr or 0.004)
    for step in range(steps):
        opt.zero_grad()
        images = render(shape, pose_matrix(qs), FOV + qs[4]) if pose else render(shape, pose_matrix(zero), FOV)
        loss = sum(((img - tgt) ** 2).mean() for img, tgt in zip(images, targets))
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e" % (step, hist[-1]))
    if pose:
        err = max(abs(float(q.detach())) / abs(s) for q, s in zip(qs, POSE_START))
        if verbose:
            print("offsets left (origin x, y, z, yaw, fov):", ["%+.5f" % float(q.detach()) for q in qs], "start", POSE_START)
    else:
        err = float((shape.heightfield.detach() - target_h).abs().mean())
        if verbose:
            print("mean |height - target|: %.5f (start %.5f)" % (err, float((0.4 * (target_h - 0.5)).abs().mean())))
    return hist, err


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--pose", action="store_true")
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr, pose=a.pose)

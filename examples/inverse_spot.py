#!/usr/bin/env python3
"""Near-light photometric stereo: recover a relief from six images under a ring of spot lights, or calibrate one lamp on a
known relief.

    python examples/inverse_spot.py [--steps 100 --size 64]          the heights
    python examples/inverse_spot.py --pose [--steps 150 --size 64]   one lamp's origin, yaw and both angles

Six spot lights (the reference's `spot` emitter) stand on a ring above the terrain and are switched on in turn; a
PerspectiveCamera looks down and takes one image per lamp.  Every step:
    si = shape.ray_intersect(ray)                               fused traversal + surface interaction
    images = hf_amd.spot_lighting(shape, si, ray, lamps)        ONE fused HIP launch: the six cone mappings, the six shadow
                                                                rays and the six films, the sample's record read once
    loss = mean((images - targets)^2);  loss.backward()         hf_spot_lighting_adjoint -> si.p, sh_n -> hf_adjoint
    hf_amd.Adam on the heights (an update + a rebuild of the acceleration data per step)
With --pose the terrain is known and torch's Adam runs on lamp 0's origin (x, y, z), its yaw about the world's z axis, its
cutoff angle and its beam width, through the kernel's reduced gradients of to_world (12 numbers) and the two angles.  The
falloff ramps linearly to 0 at the cutoff, so the image is continuous in all of them but at shadow edges.  Visibility and
the masks are held, as everywhere: the silhouette part of a moving shadow is hf_reparam_*'s."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
K = 6
EYE, LOOK = (0.15, -0.2, 2.6), (0.0, 0.0, 0.25)
RADIUS, HEIGHT, AIM = 1.5, 1.3, (0.0, 0.0, 0.2)                 # the ring of lamps
CUTOFF, BEAM, INTENSITY = 40.0, 25.0, 6.0
POSE_START = (0.06, -0.05, 0.05, math.radians(2.5), 2.0, -2.0)  # offsets of lamp 0's origin x, y, z, yaw, cutoff and beam (degrees)
POSE_LR = (0.004, 0.004, 0.004, 0.003, 0.1, 0.1)


def lamp_origin(k):
    a = 2.0 * math.pi * (k + 0.25) / K
    return (RADIUS * math.cos(a), RADIUS * math.sin(a), HEIGHT)


def pose_matrix(k, q=None):
    """3x4 to_world of lamp k; q = (dx, dy, dz, yaw, ...) moves it: a rotation about the world's z axis through the base
    origin after the base look-at frame, differentiable in q"""
    base = torch.as_tensor(hf_amd.workload.look_at(lamp_origin(k), AIM, (0.0, 0.0, 1.0)), dtype=torch.float64)[:3]
    if q is None:
        return base
    c, s = torch.cos(q[3]), torch.sin(q[3])
    z, one = torch.zeros_like(c), torch.ones_like(c)
    R = torch.stack([torch.stack([c, -s, z]), torch.stack([s, c, z]), torch.stack([z, z, one])])
    return torch.cat([R @ base[:, :3], (base[:, 3] + torch.stack([q[0], q[1], q[2]]))[:, None]], dim=1)


def lamps(q=None):
    """the rig; q: lamp 0's offsets (None: the true rig)"""
    first = hf_amd.SpotLight(pose_matrix(0, q), INTENSITY, CUTOFF + (q[4] if q is not None else 0.0),
                             BEAM + (q[5] if q is not None else 0.0))
    return [first] + [hf_amd.SpotLight(pose_matrix(k), INTENSITY, CUTOFF, BEAM) for k in range(1, K)]


def run(size=64, steps=100, lr=None, pose=False, device="cuda", verbose=True):
    """returns (the loss history, the final error: mean |height - target| in units of max_height, or with pose the largest
    |parameter - target| relative to the start's)"""
    dev = torch.device(device)
    target_h = hf_amd.workload.sine_heights(size, size, device=dev)
    cam = hf_amd.PerspectiveCamera.look_at(EYE, LOOK, (0.0, 1.0, 0.0), 30.0, film=(size, size))
    ray, _, _ = cam.sample_rays(SPP, seed=1, device=dev)

    def render(shape, rig):
        si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
        return hf_amd.spot_lighting(shape, si, ray, rig, albedo=0.8, spp=SPP)       # [K, size * size]: one launch

    with torch.no_grad():
        targets = render(hf_amd.Heightfield(heightfield=target_h, max_height=0.5), lamps())
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
        images = render(shape, lamps(qs if pose else None))
        loss = K * ((images - targets) ** 2).mean()
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
        if verbose and (step % 10 == 0 or step == steps - 1):
            print("step %4d  loss %.6e" % (step, hist[-1]))
    if pose:
        err = max(abs(float(q.detach())) / abs(s) for q, s in zip(qs, POSE_START))
        if verbose:
            print("offsets left (origin x, y, z, yaw, cutoff, beam):", ["%+.5f" % float(q.detach()) for q in qs], "start", POSE_START)
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

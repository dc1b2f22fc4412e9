"""Inverse refraction: recover the relief of a refracting surface from one view of a known pattern on the plane below it
(shape from refractive distortion).

    python examples/inverse_refraction.py --steps 100 --size 64 [--large-steps LAMBDA]

An orthographic camera looks down on a smooth-shaded heightfield (face_normals = False: the shading normal is continuous
in the heights) that is the surface of a slab of index 1.33 over a plane carrying a known smooth pattern, a sum of sines.
A tilt of the normal moves the point of the pattern a sample sees, so the image is a sensitive function of the slopes.
Every step is
    shape.ray_intersect(camera rays)                                  the coherent primary trace
    hf_amd.refraction_lighting(shape, si, ray, receiver, bitmap)      fused HIP kernel: refract, walk to the plane, look up
    loss = mean((image - target)^2);  loss.backward()                 hf_refract_lighting_adjoint -> hf_adjoint -> heights
    hf_amd.Adam.step()                                                Adam on the heights + rebuild of the acceleration data
The target image comes from a known relief (a sine bump); the start is a flat field.  The masks, the visibility and the
cell of the lookup are piecewise constant: the gradient is that of the samples that keep seeing the plane.
--large-steps LAMBDA optimises the latent (I + LAMBDA L) h instead (hf_amd.LargeSteps), as examples/inverse_heights.py."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP = 4
ORIGIN, TARGET = (0.3, 0.2, 2.0), (0.0, 0.0, 0.25)
ETA, SIGMA_T, PLANE_Z, TEXELS = 1.33, 0.2, -0.5, 64


def relief(size, device):
    """the known relief: a sine bump on heights of 0.5, amplitude 0.06"""
    x = torch.linspace(-1.0, 1.0, size, device=device)
    yy, xx = torch.meshgrid(x, x, indexing="ij")
    return (0.5 + 0.06 * torch.cos(1.5 * math.pi * xx) * torch.cos(1.5 * math.pi * yy)).contiguous()


def pattern(device, res=TEXELS):
    """the known pattern on the plane: 0.6 + 0.2 sin(3 pi x) + 0.2 sin(3 pi y + 1) + 0.1 sin(2 pi (x + y)), x, y in [-1, 1]"""
    c = (torch.arange(res, device=device, dtype=torch.float32) + 0.5) / res * 2.0 - 1.0
    yy, xx = torch.meshgrid(c, c, indexing="ij")
    data = 0.6 + 0.2 * torch.sin(3.0 * math.pi * xx) + 0.2 * torch.sin(3.0 * math.pi * yy + 1.0) + \
        0.1 * torch.sin(2.0 * math.pi * (xx + yy))
    return hf_amd.Bitmap(data.contiguous(), wrap="clamp")


def render(shape, ray, receiver, bitmap):
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    return hf_amd.refraction_lighting(shape, si, ray, receiver, bitmap, eta=ETA, sigma_t=SIGMA_T, spp=SPP)


def run(size=64, steps=100, lr=0.001, large_steps=0.0, device="cuda", verbose=True):
    """returns the loss history"""
    dev = torch.device(device)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=ORIGIN, target=TARGET, scale=(0.8, 0.8, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    receiver = hf_amd.Receiver.plane_z(PLANE_Z, (-1.0, 1.0), (-1.0, 1.0), TEXELS, TEXELS)
    bitmap = pattern(dev)
    with torch.no_grad():
        target = render(hf_amd.Heightfield(heightfield=relief(size, dev), max_height=0.5, face_normals=False), ray, receiver,
                        bitmap)
    shape = hf_amd.Heightfield(heightfield=torch.full((size, size), 0.5, device=dev), max_height=0.5, face_normals=False)
    shape.heightfield.requires_grad_(True)
    opt = hf_amd.Adam(shape, lr=lr)
    if large_steps:
        ls = hf_amd.LargeSteps(size, size, lambda_=large_steps)
        latent = ls.to_differential(shape.heightfield.detach()).requires_grad_(True)
        adam_m, adam_v = torch.zeros_like(latent), torch.zeros_like(latent)
        b1, b2, eps = 0.9, 0.999, 1e-8

        def set_heights(guess):
            v = ls.from_differential(latent, guess=guess)
            shape.heightfield = v.detach().requires_grad_(True)
            shape.parameters_changed(["heightfield"])
            return v
        heights_of_latent = set_heights(shape.heightfield.detach())
    hist = []
    for it in range(steps):
        opt.zero_grad()
        loss = ((render(shape, ray, receiver, bitmap) - target) ** 2).mean()
        loss.backward()
        if large_steps:
            latent.grad = None
            heights_of_latent.backward(shape.heightfield.grad)
            with torch.no_grad():
                g = latent.grad
                adam_m.mul_(b1).add_(g, alpha=1 - b1)
                adam_v.mul_(b2).addcmul_(g, g, value=1 - b2)
                lr_t = lr * math.sqrt(1 - b2 ** (it + 1)) / (1 - b1 ** (it + 1))
                latent.sub_(lr_t * adam_m / (adam_v.max().sqrt() + eps))
            heights_of_latent = set_heights(shape.heightfield.detach())
        else:
            opt.step()
        hist.append(float(loss.detach()))
        if verbose and (it == 0 or it == steps - 1 or it % 10 == 0):
            print(f"step {it:4d}  loss {hist[-1]:.6e}", flush=True)
    if verbose:
        print(f"loss at start {hist[0]:.6e}, at end {hist[-1]:.6e}")
    return hist


def main(argv=None):
    """parses the command line, runs the optimisation and returns the loss history"""
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--large-steps", type=float, default=0.0, metavar="LAMBDA",
                    help="optimise the latent (I + LAMBDA L) h with uniform Adam (0: off; hf_amd.LargeSteps)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    return run(size=a.size, steps=a.steps, lr=a.lr, large_steps=a.large_steps, verbose=not a.quiet)


if __name__ == "__main__":
    main()

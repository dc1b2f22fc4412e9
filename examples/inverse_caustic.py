"""Inverse caustic: recover the relief of a refracting surface from the light pattern it throws on a plane below it.

    python examples/inverse_caustic.py --steps 100 --size 64 [--large-steps LAMBDA]

A collimated light shines straight down on a smooth-shaded heightfield (face_normals = False: the shading normal is
continuous in the heights), is refracted into the denser medium below (eta 1.33) and lands on a receiver plane under the
terrain.  Every step is
    shape.ray_intersect(light samples)                      the coherent primary trace brings the light to the surface
    hf_amd.caustic_lighting(shape, si, ray, receiver)       fused HIP kernel: refract, walk to the receiver, land
    hf_amd.caustic_film(pos, value, size, size)             the light tracer's film: accumulated flux per pixel
    loss = mean((film - target)^2);  loss.backward()        film adjoint -> hf_caustic_adjoint -> hf_adjoint -> heights
    hf_amd.Adam.step()                                      Adam on the heights + rebuild of the acceleration data
The target film comes from a known relief (a sum of two sines); the start is a flat field.  The masks and the occlusion
are piecewise constant: the gradient is that of the samples that keep landing, which is what a caustic is made of.
--large-steps LAMBDA optimises the latent (I + LAMBDA L) h instead (hf_amd.LargeSteps), as examples/inverse_heights.py."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

ETA, Z_RECEIVER, SPP_AXIS = 1.33, -1.0, 2


def relief(size, device):
    """the known relief: heights in [0.35, 0.65], two sines of different period"""
    x = torch.linspace(-1.0, 1.0, size, device=device)
    yy, xx = torch.meshgrid(x, x, indexing="ij")
    return (0.5 + 0.1 * torch.sin(2.5 * math.pi * xx) * torch.cos(1.5 * math.pi * yy) + 0.05 * torch.cos(3.0 * math.pi * yy)).contiguous()


def light(size, device):
    """SPP_AXIS x SPP_AXIS collimated samples per film pixel over the inner 80 % of the field, straight down"""
    k = size * SPP_AXIS
    x = ((torch.arange(k, device=device, dtype=torch.float32) + 0.5) / k * 2.0 - 1.0) * 0.8
    yy, xx = torch.meshgrid(x, x, indexing="ij")
    o = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.full((k * k,), 2.0, device=device)]).contiguous()
    d = torch.zeros_like(o); d[2] = -1.0
    return hf_amd.Ray3f(o, d)


def render(shape, ray, receiver, size):
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    pos, value = hf_amd.caustic_lighting(shape, si, ray, receiver, eta=ETA, power=1.0 / (SPP_AXIS * SPP_AXIS))
    return hf_amd.caustic_film(pos, value, size, size)


def run(size=64, steps=100, lr=0.002, large_steps=0.0, device="cuda", verbose=True):
    """returns the loss history"""
    dev = torch.device(device)
    ray = light(size, dev)
    receiver = hf_amd.Receiver.plane_z(Z_RECEIVER, (-1.0, 1.0), (-1.0, 1.0), size, size)
    with torch.no_grad():
        target = render(hf_amd.Heightfield(heightfield=relief(size, dev), max_height=0.5, face_normals=False), ray, receiver, size)
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
        loss = ((render(shape, ray, receiver, size) - target) ** 2).mean()
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.002)
    ap.add_argument("--large-steps", type=float, default=0.0, metavar="LAMBDA",
                    help="optimise the latent (I + LAMBDA L) h with uniform Adam (0: off; hf_amd.LargeSteps)")
    a = ap.parse_args()
    run(size=a.size, steps=a.steps, lr=a.lr, large_steps=a.large_steps)

"""Inverse roughness: recover the GGX roughness of a glossy relief from one image of its reflection of a known
environment map; with --heights the roughness and the relief jointly.

    python examples/inverse_roughness.py --steps 100 --size 64 [--heights] [--large-steps LAMBDA]

An orthographic camera looks down on a smooth-shaded heightfield (face_normals = False) whose surface reflects the
environment through a GGX lobe of roughness alpha (F = 1: eta = 0).  Every step is
    shape.ray_intersect(camera rays)                           the coherent primary trace
    hf_amd.glossy_lighting(shape, si, ray, envmap, alpha)      fused HIP kernel: draw the microfacet normals, walk the
                                                               mirror rays, look the map up
    loss = mean((image - target)^2);  loss.backward()          hf_glossy_lighting_adjoint (-> hf_adjoint -> heights)
    Adam on alpha (and, with --heights, hf_amd.Adam on the heights + rebuild of the acceleration data)
The target image comes from a known relief (a sine bump) and alpha_true = 0.25 with the same seed, so the loss is 0 at
the answer; the start is alpha = 0.5 (and, with --heights, a flat field).  The drawn directions are held in the
derivative (detached sampling): the gradient is that of the estimator's expectation, not of this seed's realisation.
--large-steps LAMBDA optimises the latent (I + LAMBDA L) h instead (hf_amd.LargeSteps), as examples/inverse_heights.py.
Prints the loss and alpha per step."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hf_amd  # noqa: E402

SPP, NUM_RAYS, SEED = 4, 4, 1
ALPHA_TRUE, ALPHA_START = 0.25, 0.5
ORIGIN, TARGET = (0.3, 0.2, 2.0), (0.0, 0.0, 0.25)


def relief(size, device):
    """the known relief: a sine bump on heights of 0.5, amplitude 0.06"""
    x = torch.linspace(-1.0, 1.0, size, device=device)
    yy, xx = torch.meshgrid(x, x, indexing="ij")
    return (0.5 + 0.06 * torch.cos(1.5 * math.pi * xx) * torch.cos(1.5 * math.pi * yy)).contiguous()


def environment(device, W0=32, H=17):
    """a map with a bright lobe near the zenith on a dim smooth ground: its blur tells the roughness"""
    th = math.pi * torch.arange(H, device=device, dtype=torch.float32)[:, None] / (H - 1)
    ph = 2.0 * math.pi * (torch.arange(W0, device=device, dtype=torch.float32)[None, :] + 0.5) / W0
    data = 0.2 + 0.1 * torch.cos(ph) * torch.sin(th) + 2.0 * torch.exp(-(th / 0.5) ** 2) + 0.0 * ph
    return hf_amd.Envmap(data.contiguous())


def render(shape, ray, envmap, alpha):
    si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
    return hf_amd.glossy_lighting(shape, si, ray, envmap, alpha, eta=0.0, spp=SPP, num_rays=NUM_RAYS, seed=SEED)


def run(size=64, steps=100, lr=0.01, lr_heights=0.001, heights=False, large_steps=0.0, device="cuda", verbose=True):
    """returns (the loss history, the alpha history, alpha_true)"""
    dev = torch.device(device)
    rays = hf_amd.workload.ortho_rays(size, size, SPP, dev, seed=1, origin=ORIGIN, target=TARGET, scale=(0.8, 0.8, 1.0))
    ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
    envmap = environment(dev)
    known = hf_amd.Heightfield(heightfield=relief(size, dev), max_height=0.5, face_normals=False)
    with torch.no_grad():
        target = render(known, ray, envmap, ALPHA_TRUE)
    alpha = torch.tensor(ALPHA_START, device=dev, requires_grad=True)
    opt_alpha = torch.optim.Adam([alpha], lr=lr)
    shape = known
    if heights:
        shape = hf_amd.Heightfield(heightfield=torch.full((size, size), 0.5, device=dev), max_height=0.5, face_normals=False)
        shape.heightfield.requires_grad_(True)
        opt = hf_amd.Adam(shape, lr=lr_heights)
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
    hist, alphas = [], []
    for it in range(steps):
        opt_alpha.zero_grad()
        if heights:
            opt.zero_grad()
        loss = ((render(shape, ray, envmap, alpha) - target) ** 2).mean()
        loss.backward()
        hist.append(float(loss.detach())); alphas.append(float(alpha.detach()))
        if verbose and (it == 0 or it == steps - 1 or it % 10 == 0):
            print(f"step {it:4d}  loss {hist[-1]:.6e}  alpha {alphas[-1]:.4f}", flush=True)
        opt_alpha.step()
        with torch.no_grad():
            alpha.clamp_(1e-3, 1.0)
        if heights and large_steps:
            latent.grad = None
            heights_of_latent.backward(shape.heightfield.grad)
            with torch.no_grad():
                g = latent.grad
                adam_m.mul_(b1).add_(g, alpha=1 - b1)
                adam_v.mul_(b2).addcmul_(g, g, value=1 - b2)
                lr_t = lr_heights * math.sqrt(1 - b2 ** (it + 1)) / (1 - b1 ** (it + 1))
                latent.sub_(lr_t * adam_m / (adam_v.max().sqrt() + eps))
            heights_of_latent = set_heights(shape.heightfield.detach())
        elif heights:
            opt.step()
    alphas.append(float(alpha.detach()))
    if verbose:
        print(f"loss at start {hist[0]:.6e}, at end {hist[-1]:.6e}; alpha {alphas[0]:.4f} -> {alphas[-1]:.4f} (true {ALPHA_TRUE})")
    return hist, alphas, ALPHA_TRUE


def main(argv=None):
    """parses the command line, runs the optimisation and returns (loss history, alpha history, alpha_true)"""
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.01, help="Adam step of alpha")
    ap.add_argument("--lr-heights", type=float, default=0.001)
    ap.add_argument("--heights", action="store_true", help="recover the relief too, from a flat field")
    ap.add_argument("--large-steps", type=float, default=0.0, metavar="LAMBDA",
                    help="with --heights: optimise the latent (I + LAMBDA L) h with uniform Adam (0: off; hf_amd.LargeSteps)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    return run(size=a.size, steps=a.steps, lr=a.lr, lr_heights=a.lr_heights, heights=a.heights, large_steps=a.large_steps,
               verbose=not a.quiet)


if __name__ == "__main__":
    main()

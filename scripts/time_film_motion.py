#!/usr/bin/env python3
"""Time the film of moving, weighted samples: forward plus backward to the values, the positions and the weights (HIP
events, warm-up, median of the timed runs), for the library's film (hf_amd.film_gaussian(..., weight=), --path native)
or the torch splat() of examples/inverse_pose.py (--path splat), on the same seeded inputs: the samples of a film x film
image at spp samples per pixel, moved by a fraction of a pixel, weights near 1.  The same script times any checkout:
--root names the repository whose hf_amd and examples are imported (default: this one), --label goes into the record.
usage: python scripts/time_film_motion.py [--root DIR --label NAME --path native splat --size 64x4 512x16 --warmup 2
       --iters 10 --out FILE]   (appends one JSON line per path and size)"""
import argparse, json, os, statistics, sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this commit")
ap.add_argument("--path", nargs="*", default=["native", "splat"], choices=["native", "splat"])
ap.add_argument("--size", nargs="*", default=["64x4", "512x16"], help="FILMxSPP")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
root = os.path.abspath(a.root)
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "examples"))
import torch
import hf_amd
import inverse_pose as ip

dev = torch.device("cuda", 0)
for size in a.size:
    film, spp = (int(v) for v in size.split("x"))
    gen = torch.Generator(device=dev).manual_seed(film * 131 + spp)
    base = hf_amd.workload.film_positions(film, film, spp, dev)
    n = base.shape[1]
    pos = (base + 0.3 * torch.randn((2, n), device=dev, generator=gen)).requires_grad_(True)
    vals = torch.rand(n, device=dev, generator=gen).requires_grad_(True)
    det = (1.0 + 0.05 * torch.randn(n, device=dev, generator=gen)).requires_grad_(True)
    g = torch.randn(film * film, device=dev, generator=gen)
    for path in a.path:
        def step():
            if path == "native":
                img = hf_amd.film_gaussian((vals * det)[None], pos, film, film, weight=det)[0]
            else:
                img = ip.splat(vals * det, det, pos, film)
            return torch.autograd.grad(img, (vals, pos, det), g)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for e0, e1 in ev:
            e0.record(); grads = step(); e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        rec = dict(commit=a.label, path=path, kind="film forward + backward(values, pos, weight)", film=film, spp=spp,
                   samples=n, ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                   runs=a.iters, grad_pos_norm=round(float(grads[1].norm()), 6), grad_values_norm=round(float(grads[0].norm()), 6))
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

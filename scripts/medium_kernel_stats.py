#!/usr/bin/env python3
"""The fused medium launch on the scene of tests/test_gpu_medium.py, for a profiler to look at: both wavefronts (32768
samples), the two lights, K = 4 points, each of the three media `--iters` times, image + value + visibility words.  Run
it under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/medium_kernel_stats.py`; the line of
hf_medium_kernel in DIR's kernel_stats file is what profiles/medium/kernel_trace_stats.txt records.  No timing is taken
here and no claim follows from it.
usage: python scripts/medium_kernel_stats.py [--iters 10]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import hf_amd  # noqa: E402
import medium_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
shape = hf_amd.Heightfield(heightfield=hf_amd.workload.sine_heights(96, 96, device="cuda"), max_height=0.5)
rays = torch.cat([hf_amd.workload.ortho_rays(*R.FILM, "cuda", seed=1, origin=R.ORIGIN, target=R.TARGET, scale=(0.9, 0.9, 1.0)),
                  R.wide_rays(hf_amd.workload.ortho_rays, "cuda")], 1).contiguous()
ray = hf_amd.Ray3f(rays[0:3], rays[3:6], rays[6])
si = shape.ray_intersect(ray, hf_amd.RayFlags.All)
rig = [hf_amd.DirectionalLight(v, E) for v, E in R.RIG]
for name, spec in R.MEDIA.items():
    medium = hf_amd.Medium(**spec)
    for _ in range(a.iters):
        image, value, bits = hf_amd.medium_lighting(shape, si, ray, rig, medium, spp=R.FILM[2], num_steps=R.K, seed=R.SEED,
                                                    return_value=True, return_visibility=True)
    torch.cuda.synchronize()
    print(name, "mean image", float(image.mean()), "visible share", float((bits != 0).float().mean()))

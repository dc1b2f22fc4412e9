#!/usr/bin/env python3
"""Where the tolerances of the derivative and projection tests of tests/test_gpu_thinlens.py come from (CPU only, no
device).  The scenes of that test -- film 13 x 7, the crop window (3, 2, 5, 4) and none, spp 1, 3, 4, the lenses
aperture_radius in {0, 0.05, 0.3} x focus_distance in {0.5, 2} with near_clip 1e-2 under the look_at pose of
tests/sensor_ref.py, the tangent directions() and the cotangents() of tests/thinlens_ref.py; for the way back the points of
project_points() under both crop windows -- are run through tests/thinlens_ref.py in float32 numpy against float64: the
restatement goes through the five matrices and numpy.linalg.inv, so in float32 it is the coarser of the two (the kernels
form everything in double and round once).  Per scene the errors as thinlens_ref.ray_derivative_errors / project_errors
measure them; last, the maxima.  The GPU is allowed four times the maxima (the F32 dict of the test).
usage: python scripts/thinlens_f32_error.py [--out profiles/thinlens/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import thinlens_ref as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
out, worst = {}, {}
for radius, focus in T.LENSES:
    for crop in (T.CROP, None):
        for spp in T.SPPS:
            s = T.scene(crop, radius, focus)
            ids, pos, D = T.wavefront(s, spp)
            go, gd = T.cotangents(len(ids))
            _, _, _, do, dd = T.rays(s, pos, D, np.float32, *T.directions())
            e = T.ray_derivative_errors(s, spp, (do, dd), T.rays_adjoint(s, pos, D, go, gd, np.float32))
            out[f"r={radius} f={focus} crop={crop} spp={spp}"] = e
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
for radius, focus in T.LENSES:
    for crop in (T.CROP, None):
        s = T.scene(crop, radius, focus, far=T.PROJECT_FAR)
        p, active, D, ref = T.project_case(s)
        _, _, _, got = T.project_case(s, np.float32)
        e = T.project_errors(s, p, active, got, ref)
        edge, depth = T.mask_margins(s, p, D)
        e["lanes"] = {"n": int(len(active)), "inside_z": int(ref.inside.sum()), "valid": int(ref.valid.sum()),
                      "s_crop_margin": edge, "depth_margin": depth,
                      "masks_equal_in_float32": bool((got.inside == ref.inside).all() and (got.valid == ref.valid).all())}
        out[f"project r={radius} f={focus} crop={crop}"] = e
        for k, v in e.items():
            if k != "lanes":
                worst[k] = max(worst.get(k, 0.0), v)
out["max"] = worst
text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")

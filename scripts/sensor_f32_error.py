#!/usr/bin/env python3
"""Where the tolerances of the derivative and projection tests of tests/test_gpu_sensor.py come from (CPU only, no
device).  The scenes of that test -- film 13 x 7, the crop window (3, 2, 5, 4) and none, spp 1, 3, 4, both sensor types
under the look_at pose of tests/sensor_ref.py, the tangent directions() and the cotangents() of that module; for the way
back the points of project_points() under both crop windows -- are run through tests/sensor_ref.py in float32 numpy
against float64: the restatement goes through the five matrices and numpy.linalg.inv, so in float32 it is the coarser of
the two (the kernels form everything in double and round once).  Per scene the errors as sensor_ref.ray_derivative_errors
/ project_errors measure them; last, the maxima.  The GPU is allowed four times the maxima (the F32 dict of the test).
usage: python scripts/sensor_f32_error.py [--out profiles/sensor/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import sensor_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
out, worst = {}, {}
for type_, tname in ((R.PERSPECTIVE, "perspective"), (R.ORTHOGRAPHIC, "orthographic")):
    for crop in (R.CROP, None):
        for spp in R.SPPS:
            s = R.scene(type_, crop)
            ids, pos = R.wavefront(s, spp)
            dtw, dfov = R.directions()
            go, gd = R.cotangents(len(ids))
            _, _, _, do, dd = R.rays(s, pos, np.float32, dtw, dfov)
            e = R.ray_derivative_errors(s, spp, (do, dd), R.rays_adjoint(s, pos, go, gd, np.float32))
            out[f"{tname} crop={crop} spp={spp}"] = e
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
for crop in (R.CROP, None):
    s = R.scene(R.PERSPECTIVE, crop, near=R.PROJECT_CLIP[0], far=R.PROJECT_CLIP[1])
    p, active, ref = R.project_case(s)
    _, _, got = R.project_case(s, np.float32)
    e = R.project_errors(s, p, active, got, ref)
    e["lanes"] = {"n": int(len(active)), "inside_z": int(ref.inside.sum()), "valid": int(ref.valid.sum()),
                  "masks_equal_in_float32": bool((got.inside == ref.inside).all() and (got.valid == ref.valid).all())}
    out[f"project crop={crop}"] = e
    for k, v in e.items():
        if k != "lanes":
            worst[k] = max(worst.get(k, 0.0), v)
out["max"] = worst
text = json.dumps(out, indent=1)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")

#!/usr/bin/env python3
"""Where the origin tolerance of tests/test_gpu_medium.py comes from (CPU only: the oracle and the restatement, no device).
The scene of that test -- sine_heights(96), max_height 0.5, two orthographic 64 x 64 x 4 wavefronts from one origin of
which the second passes partly beside the terrain (tests/medium_ref.py: ORIGIN, WIDE) -- under the three media MEDIA and
the two lights RIG, K = 4 points per sample: the oracle intersects the primary rays, tests/medium_ref.py forms shadow
ray k of every sample towards every light in float64 (the exact point o + u_k d) and as the kernel does (u_k rounded to
float32, one fused multiply-add per component), and the oracle's ray_test decides the float32 rays.
Per medium: the shares of hits and of eligible samples, the smallest S, per light the visible share of the traced rays,
the largest distance between the float32 and the float64 origin, and the share of traced lanes left out of the
comparison with the oracle (origin closer to the primary hit than the sky row's spawn offset); last, the maxima.  The GPU
is allowed four times `origin_max` (tests/test_gpu_medium.py), and at most row_helpers.UNSURE_CAP of its lanes may be
left out.
usage: python scripts/medium_f32_error.py [--out profiles/medium/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import medium_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
r, t, p, field = R.oracle_scene()
lights = R.rig()
out = {}
for name, spec in R.MEDIA.items():
    M = R.medium(**spec)
    q = R.segment(M, r[0:3], r[3:6], t)
    R.assert_scene(name, q, t)
    e = {"hits": float(np.isfinite(t).mean()), "eligible": float(q.elig.mean()), "S_min": float(q.S.min()), "lights": []}
    err, near, traced, seen = 0.0, 0, 0, 0
    for L in lights:
        v = tr = 0
        for k in range(R.K):
            x = R.probe(M, L, r, t, p, field, k)
            err = max(err, float(np.abs(x.o32 - x.o64)[:, x.tr].max()))
            near += int(x.near.sum()); tr += int(x.tr.sum()); v += int(x.vis.sum())
        e["lights"].append({"nu": R.nu(M, L), "visible_of_traced": v / tr})
        traced += tr; seen += v
    e.update(origin_err=err, left_out_share=near / traced, visible_of_traced=seen / traced)
    assert 0.05 <= e["visible_of_traced"] <= 0.95, e
    out[name] = e
    print(name, json.dumps(e), flush=True)
out["maxima"] = {"origin_max": max(v["origin_err"] for v in out.values()), "left_out_share_max": max(v["left_out_share"] for v in out.values())}
print("maxima", json.dumps(out["maxima"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

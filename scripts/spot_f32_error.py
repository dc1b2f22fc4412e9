#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_spot.py come from (CPU only: the oracle and the restatement, no device).  The 4
scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins, flat and
smooth shading normals -- under the rig of 8 spot lights of tests/spot_ref.py (RIG, albedo ALBEDO) are run through the
oracle's intersection, the restatement's shadow rays and the oracle's ray_test; tests/spot_ref.py (forward, tangent, adjoint
with the K x 15 reduced numbers) is then evaluated in float32 numpy against float64 on the same float32 records and
visibility, for the whole rig in one evaluation, weighted and unweighted (weights in [0.5, 1.5], standard normal upstream
gradients and tangents: spot_ref.inputs).  Lanes within KINK of theta = beam are taken out of a light's visibility first
(the slope of the falloff jumps there).
Per scene and light: the shares the issue of this row quotes (in cone of eligible, in the zone of traced, occluded of traced),
the share of samples on which rounding may decide a mask (a deciding quantity within MARGIN; left out of mask comparisons)
and the share within KINK; per scene: the worst error of every quantity (spot_ref.errors); last, the maxima.  The GPU is
allowed four times the maxima (tests/test_gpu_spot.py F32).
usage: python scripts/spot_f32_error.py [--out profiles/spot/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import spot_ref as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
lights = P.rig()
K = len(lights)
out = {}
for key, rec, r, t, field in P.oracle_scenes():
    n = len(t)
    x = P.inputs(n, P.SPP, K)
    e = {"hits": float(np.isfinite(t).mean()), "lights": {}}
    vis, union = [], np.zeros(n, bool)
    for name, L in zip(P.NAMES, lights):
        q = P.probe(L, rec, r, t, field)
        e["lights"][name] = q.shares
        union |= q.unsure
        vis.append(P.steady(L, rec["p"], q.vis))
    e["unsure_union"] = float(union.mean())
    P.assert_shares(e["lights"], e["unsure_union"])
    vis = np.stack(vis)
    for weighted in (True, False):
        r64 = P.evaluate(lights, rec, x, vis, P.SPP, np.float64, weighted)
        r32 = P.evaluate(lights, rec, x, vis, P.SPP, np.float32, weighted)
        for k, err in P.errors(r32, r64).items():
            e["err_" + k] = max(e.get("err_" + k, 0.0), err)
    e["value_max"] = float(np.abs(r64.value).max())
    out[key] = e
    print(key, json.dumps(e), flush=True)
ks = [k for k in next(iter(out.values())) if k.startswith("err_")]
out["maxima"] = {k: max(v[k] for v in out.values()) for k in ks}
scenes = [v for v in out.values() if "hits" in v]
out["shares"] = {"unsure_union_max": max(v["unsure_union"] for v in scenes),
                 "unsure_share_max": max(s["unsure_share"] for v in scenes for s in v["lights"].values()),
                 "kink_share_max": max(s["kink_share"] for v in scenes for s in v["lights"].values())}
print("maxima", json.dumps(out["maxima"]))
print("shares", json.dumps(out["shares"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

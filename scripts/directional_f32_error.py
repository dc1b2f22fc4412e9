#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_directional.py come from (CPU only: the oracle and the restatement, no device).
The 4 scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins,
flat and smooth shading normals -- under the rig of 8 directional lights of tests/directional_ref.py (RIG, albedo ALBEDO)
are run through the oracle's intersection, the restatement's shadow rays and the oracle's ray_test;
tests/directional_ref.py (forward, tangent, adjoint with the K x 4 reduced numbers) is then evaluated in float32 numpy
against float64 on the same float32 records and visibility, for the whole rig in one evaluation, weighted and unweighted
(weights in [0.5, 1.5], standard normal upstream gradients and tangents: directional_ref.inputs).
Per scene and light: the shares the issue of this row quotes (traced of eligible, occluded of traced); per scene: the share
of samples on which rounding may decide a mask (a deciding quantity within MARGIN; left out of mask and value comparisons)
over the union of the rig, and the worst error of every quantity (directional_ref.errors); last, the maxima.  The GPU is
allowed four times the maxima (tests/test_gpu_directional.py F32).
usage: python scripts/directional_f32_error.py [--out profiles/directional/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import directional_ref as D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
lights = D.rig()
K = len(lights)
out = {}
for key, rec, r, t, field in D.oracle_scenes():
    n = len(t)
    x = D.inputs(n, D.SPP, K)
    e = {"hits": float(np.isfinite(t).mean()), "lights": {}}
    vis, union = [], np.zeros(n, bool)
    for name, L in zip(D.NAMES, lights):
        q = D.probe(L, rec, r, t, field)
        e["lights"][name] = dict(q.shares, unsure_share=float(q.unsure.mean()))
        union |= q.unsure
        vis.append(q.vis)
    e["unsure_union"] = float(union.mean())
    D.assert_shares(e["lights"], e["unsure_union"])
    vis = np.stack(vis)
    for weighted in (True, False):
        r64 = D.evaluate(lights, rec, x, vis, D.SPP, np.float64, weighted)
        r32 = D.evaluate(lights, rec, x, vis, D.SPP, np.float32, weighted)
        for k, err in D.errors(r32, r64).items():
            e["err_" + k] = max(e.get("err_" + k, 0.0), err)
    e["value_max"] = float(np.abs(r64.value).max())
    out[key] = e
    print(key, json.dumps(e), flush=True)
ks = [k for k in next(iter(out.values())) if k.startswith("err_")]
out["maxima"] = {k: max(v[k] for v in out.values()) for k in ks}
scenes = [v for v in out.values() if "hits" in v]
out["shares"] = {"unsure_union_max": max(v["unsure_union"] for v in scenes),
                 "unsure_share_max": max(s["unsure_share"] for v in scenes for s in v["lights"].values())}
print("maxima", json.dumps(out["maxima"]))
print("shares", json.dumps(out["shares"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_specular.py come from (CPU only: the oracle and the restatements, no device).
The 4 scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins,
flat and smooth shading normals -- under the rig of 8 directional lights of tests/directional_ref.py are run through the
oracle's intersection, the directional restatement's shadow rays and the oracle's ray_test: the visibility byte of the
directional row.  tests/specular_ref.py (forward, tangent, adjoint with the K x 4 reduced numbers) is then evaluated in
float32 numpy against float64 on the same float32 records and visibility, for the whole rig in one evaluation, weighted
and unweighted (specular_ref.inputs), with the two roughness rows of the test: "row", spread over [0.05, 0.6], and
"sharp", a constant 0.02; eta = specular_ref.ETA.
Per scene and roughness row: the worst error of every quantity (specular_ref.errors), the largest value and the share of
samples that carry a highlight of any light; last, the maxima per roughness row.  The GPU is allowed four times the maxima
(tests/test_gpu_specular.py F32).
usage: python scripts/specular_f32_error.py [--out profiles/specular/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import directional_ref as D  # noqa: E402
import specular_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
lights = D.rig()
K = len(lights)
out = {}
for key, rec, r, t, field in D.oracle_scenes():
    n = len(t)
    x = R.inputs(n, D.SPP, K)
    e = {"hits": float(np.isfinite(t).mean()), "lights": {}}
    vis, union = [], np.zeros(n, bool)
    for name, L in zip(D.NAMES, lights):
        q = D.probe(L, rec, r, t, field)
        e["lights"][name] = q.shares
        union |= q.unsure
        vis.append(q.vis)
    D.assert_shares(e["lights"], float(union.mean()))
    vis = np.stack(vis)
    for kind in ("row", "sharp"):
        alpha = R.alpha_row(kind, n)
        f = {}
        for weighted in (True, False):
            r64 = R.evaluate(lights, rec["sh_n"], r[3:6], x, alpha, R.ETA, vis, D.SPP, np.float64, weighted)
            r32 = R.evaluate(lights, rec["sh_n"], r[3:6], x, alpha, R.ETA, vis, D.SPP, np.float32, weighted)
            for k, err in R.errors(r32, r64).items():
                f["err_" + k] = max(f.get("err_" + k, 0.0), err)
        f["value_max"] = float(np.abs(r64.value).max())
        f["lit_share"] = float((r64.value > 0).any(0).mean())
        e[kind] = f
    out[key] = e
    print(key, json.dumps({k: e[k] for k in ("row", "sharp")}), flush=True)
scenes = list(out.values())
out["maxima"] = {kind: {k: max(v[kind][k] for v in scenes) for k in scenes[0][kind] if k.startswith("err_")} for kind in ("row", "sharp")}
print("maxima", json.dumps(out["maxima"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

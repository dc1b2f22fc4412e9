#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_bumpmap.py come from (CPU only: the oracle and the restatement, no device).
The 4 scenes of that test -- tests/row_scenes.py CASES, the view `steep` -- are run through the oracle's intersection;
tests/bumpmap_ref.py (forward, tangent, adjoint) is then evaluated in float32 numpy against float64 on the same float32
records, for both textures (bumpmap_ref.TEXTURES: 37 x 29 and 16 x 8, bumpmap_ref.texture), both wraps and both scales
(bumpmap_ref.SCALES), under standard normal upstream gradients and tangents (bumpmap_ref.inputs; duv scaled by 0.01; zero
on the lanes within MARGIN of a cell edge, where the slopes jump).  Per run: the shares the tests assert (hit samples near a
cell edge, samples near the pass-through threshold, the smallest |<n_geo, c / |c|>|, the hits with sigma = -1) and the
error of every quantity (bumpmap_ref.errors: per component as the largest difference over max(1, the largest value) on the
lanes away from cell edges, grad_tex as a relative L2); last, the maxima PER TEXTURE AND SCALE -- the slopes are multiplied
by TW, TH and scale, and the figures grow with them.  The GPU is allowed four times the maxima (bumpmap_ref.F32, TOL).
usage: python scripts/bumpmap_f32_error.py [--out profiles/bumpmap/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import bumpmap_ref as R  # noqa: E402
import row_scenes as RS  # noqa: E402
from oracle import hf_oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
hf_oracle.build()
out, maxima = {}, {}
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "steep")
    rec = R.oracle_records(sc, hf_oracle, face_normals)
    for TW, TH in R.TEXTURES:
        tex = R.texture(TW, TH)
        x = R.inputs(sc.n, tex.shape)
        for wname, wrap in R.WRAPS.items():
            for scale in R.SCALES:
                args = (tex, *R.record_args(rec), rec["hit"], wrap, scale)
                _, _, s = R.forward(*args)
                keep = ~R.near_edge(s)
                r64, r32 = R.evaluate(*args, x, keep, np.float64), R.evaluate(*args, x, keep, np.float32)
                assert np.array_equal(r64["mask"], r32["mask"])
                e = dict(R.shares(s, rec["hit"]), hits=float(rec["hit"].mean()))
                e.update({"err_" + k: v for k, v in R.errors(r32, r64, keep).items()})
                key = "%s/%s/%dx%d/%s/%g" % (name, "face" if face_normals else "smooth", TW, TH, wname, scale)
                out[key] = e
                m = maxima.setdefault(R.table_key(TW, TH, scale), {})
                for k, v in e.items():
                    if k.startswith("err_"):
                        m[k] = max(m.get(k, 0.0), v)
                print(key, json.dumps(e), flush=True)
runs = list(out.values())
out["maxima"] = maxima
out["shares"] = {"near_edge_max": max(v["near_edge"] for v in runs), "near_threshold_max": max(v["near_threshold"] for v in runs),
                 "min_cosine": min(v["min_cosine"] for v in runs), "sigma_negative_max": max(v["sigma_negative"] for v in runs)}
print("maxima", json.dumps(out["maxima"]))
print("shares", json.dumps(out["shares"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

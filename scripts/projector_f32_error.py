#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_projector.py come from (CPU only: the oracle and the restatement, no device).
The 8 scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins,
flat and smooth shading normals, the two projectors of tests/projector_ref.py (PROJECTORS, scale SCALE, albedo ALBEDO,
the 16 x 8 texture `random` of refract_ref.textures) -- are run through the oracle's intersection, the restatement's
shadow rays and the oracle's ray_test; tests/projector_ref.py (forward, tangent, adjoint with the 14 reduced numbers) is
then evaluated in float32 numpy against float64 on the same float32 records and visibility, under wrap clamp and repeat
and without a texture (weights in [0.5, 1.5], standard normal upstream gradients and tangents: projector_ref.inputs).
Lanes whose texel coordinate lies within BORDER of a border between two cells of the lookup are taken out of the
visibility first (another rounding may read another cell there: the slopes jump).
Per scene: the shares the issue of this row quotes (lit of eligible, traced of eligible, occluded of traced), the smallest
ref.z of a traced sample, the share of samples on which rounding may decide a mask (a deciding quantity within MARGIN; left
out of mask comparisons), and the worst error of every quantity (projector_ref.errors); last, the maxima.  The GPU is
allowed four times the maxima (tests/test_gpu_projector.py F32).
usage: python scripts/projector_f32_error.py [--out profiles/projector/f32_error.json]"""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import hf_amd  # noqa: E402
from oracle import hf_oracle as O  # noqa: E402
import projector_ref as P  # noqa: E402
import lighting_scenes as LS  # noqa: E402

SPP = 4
TW, TH = P.TEX
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
O.build()
h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
f = O.OracleField(h, max_height=0.5)
tex = P.textures(TW, TH)["random"]
out = {}
for origin in ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0)):
    r = hf_amd.workload.ortho_rays(64, 64, SPP, "cpu", seed=1, origin=origin, target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0)).numpy()
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, O.RAY_ALL)
    hit = np.isfinite(t)
    sc = types.SimpleNamespace(h64=h.astype(np.float64), max_height=0.5, to_world=LS.IDENTITY, flip=False)
    smooth = LS.smooth_normals(sc, r, prim, hit).astype(np.float32)
    n = len(t)
    x = P.inputs(n, SPP, (TH, TW))
    for mode, sh in (("face", rec["sh_n"]), ("smooth", smooth)):
        el, _ = P.eligible(sh, r[3:6], t)
        for pname in sorted(P.PROJECTORS):
            pr = P.PROJECTORS[pname]()
            tr, unsure = P.traced(pr, rec["p"], sh, r[3:6], t)
            o, w, maxt, trk = P.rays(pr, rec["p"], rec["n"], sh, r[3:6], t)
            rows = np.concatenate([o, w, maxt[None]]).astype(np.float32)
            occ = np.zeros(n, bool); occ[tr] = f.ray_test(rows[:, tr]).astype(bool)
            vis = tr & ~occ
            m = P.mapping(pr, rec["p"])
            e = {"hits": float(hit.mean()), "eligible": float(el.mean()), "lit_of_eligible": float(m.lit[el].mean()),
                 "traced_of_eligible": float(tr[el].mean()), "occluded_of_traced": float(occ[tr].mean()),
                 "smallest_ref_z": float(m.ref[2][tr].min()), "unsure_share": float(unsure.mean())}
            assert e["unsure_share"] <= 1e-3, e
            steady = P.steady(pr, rec["p"], vis)
            e["near_border_of_visible"] = float(1.0 - steady.sum() / max(vis.sum(), 1))
            record = {"p": rec["p"], "sh_n": sh}
            lanes = np.nan_to_num(m.ref[2]) > 0
            for name, tx, wrap in (("clamp", tex, P.CLAMP), ("repeat", tex, P.REPEAT), ("none", None, P.REPEAT)):
                r64 = P.evaluate(pr, record, x, tx, wrap, steady, SPP, np.float64)
                r32 = P.evaluate(pr, record, x, tx, wrap, steady, SPP, np.float32)
                for k, err in P.errors(r32, r64, lanes).items():
                    e["err_" + k] = max(e.get("err_" + k, 0.0), err)
                e["value_max"] = max(e.get("value_max", 0.0), float(np.abs(r64.value).max()))
            key = "origin %s, %s normals, projector %s" % (origin, mode, pname)
            out[key] = e
            print(key, json.dumps(e), flush=True)
ks = [k for k in next(iter(out.values())) if k.startswith("err_")]
out["maxima"] = {k: max(v[k] for v in out.values()) for k in ks}
out["shares"] = {"unsure_share_max": max(v["unsure_share"] for v in out.values() if "hits" in v),
                 "smallest_ref_z": min(v["smallest_ref_z"] for v in out.values() if "hits" in v)}
print("maxima", json.dumps(out["maxima"]))
print("shares", json.dumps(out["shares"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

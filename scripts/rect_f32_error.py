#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_rect.py come from (CPU only: the oracle and the restatement, no device).
The 8 scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins,
flat and smooth shading normals, the two lamps of tests/rect_ref.py (LAMPS, radiance RADIANCE, albedo ALBEDO) -- are run
through the oracle's intersection, the restatement's shadow rays and the oracle's ray_test; tests/rect_ref.py is then
evaluated in float32 numpy against float64 on the same float32 records and visibility, for K = 1, 8, 32, without a
texture and with the two 16 x 8 textures (weights in [0.5, 1.5], standard normal upstream gradients and tangents:
rect_ref.inputs).
Per scene: the shares the issue of this row quotes (traced draws of eligible samples, occluded of traced, samples in
penumbra, at K = 8), the smallest r of a traced draw, the share of samples on which rounding may decide a mask (a deciding
quantity within MARGIN; left out of mask comparisons), and the worst error of every quantity (value and image absolute;
every derivative as the L2 norm of the difference over the L2 norm of the float64 result); last, the maxima.  The GPU is
allowed four times the maxima (tests/test_gpu_rect.py F32).
usage: python scripts/rect_f32_error.py [--out profiles/rect/f32_error.json]"""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import hf_amd  # noqa: E402
from oracle import hf_oracle as O  # noqa: E402
import rect_ref as A  # noqa: E402
import lighting_scenes as LS  # noqa: E402

SPP, TW, TH, SEED, KMAX = 4, 16, 8, 5, 32
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
O.build()
h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
f = O.OracleField(h, max_height=0.5)
TEX = {None: None, **A.textures(TW, TH)}
out = {}
for origin in ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0)):
    r = hf_amd.workload.ortho_rays(64, 64, SPP, "cpu", seed=1, origin=origin, target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0)).numpy()
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, O.RAY_ALL)
    hit = np.isfinite(t)
    sc = types.SimpleNamespace(h64=h.astype(np.float64), max_height=0.5, to_world=LS.IDENTITY, flip=False)
    smooth = LS.smooth_normals(sc, r, prim, hit).astype(np.float32)
    n = len(t)
    ids = np.arange(n, dtype=np.uint32)
    x = A.inputs(n, SPP, (TH, TW))
    for mode, sh in (("face", rec["sh_n"]), ("smooth", smooth)):
        el, front = A.eligible(sh, r[3:6], t)
        for lname in A.LAMPS:
            lm = A.LAMPS[lname](A.RADIANCE)
            g = A.geometry(rec["p"], sh, A.draws(ids, KMAX, SEED), lm)
            tr, margin = A.traced(sh, r[3:6], t, g)
            bits = np.zeros((KMAX, n), bool)
            for k in range(KMAX):
                o, w, maxt, trk = A.rays(rec["p"], rec["n"], sh, r[3:6], t, ids, k, SEED, lm)
                assert np.array_equal(trk, tr[k])
                rows = np.concatenate([o, w, maxt[None]]).astype(np.float32)
                occ = np.zeros(n, bool); occ[trk] = f.ray_test(rows[:, trk]).astype(bool)
                bits[k] = trk & ~occ
            t8, b8 = tr[:8], bits[:8]
            some, every = b8.any(0), (b8 == t8).all(0)
            unsure = el & ((front < A.MARGIN) | (margin < A.MARGIN).any(0))
            e = {"hits": float(hit.mean()), "eligible": float(el.mean()), "traced_of_eligible_draws": float(t8[:, el].mean()),
                 "occluded_of_traced": float(1.0 - b8.sum() / t8.sum()), "penumbra_of_eligible": float((some & ~every)[el].mean()),
                 "smallest_r": float(g.r[tr].min()), "unsure_share": float(unsure.mean())}
            for K in (1, 8, 32):
                for name, tex in TEX.items():
                    res = {}
                    for dt in (np.float64, np.float32):
                        c = (rec["p"], sh, r[3:6], t, x.w, bits[:K], ids, SEED, lm, tex, A.ALBEDO, SPP)
                        img, val = A.forward(*c, dt)
                        gn, gp, gw, gt = A.adjoint(*c, x.gi, dt)
                        dimg, dval = A.tangent(*c, x.dn, x.dp, x.dw, x.dtex, dt)
                        res[dt] = dict(value=val, image=img, grad_sh_n=gn, grad_p=gp, grad_weight=gw, dimage=dimg)
                        if tex is not None:
                            res[dt]["grad_tex"] = gt
                    for k in res[np.float64]:
                        a64, a32 = res[np.float64][k], res[np.float32][k].astype(np.float64)
                        err = float(np.abs(a64 - a32).max()) if k in ("value", "image") else \
                            float(np.linalg.norm(a64 - a32) / np.linalg.norm(a64))
                        e["err_" + k] = max(e.get("err_" + k, 0.0), err)
                    e["value_max"] = max(e.get("value_max", 0.0), float(np.abs(res[np.float64]["value"]).max()))
            key = "origin %s, %s normals, lamp %s" % (origin, mode, lname)
            out[key] = e
            print(key, json.dumps(e), flush=True)
ks = [k for k in next(iter(out.values())) if k.startswith("err_")]
out["maxima"] = {k: max(v[k] for v in out.values()) for k in ks}
out["shares"] = {"unsure_share_max": max(v["unsure_share"] for v in out.values() if "hits" in v),
                 "smallest_r": min(v["smallest_r"] for v in out.values() if "hits" in v)}
print("maxima", json.dumps(out["maxima"]))
print("shares", json.dumps(out["shares"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

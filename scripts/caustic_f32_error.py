#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_caustic.py come from (CPU only: the oracle and the restatements, no device).
The 16 scenes of that test -- sine_heights(96), max_height 0.5, the 64 x 64 x 4 orthographic wavefront from two origins,
flat and smooth shading normals, eta 1.33 and 1 / 1.33, receivers z = -0.5 and z = 0.2 -- are run through the oracle's
intersection and ray_test and tests/caustic_ref.py, which is then evaluated in float32 numpy against float64 on the same
float32 records (weights in [0.5, 1.5], power 1, standard normal upstream gradients and tangents, default_rng(3)).
Per scene: the shares of the masks and the errors (pos in pixels, value absolute, every derivative as the L2 norm of the
difference over the L2 norm of the float64 result); last, the maxima per quantity.
usage: python scripts/caustic_f32_error.py [--out profiles/caustic/f32_error.json]"""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import hf_amd  # noqa: E402
from oracle import hf_oracle as O  # noqa: E402
import caustic_ref as R  # noqa: E402
import lighting_scenes as LS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
O.build()
h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
f = O.OracleField(h, max_height=0.5)
out = {}
for origin in ((1.2, 0.3, 1.2), (0.6, 0.35, 2.0)):
    r = hf_amd.workload.ortho_rays(64, 64, 4, "cpu", seed=1, origin=origin, target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0)).numpy()
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, O.RAY_ALL)
    hit = np.isfinite(t)
    sc = types.SimpleNamespace(h64=h.astype(np.float64), max_height=0.5, to_world=LS.IDENTITY, flip=False)
    smooth = LS.smooth_normals(sc, r, prim, hit).astype(np.float32)
    for mode, sh in (("face", rec["sh_n"]), ("smooth", smooth)):
        for eta in (1.33, 1 / 1.33):
            for z in (-0.5, 0.2):
                rcv = R.plane_z(z, (-1, 1), (-1, 1), 64, 64)
                arg = (rec["p"], rec["n"], sh, r[3:6], t, None)
                tr, o, wo, maxt, vx = R.rays(*arg, eta, rcv)
                rows = np.concatenate([o, wo, maxt[None]]).astype(np.float32)
                occ = np.zeros(len(t), bool); occ[tr] = f.ray_test(rows[:, tr]).astype(bool)
                rows[6] = np.where(tr, np.inf, -1)
                occ_inf = np.zeros(len(t), bool); occ_inf[tr] = f.ray_test(rows[:, tr]).astype(bool)
                vis = tr & ~occ
                n = len(t); rng = np.random.default_rng(3)
                w = rng.uniform(0.5, 1.5, n).astype(np.float32)
                gpos, gv = rng.normal(size=(2, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
                dn, dp, dw = (rng.normal(size=s).astype(np.float32) for s in ((3, n), (3, n), (n,)))
                res = {}
                for dt in (np.float64, np.float32):
                    pos, val = R.forward(*arg, w, eta, 1.0, rcv, vis, dt)
                    gm, gp, gw = R.adjoint(*arg, w, eta, 1.0, rcv, vis, gpos, gv, dt)
                    dpos, dval = R.tangent(*arg, w, eta, 1.0, rcv, vis, dn, dp, dw, dt)
                    res[dt] = dict(pos=pos, value=val, grad_sh_n=gm, grad_p=gp, grad_weight=gw, dpos=dpos, dvalue=dval)
                el = vx.eligible
                e = {"hits": float(hit.mean()), "eligible_of_hits": float(el.sum() / hit.sum()),
                     "tir_of_hits": float((el & vx.tir).sum() / hit.sum()),
                     "inconsistent": int((el & ~vx.tir & ~vx.consistent).sum()), "traced": int(tr.sum()),
                     "occluded_of_traced": float(occ.sum() / max(tr.sum(), 1)), "answers_changed_by_maxt": int((occ != occ_inf).sum()),
                     "lanes_within_1e-5_of_a_decision": int((hit & (vx.margin < 1e-5)).sum())}
                for k in res[np.float64]:
                    a64, a32 = res[np.float64][k], res[np.float32][k].astype(np.float64)
                    e["err_" + k] = float(np.abs(a64 - a32).max()) if k in ("pos", "value") else float(np.linalg.norm(a64 - a32) / np.linalg.norm(a64))
                key = "origin %s, %s normals, eta %.4f, z %.1f" % (origin, mode, eta, z)
                out[key] = e
                print(key, json.dumps(e), flush=True)
ks = [k for k in next(iter(out.values())) if k.startswith("err_")]
out["maxima"] = {k: max(v[k] for v in out.values()) for k in ks}
print("maxima", json.dumps(out["maxima"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

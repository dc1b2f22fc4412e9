#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_glossy.py come from (CPU only: the oracle and the restatements, no device).
The scenes of that test -- sine_heights(96), max_height 0.5, the 25 x 23 x 4 orthographic wavefront from two origins,
flat and smooth shading normals, eta 0 and 1.5 and the seven (num_rays, alpha, map, rotation) combinations of
tests/glossy_ref.py COMBOS -- are run through the oracle's intersection and ray_test and tests/glossy_ref.py, which is
then evaluated in float32 numpy against float64 on the same float32 records (weights in [0.5, 1.5], standard normal
upstream gradients and tangents, 0.1 standard normal for alpha; default_rng(3); spp 4).  Per scene: the shares of the
masks and of the samples with a direction within 1e-5 of a mask decision (<wi, h>, c_o, <g, wo>, c_i, <g, wi>; the
denominator of the draw's norm within 1e-4) -- these are left out of every comparison --, the share of samples with a
lookup within 1e-4 of a cell border (counted, NOT left out: the direction is held, so no derivative of this row jumps
there), and the errors (value and image absolute; every derivative, the ray directions, origins and microfacet normals
as the L2 norm of the difference over the L2 norm of the float64 result); last, the maxima per quantity.
usage: python scripts/glossy_f32_error.py [--out profiles/glossy/f32_error.json]"""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import hf_amd  # noqa: E402
from oracle import hf_oracle as O  # noqa: E402
import envmap_ref as E  # noqa: E402
import glossy_ref as G  # noqa: E402
import reflect_ref as R  # noqa: E402
import lighting_scenes as LS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
O.build()
MARGIN, BORDER = 1e-5, 1e-4
h = hf_amd.workload.sine_heights(96, 96, device="cpu").numpy()
f = O.OracleField(h, max_height=0.5)
out = {}
for origin in G.ORIGINS:
    r = hf_amd.workload.ortho_rays(*G.FILM, "cpu", seed=1, origin=origin, target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0)).numpy()
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, O.RAY_ALL)
    hit = np.isfinite(t)
    n = len(t)
    sc = types.SimpleNamespace(h64=h.astype(np.float64), max_height=0.5, to_world=LS.IDENTITY, flip=False)
    smooth = LS.smooth_normals(sc, r, prim, hit).astype(np.float32)
    for mode, sh in (("face", rec["sh_n"]), ("smooth", smooth)):
        for K, akind, name, rname in G.COMBOS:
            al = G.alpha_row(akind, n)
            rot = G.ROTS[rname]
            W, H = G.MAP_SIZES[name]
            data = E.MAPS[name](W, H)
            bits, margin, near = np.zeros((K, n), bool), np.full(n, np.inf), np.zeros(n, bool)
            e_ray = {"ray_d": [0.0, 0.0], "ray_o": [0.0, 0.0], "ray_h": [0.0, 0.0]}
            for k in range(K):
                tr, o, wo, maxt, hh, m, dr = G.rays(rec["p"], rec["n"], sh, r[3:6], t, al, k, G.SEED)
                rows = np.concatenate([o, wo, maxt[None]]).astype(np.float32)
                occ = np.zeros(n, bool); occ[tr] = f.ray_test(rows[:, tr]).astype(bool)
                bits[k] = tr & ~occ
                margin = np.minimum(margin, m)
                near |= bits[k] & ~R.smooth_lanes(wo, W, H, rot, BORDER)
                d32 = G.draw(sh, r[3:6], al, np.arange(n), k, G.SEED, 0.0, np.float32)
                sure = tr & (m > MARGIN)
                for key, x64, x32 in (("ray_d", wo, d32.wo), ("ray_h", hh, d32.h)):
                    e_ray[key][0] += ((x64 - x32)[:, sure] ** 2).sum(); e_ray[key][1] += (x64[:, sure] ** 2).sum()
            keep = (margin > MARGIN) | ~hit
            lit = bits.any(0)
            masks = {"hits": float(hit.mean()), "lit_samples": int(lit.sum()), "set_bits_of_hits": float(bits.sum() / (K * hit.sum())),
                     "unsure_share": float((hit & ~keep).mean()), "near_border_share": float(near.mean())}
            for eta in (0.0, 1.5):
                w, gi, gv, dn, dw, da, dd = G.test_inputs(n, data.shape)
                dn = dn * keep
                arg = (rec["n"], sh, r[3:6], t, None, w, al, eta, K, G.SEED, None, data, rot, bits, G.SPP)
                res = {}
                for dt in (np.float64, np.float32):
                    img, val = G.forward(*arg, dtype=dt)
                    gm, gw, ga, gd = G.adjoint(*arg, gi * keep.reshape(-1, G.SPP).all(1), gv * keep, dtype=dt)
                    dimg, dval = G.tangent(*arg, dn, dw * keep, da * keep, dd, dtype=dt)
                    res[dt] = dict(value=val[keep], image=img[keep.reshape(-1, G.SPP).all(1)], grad_sh_n=gm[:, keep], grad_weight=gw[keep],
                                   grad_alpha=ga[keep], grad_data=gd, dimage=dimg[keep.reshape(-1, G.SPP).all(1)], dvalue=dval[keep])
                e = dict(masks)
                for k_ in res[np.float64]:
                    a64, a32 = res[np.float64][k_], res[np.float32][k_].astype(np.float64)
                    e["err_" + k_] = float(np.abs(a64 - a32).max()) if k_ in ("value", "image") else float(np.linalg.norm(a64 - a32) / np.linalg.norm(a64))
                for k_, (num, den) in e_ray.items():
                    if den:
                        e["err_" + k_] = float(np.sqrt(num / den))
                key = "origin %s, %s normals, eta %.1f, K %d, alpha %s, map %s, %s" % (origin, mode, eta, K, akind, name, rname)
                out[key] = e
                print(key, json.dumps(e), flush=True)
ks = sorted({k for v in out.values() for k in v if k.startswith("err_") or k.endswith("_share")})
out["maxima"] = {k: max(v.get(k, 0.0) for v in out.values()) for k in ks}
print("maxima", json.dumps(out["maxima"]))
assert out["maxima"]["unsure_share"] <= 1e-3, "a scene has more than 1e-3 of its samples near a mask decision: change the scene"
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

#!/usr/bin/env python3
"""Where the tolerances of tests/test_gpu_row_scenes.py come from (CPU only: the oracle and the restatements, no device).
Every (row, scene, shading mode) of tests/row_scenes.py -- the directional, spot, caustic, refract, rect, projector, reflect and glossy rows on `affine` (flat and smooth
normals), `mirror_flip` and `flip_below` of tests/lighting_scenes.py, 25 x 23 x 4 samples, the rows' rigs carried to world
-- is run through the oracle's intersection, the restatement's shadow rays and the oracle's ray_test; the restatement
(directional_ref / spot_ref: forward, tangent, adjoint with the reduced numbers of the lights) is then evaluated in float32
numpy against float64 on the same float32 records and visibility, for the whole rig in one evaluation, weighted and
unweighted (the rows' own inputs()).  For the spot row lanes within KINK of theta = beam are taken out of a light's
visibility first, as scripts/spot_f32_error.py does.  The caustic row (tests/caustic_ref.py, the oblique view, eta 1.33
and 1 / 1.33, the far and the cutting receiver carried to world) is measured as scripts/caustic_f32_error.py measures it, the rect row
(tests/rect_ref.py, both lamps, 8 draws, with and without a texture) in the measures of tests/test_gpu_rect.py, the
projector row (tests/projector_ref.py, both projectors, that test's three variants of wrap and texture) in projector_ref.errors(), the
reflect row (tests/reflect_ref.py, the oblique view, eta 0 and 1.5, two maps) in the measures of tests/test_gpu_reflect.py, the
refract row (tests/refract_ref.py, the caustic row's runs on a textured receiver, two variants of absorption, texture and wrap)
and the glossy row (tests/glossy_ref.py, 4 draws, two roughness rows and maps, eta 0 and 1.5) in those of their own tests.
The specular row (tests/specular_ref.py, the steep view, the directional row's rig and visibility, eta 1.5) is measured in
specular_ref.errors() per roughness row ("row" on every case, "sharp" on affine with smooth normals: its maxima are a
dict per roughness row); of the medium row (tests/medium_ref.py, the three media of row_scenes.MEDIA carried to world,
4 points per sample) only the origin of a shadow ray has a float32 restatement: the measure of scripts/medium_f32_error.py,
per (scene, medium), with the populations tests/test_row_scenes.py asserts -- its values keep the row's own rule.
Per triple: the populations tests/test_row_scenes.py asserts and the error of every quantity (the rows' own errors());
last, per row, the maxima over the triples.  The GPU is allowed four times the maxima (tests/test_gpu_row_scenes.py F32).
usage: python scripts/row_scenes_f32_error.py [--out profiles/row_scenes/f32_error.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import row_scenes as RS  # noqa: E402
from oracle import hf_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
O.build()
out = {}
for row in RS.ROWS:
    M = RS.REF[row]
    out[row] = {}
    for name, face_normals in RS.CASES:
        sc = RS.scene(name, RS.VIEW_OF[row])
        m = RS.model(row, sc, O, face_normals)
        RS.conditions(row, sc, m.pop)
        K = len(m.lights)
        x = M.inputs(sc.n, RS.SPP, K)
        vis = m.vis if row == "directional" else np.stack([M.steady(L, m.rec["p"], v) for L, v in zip(m.lights, m.vis)])
        e = {"hits": int(np.isfinite(m.t).sum()), "eligible": int(m.pop.eligible.sum()), "unsure_union": m.pop.unsure_share,
             "ends_inside_the_bound": m.pop.inside, "changed_by_inf": m.pop.changed, "lights": m.pop.shares,
             "max_coordinate": float(np.abs(m.rec["p"]).max())}
        for weighted in (True, False):
            r64 = M.evaluate(m.lights, m.rec, x, vis, RS.SPP, np.float64, weighted)
            r32 = M.evaluate(m.lights, m.rec, x, vis, RS.SPP, np.float32, weighted)
            for k, err in M.errors(r32, r64).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
        e["value_max"] = float(np.abs(r64.value).max())
        key = "%s, %s normals" % (name, "face" if face_normals else "smooth")
        out[row][key] = e
        print(row, key, json.dumps(e), flush=True)
    ks = [k for k in e if k.startswith("err_")]
    out[row]["maxima"] = {k: max(v[k] for v in out[row].values()) for k in ks}
    print(row, "maxima", json.dumps(out[row]["maxima"]))
# ---- the caustic row: tests/test_gpu_caustic.py's measures (pos in pixels, value absolute, every derivative as the L2 norm
# of the difference over the L2 norm of the float64 result) and the rays' maxt relative to itself, on the lanes that no rounding decides
import caustic_ref as C  # noqa: E402
out["caustic"] = {}
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "oblique")
    runs = RS.caustic_model(sc, O, face_normals)
    RS.caustic_conditions(sc, runs)
    w, gpos, gv, dn, dp, dw = RS.caustic_inputs(sc.n)
    for (eta, plane), r in runs.items():
        res = {}
        for dt in (np.float64, np.float32):
            arg = (*r.a, None, w, eta, 1.0, r.rref, r.vis)
            pos, val = C.forward(*arg, dt)
            gm, gp, gw = C.adjoint(*arg, gpos, gv, dt)
            dpos, dval = C.tangent(*arg, dn, dp, dw, dt)
            res[dt] = dict(pos=pos, value=val, grad_sh_n=gm, grad_p=gp, grad_weight=gw, dpos=dpos, dvalue=dval)
        e = dict(r.counts)
        e["max_pos"] = float(np.abs(res[np.float64]["pos"][:, r.vis]).max())
        for k in res[np.float64]:
            a64, a32 = res[np.float64][k][..., r.sure], res[np.float32][k][..., r.sure].astype(np.float64)
            e["err_" + k] = float(np.abs(a64 - a32).max()) if k in ("pos", "value") else float(np.linalg.norm(a64 - a32) / np.linalg.norm(a64))
        # maxt = s of the traced rays, relative: near the critical angle and at grazing incidence on the receiver s is a
        # quotient of two small numbers (the worst lane here: s = 169, <wo, N> = -0.006, cos_theta_t^2 = 7e-4)
        # -- which is why the ray's END is held to the receiver as well: |<p + wo s - origin, N>| in world units, where
        # an error of s counts <wo, N> times
        v32 = C.vertex(*r.a, None, eta, r.rref, np.float32)
        lanes = r.traced & r.sure
        e["err_maxt"] = float((np.abs(v32.s.astype(np.float64) - r.v.s)[lanes] / r.v.s[lanes]).max())
        e["err_end"] = float(RS.caustic_end(r, v32.wo.astype(np.float64), v32.s.astype(np.float64))[lanes].max())
        key = "%s, %s normals, eta %.4f, %s" % (name, "face" if face_normals else "smooth", eta, plane)
        out["caustic"][key] = e
        print("caustic", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["caustic"]["maxima"] = {k: max(v[k] for v in out["caustic"].values()) for k in ks}
print("caustic maxima", json.dumps(out["caustic"]["maxima"]))
# ---- the rect row: tests/test_gpu_rect.py's measures, both lamps, without a texture and with the smooth one
import rect_ref as A  # noqa: E402
out["rect"] = {}
tex = A.textures(*RS.RECT_TEX)["smooth"]
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "steep")
    f, rec, t, _ = RS.oracle_records(sc, O, face_normals)
    runs = RS.rect_model(sc, O, face_normals)
    RS.rect_conditions(sc, runs)
    x = A.inputs(sc.n, RS.SPP, RS.RECT_TEX[::-1])
    for lname, r in runs.items():
        e = dict(r.counts)
        pix = r.sure.reshape(-1, RS.SPP).all(1)
        for tx in (None, tex):
            r64, r32 = (RS.rect_evaluate(r, rec, sc.rays[3:6], t, x, tx, dt) for dt in (np.float64, np.float32))
            for k, err in RS.rect_errors(r32, r64, r.sure, pix).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
        e["value_max"] = float(np.abs(r64["value"]).max())
        key = "%s, %s normals, %s" % (name, "face" if face_normals else "smooth", lname)
        out["rect"][key] = e
        print("rect", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["rect"]["maxima"] = {k: max(v[k] for v in out["rect"].values()) for k in ks}
print("rect maxima", json.dumps(out["rect"]["maxima"]))
# ---- the projector row: projector_ref.errors(), both projectors, the variants of tests/test_gpu_projector.py
import projector_ref as PR  # noqa: E402
out["projector"] = {}
ptex = PR.textures(*PR.TEX)["random"]
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "steep")
    runs, rec, t = RS.projector_model(sc, O, face_normals)
    RS.projector_conditions(sc, runs)
    x = PR.inputs(sc.n, RS.SPP, PR.TEX[::-1])
    for pname, r in runs.items():
        e = dict(r.counts)
        for wrap, textured in RS.PROJ_VARIANTS:
            b = (r.pr, rec, x, ptex if textured else None, {"clamp": PR.CLAMP, "repeat": PR.REPEAT}[wrap], r.steady, RS.SPP)
            r64, r32 = PR.evaluate(*b, np.float64), PR.evaluate(*b, np.float32)
            for k, err in PR.errors(r32, r64, r.lanes & r.sure).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
        e["value_max"] = float(np.abs(r64.value).max())
        key = "%s, %s normals, %s" % (name, "face" if face_normals else "smooth", pname)
        out["projector"][key] = e
        print("projector", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["projector"]["maxima"] = {k: max(v[k] for v in out["projector"].values()) for k in ks}
print("projector maxima", json.dumps(out["projector"]["maxima"]))
# ---- the reflect row: tests/test_gpu_reflect.py's measures, eta 0 and 1.5, two maps under two rotations
import envmap_ref as E  # noqa: E402
out["reflect"] = {}
rots = RS.reflect_rots()
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "oblique")
    r, rec, t = RS.reflect_model(sc, O, face_normals)
    RS.reflect_conditions(sc, r)
    e = dict(r.counts)
    for mname, rname in RS.REFLECT_PAIRS:
        full = E.MAPS[mname](*RS.REFLECT_MAPS[mname])
        keep = RS.reflect_keep(r, full, rots[rname])
        e["left_out"] = max(e.get("left_out", 0.0), float((r.vis & ~keep).mean()))
        x = RS.reflect_inputs(sc.n, full.shape)
        for eta in RS.REFLECT_ETAS:
            r64, r32 = (RS.reflect_evaluate(r, eta, full, rots[rname], x, keep, dt) for dt in (np.float64, np.float32))
            for k, err in RS.reflect_errors(r32, r64, keep, r.vis).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
    key = "%s, %s normals" % (name, "face" if face_normals else "smooth")
    out["reflect"][key] = e
    print("reflect", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["reflect"]["maxima"] = {k: max(v[k] for v in out["reflect"].values()) for k in ks}
print("reflect maxima", json.dumps(out["reflect"]["maxima"]))
# ---- the refract row: tests/test_gpu_refract.py's measures over REFRACT_VARIANTS, and the landing position in texels
import refract_ref as RR  # noqa: E402
out["refract"] = {}
rtex = RR.textures(*RS.REFRACT_TEX)
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "oblique")
    runs = RS.refract_model(sc, O, face_normals)
    RS.refract_conditions(sc, runs)
    x = RR.inputs(sc.n, RS.SPP, RS.REFRACT_TEX[::-1])
    for (eta, plane), r in runs.items():
        e = dict(r.counts)
        for sigma_t, tname, wrap in RS.REFRACT_VARIANTS:
            b = (r, eta, sigma_t, rtex[tname], {"clamp": RR.CLAMP, "repeat": RR.REPEAT}[wrap], x)
            r64, r32 = RS.refract_evaluate(*b, np.float64), RS.refract_evaluate(*b, np.float32)
            for k, err in RS.refract_errors(r32, r64, r.keep, r.pix).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
        p64, p32 = (RR.forward(*r.a, None, None, eta, 0.0, r.rref, rtex["smooth"], RR.CLAMP, r.vis, 1, dt)[2] for dt in (np.float64, np.float32))
        e["err_pos"] = float(np.abs(p64 - p32)[:, r.keep].max())
        key = "%s, %s normals, eta %.4f, %s" % (name, "face" if face_normals else "smooth", eta, plane)
        out["refract"][key] = e
        print("refract", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["refract"]["maxima"] = {k: max(v[k] for v in out["refract"].values()) for k in ks}
print("refract maxima", json.dumps(out["refract"]["maxima"]))
# ---- the glossy row: tests/test_gpu_glossy.py's measures, GLOSSY_COMBOS at eta 0 and 1.5, and the rays' directions and normals
import glossy_ref as G  # noqa: E402
out["glossy"] = {}
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "oblique")
    key = "%s, %s normals" % (name, "face" if face_normals else "smooth")
    e = {}
    for akind, mname, rname in RS.GLOSSY_COMBOS:
        r = RS.glossy_model(sc, O, face_normals, akind)
        RS.glossy_conditions(sc, r)
        e["alpha %s" % akind] = r.counts
        full = E.MAPS[mname](*G.MAP_SIZES[mname])
        x = G.test_inputs(sc.n, full.shape)
        for eta in RS.GLOSSY_ETAS:
            r64, r32 = (RS.glossy_evaluate(r, eta, full, G.ROTS[rname], x, dt) for dt in (np.float64, np.float32))
            for k, err in RS.glossy_errors(r32, r64, r.keep).items():
                e["err_" + k] = max(e.get("err_" + k, 0.0), err)
        num = np.zeros(4)
        for k in range(RS.GLOSSY_K):
            dr = G.draw(r.a[1], r.a[2], r.alpha, np.arange(sc.n), k, RS.GLOSSY_SEED, 0.0, np.float32)
            num += RS.glossy_ray_errors(dr.wo.astype(np.float64), dr.h.astype(np.float64), r, k, r.traced[k] & r.sure_k[k])
        e["err_ray_d"] = max(e.get("err_ray_d", 0.0), float(np.sqrt(num[0] / num[1])))
        e["err_ray_h"] = max(e.get("err_ray_h", 0.0), float(np.sqrt(num[2] / num[3])))
    out["glossy"][key] = e
    print("glossy", key, json.dumps(e), flush=True)
ks = [k for k in e if k.startswith("err_")]
out["glossy"]["maxima"] = {k: max(v[k] for v in out["glossy"].values()) for k in ks}
print("glossy maxima", json.dumps(out["glossy"]["maxima"]))
# ---- the specular row: specular_ref.errors() per roughness row, on the oracle's records and the directional row's visibility
import specular_ref as SP  # noqa: E402
out["specular"] = {}
for name, face_normals in RS.CASES:
    sc = RS.scene(name, "steep")
    m = RS.specular_model(sc, O, face_normals)
    RS.specular_conditions(sc, m.pop, m.lit)
    x = SP.inputs(sc.n, RS.SPP, len(m.lights))
    e = {"hits": int(np.isfinite(m.t).sum()), "eligible": int(m.pop.eligible.sum()), "unsure_union": m.pop.unsure_share, "lit": m.lit}
    for akind in RS.specular_kinds(name, face_normals):
        e[akind] = {}
        for weighted in (True, False):
            r64, r32 = (RS.specular_evaluate(m.lights, m.rec, sc.rays[3:6], x, akind, m.vis, dt, weighted) for dt in (np.float64, np.float32))
            for k, err in SP.errors(r32, r64).items():
                e[akind]["err_" + k] = max(e[akind].get("err_" + k, 0.0), err)
        e[akind]["value_max"] = float(np.abs(r64.value).max())
    key = "%s, %s normals" % (name, "face" if face_normals else "smooth")
    out["specular"][key] = e
    print("specular", key, json.dumps(e), flush=True)
out["specular"]["maxima"] = {akind: {k: max(v[akind][k] for v in out["specular"].values() if akind in v) for k in e["row"] if k.startswith("err_")}
                             for akind in ("row", "sharp")}
print("specular maxima", json.dumps(out["specular"]["maxima"]))
# ---- the medium row: scripts/medium_f32_error.py's measure of an origin (the point formed as the kernel forms it, the
# distance rounded to float32 and one fused multiply-add per component, against the exact o + u_k d), every (scene, medium)
out["medium"] = {}
for name in RS.SCENES:
    for mname in RS.MEDIUM_NAMES:
        sc = RS.scene(name, RS.MEDIA[mname]["view"])
        r = RS.medium_model(sc, O, mname)
        RS.medium_conditions(sc, r)
        e = dict(r.counts)
        e.update(lights=r.shares, nu=[float(v) for v in r.nu], max_coordinate=float(np.abs(r.origins64[:, :, r.q.elig]).max()),
                 err_origin=float(np.abs(r.origins32 - r.origins64)[:, :, r.q.elig].max()))
        key = "%s, %s" % (name, mname)
        out["medium"][key] = e
        print("medium", key, json.dumps(e), flush=True)
out["medium"]["maxima"] = {"err_origin": max(v["err_origin"] for v in out["medium"].values())}
print("medium maxima", json.dumps(out["medium"]["maxima"]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)

#!/usr/bin/env python3
"""Old against new, bit for bit: two builds of libhf.so on the same seeded inputs, one process each on the same device.

usage: scripts/ab_reflection_rows.py OLD.so NEW.so [--out build/ab_reflection_rows] [--compare-only]

Every lighting row that shares the map lookup, the tangent film or the launcher (sky, bounce, envmap, reflect, glossy) and
hf_envmap_eval / _eval_adjoint run on the scenes of tests/lighting_scenes.py and on the 96 x 96 sine field of the
reflection tests, at spp 1, 4, 64 (shuffle-tree film), 3 and 128 (atomic film, one-lane-per-pixel tangent), with and
without `weight`; reflect and glossy through the C ABI, also with `active`, `value` and the image NULL in turn.  A child
process per library writes its outputs to OUT/{old,new}.npz; the parent compares and prints the table:

  * outputs computed without float atomics (every key that does not end in `.atomic`) must differ in 0 words;
  * outputs accumulated with float atomics are held to the bound the GPU test of that row uses for the same quantity,
    applied to |old - new|: images at spp 3 / 128 -- sky, bounce: tests/lighting_scenes.py _close without its sum term;
    envmap: 1e-5 |value| + 1e-7 S (tests/test_gpu_envmap_lighting.py _close; S from the restatement); reflect, glossy:
    2.5e-7 max |value| (the film bound of their odd-sizes tests); grad_data -- envmap and eval_adjoint: per texel
    (m + 5) 2^-24 sum |terms| with m and the sum from tests/envmap_ref.py; reflect, glossy: the relative L2 of TOL["grad_data"]
    in tests/test_gpu_reflect.py / test_gpu_glossy.py.

--compare-only: the two .npz files are there already (no device needed).  The last line is `RESULT: PASS` or `RESULT: FAIL`.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SPPS = (1, 4, 64, 3, 128)
ATOMIC_SPP = (3, 128)
ALBEDO, ETA, ALPHA = 0.7, 1.5, 0.3
MAP, DEFENSIVE = "sun", 0.25


def _inputs(tag, m, shape=None):
    """the seeded upstream gradients and tangents of a case: the same in both processes and in the comparison"""
    rng = np.random.default_rng(sum(map(ord, tag)))
    f = np.float32
    r = {"weight": rng.uniform(0.5, 1.5, m).astype(f), "gvalue": rng.normal(size=m).astype(f),
         "dn": rng.uniform(-0.25, 0.25, (3, m)).astype(f), "dw": rng.uniform(-0.5, 0.5, m).astype(f),
         "da": rng.uniform(-0.1, 0.1, m).astype(f), "active": (rng.uniform(size=m) < 0.9).astype(np.uint8)}
    if shape is not None:
        r["ddata"] = rng.uniform(-0.5, 0.5, shape).astype(f)
    return r


def _gimg(tag, shape):
    return np.random.default_rng(7 + sum(map(ord, tag))).normal(size=shape).astype(np.float32)


# ---- the child: one library, every case, one .npz ------------------------------------------------------------------------
def dump(lib_path, out):
    os.environ["HF_LIB"] = os.path.abspath(lib_path)
    import torch
    import torch.autograd.forward_ad as fwAD
    import hf_amd as hf
    import envmap_ref as E
    import lighting_scenes as LS
    lib, check, fp = hf._capi.lib(), hf._capi.check, hf._capi._fp
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    npy = lambda x: x.detach().cpu().numpy()
    R = {}
    full = E.MAPS[MAP]()                                     # [H, W] with the seam column
    H, W = full.shape
    dat = cu(full.astype(np.float32))
    stream = lambda: torch.cuda.current_stream().cuda_stream
    rows = lambda x: None if x is None else (fp * 3)(*[x.data_ptr() + 4 * k * x.shape[1] for k in range(3)])
    ptr = lambda x: None if x is None else x.data_ptr()

    def scenes():
        for name in LS.NAMES:
            sc = LS.scene(name)
            shape = hf.Heightfield(heightfield=cu(sc.h), max_height=sc.max_height, to_world=np.asarray(sc.to_world, np.float64),
                                   flip_normals=sc.flip)
            yield name, shape, cu(sc.rays), cu(sc.lights)
        rays = hf.workload.ortho_rays(64, 64, 4, "cuda", seed=1, origin=(1.2, 0.3, 1.2), target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0))
        yield ("sine96", hf.Heightfield(heightfield=hf.workload.sine_heights(96, 96, device="cuda"), max_height=0.5), rays,
               cu(LS.lights(2, LS.IDENTITY, False)))

    def sub(si, ray, m, sh_n=None, requires_grad=False):
        s = hf.SurfaceInteraction3f()
        cut = lambda x: x.detach()[..., :m].contiguous()
        s.p, s.n, s.t = cut(si.p), cut(si.n), cut(si.t)
        s.sh_frame = hf.Frame3f(None, None, cut(si.sh_frame.n).requires_grad_(requires_grad) if sh_n is None else sh_n)
        return s, hf.Ray3f(cut(ray.o), cut(ray.d))

    def api_row(tag, call, si, ray, m, spp, inp, weighted, env_of=None):
        """a row through the Python API: forward, backward (autograd) and jvp (forward AD).  call(si, ray, weight, env)
        returns (image, *records); env_of(data): the Envmap of the rows that have one"""
        data0 = dat[:, :-1].contiguous()
        s, r = sub(si, ray, m, requires_grad=True)
        wt = cu(inp["weight"]).requires_grad_(True) if weighted else None
        env = env_of(data0.clone().requires_grad_(True)) if env_of else None
        img, *rec = call(s, r, wt, env)
        R[f"{tag}/image" + (".atomic" if spp in ATOMIC_SPP else "")] = npy(img)
        for j, x in enumerate(rec):
            R[f"{tag}/record{j}"] = npy(x)
        (img * cu(_gimg(tag, tuple(img.shape)))).sum().backward()
        R[f"{tag}/grad_sh_n"] = npy(s.sh_frame.n.grad)
        if weighted:
            R[f"{tag}/grad_weight"] = npy(wt.grad)
        if env:
            R[f"{tag}/grad_data.atomic"] = npy(env.data.grad)
        with fwAD.dual_level():
            s2, r2 = sub(si, ray, m)
            s2.sh_frame.n = fwAD.make_dual(s2.sh_frame.n, cu(inp["dn"]))
            wd = fwAD.make_dual(cu(inp["weight"]), cu(inp["dw"])) if weighted else None
            env2 = env_of(fwAD.make_dual(data0, cu(inp["ddata"][:, :-1]))) if env_of else None
            out = call(s2, r2, wd, env2)
            R[f"{tag}/tangent_image"] = npy(fwAD.unpack_dual(out[0]).tangent)

    def abi_row(tag, row, shape, si, ray, m, spp, inp, weighted):
        """reflect (row = 'reflect') or glossy through the C ABI: forward with `active`, then `active`, `value` and the
        image NULL in turn; the adjoint and the tangent on the first forward's visibility, the tangent without its image too"""
        cut = lambda x: x.detach()[..., :m].contiguous()
        p, nr, sn, d, t = cut(si.p), cut(si.n), cut(si.sh_frame.n), cut(ray.d), cut(si.t)
        glossy = row == "glossy"
        wt = cu(inp["weight"]) if weighted else None
        act, al = cu(inp["active"]), torch.full((m,), ALPHA, device="cuda")
        vdt = torch.int32 if glossy else torch.uint8
        rot = (C.c_float * 9)(*[float(v) for v in E.DEFAULT_ROT.reshape(-1)])

        def mid(active):
            lob = (al.data_ptr(), ETA, LS.K, LS.SEED, None) if glossy else (ETA,)
            return (ptr(active), ptr(wt), *lob, W, H, dat.data_ptr(), C.byref(rot))
        fwd_entry = lib.hf_glossy_lighting if glossy else lib.hf_reflect_lighting

        def forward(sfx, active, want_image=True, want_value=True):
            img = torch.empty(m // spp, device="cuda") if want_image else None
            val = torch.empty(m, device="cuda") if want_value else None
            vis = torch.empty(m, dtype=vdt, device="cuda")
            check(fwd_entry(shape._h, m, spp, rows(p), rows(nr), rows(sn), rows(d), t.data_ptr(), *mid(active), ptr(img), ptr(val),
                            vis.data_ptr(), stream()))
            if want_image:
                R[f"{tag}/{sfx}image" + (".atomic" if spp in ATOMIC_SPP else "")] = npy(img)
            if want_value:
                R[f"{tag}/{sfx}value"] = npy(val)
            R[f"{tag}/{sfx}vis"] = npy(vis)
            return vis
        vis = forward("", act)
        forward("no_active/", None)
        forward("no_value/", act, want_value=False)
        forward("no_image/", act, want_image=False)
        head = (m, spp, rows(sn), rows(d), t.data_ptr(), *mid(act), vis.data_ptr())
        gi, gv = cu(_gimg(tag, (m // spp,))), cu(inp["gvalue"])
        gn, gw, ga, gd = torch.empty((3, m), device="cuda"), torch.empty(m, device="cuda"), torch.empty(m, device="cuda"), torch.zeros((H, W), device="cuda")
        if glossy:
            check(lib.hf_glossy_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(gn), ptr(gw if weighted else None),
                                                 ga.data_ptr(), gd.data_ptr(), stream()))
            R[f"{tag}/grad_alpha"] = npy(ga)
        else:
            check(lib.hf_reflect_lighting_adjoint(*head, gi.data_ptr(), gv.data_ptr(), rows(gn), ptr(gw if weighted else None),
                                                  gd.data_ptr(), stream()))
        R[f"{tag}/grad_sh_n"] = npy(gn)
        if weighted:
            R[f"{tag}/grad_weight"] = npy(gw)
        R[f"{tag}/grad_data.atomic"] = npy(gd)
        dn, dw, da, dda = cu(inp["dn"]), cu(inp["dw"]) if weighted else None, cu(inp["da"]), cu(inp["ddata"])
        tan_in = (rows(dn), ptr(dw), da.data_ptr(), dda.data_ptr()) if glossy else (rows(dn), ptr(dw), dda.data_ptr())
        tan_entry = lib.hf_glossy_lighting_tangent if glossy else lib.hf_reflect_lighting_tangent
        for sfx, want_image in (("", True), ("no_image/", False)):
            dimg = torch.empty(m // spp, device="cuda") if want_image else None
            dval = torch.empty(m, device="cuda")
            check(tan_entry(*head, *tan_in, ptr(dimg), dval.data_ptr(), stream()))
            if want_image:
                R[f"{tag}/tangent_image"] = npy(dimg)
            R[f"{tag}/{sfx}tangent_value"] = npy(dval)

    def rays7(r):
        return npy(torch.cat([r.o, r.d, r.maxt[None]]))
    env_of = lambda data: hf.Envmap(data, defensive=DEFENSIVE)
    for name, shape, rt, lights in scenes():
        ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
        si = shape.ray_intersect(ray, hf.RayFlags.All)
        n = len(ray)
        R[f"{name}/rows/sh_n"], R[f"{name}/rows/d"], R[f"{name}/rows/t"] = npy(si.sh_frame.n), npy(ray.d), npy(si.t)
        env = env_of(dat[:, :-1].contiguous())
        R[f"{name}/table"] = npy(env.table())
        for k in range(2):                                   # the materialised rays of every row
            R[f"{name}/sky/rays{k}"] = rays7(hf.sky_rays(si, ray, k, seed=LS.SEED))
            R[f"{name}/bounce/rays{k}"] = rays7(hf.bounce_rays(shape, si, ray, k, seed=LS.SEED))
            r, wgt = hf.envmap_rays(si, ray, env, k, seed=LS.SEED, return_weight=True)
            R[f"{name}/envmap/rays{k}"], R[f"{name}/envmap/rays{k}_weight"] = rays7(r), npy(wgt)
            r, h = hf.glossy_rays(si, ray, ALPHA, k, seed=LS.SEED, active=cu(_inputs(name, n)["active"]).bool(), return_normal=True)
            R[f"{name}/glossy/rays{k}"], R[f"{name}/glossy/rays{k}_h"] = rays7(r), npy(h)
        R[f"{name}/reflect/rays"] = rays7(hf.reflection_rays(si, ray))
        R[f"{name}/reflect/rays_active"] = rays7(hf.reflection_rays(si, ray, active=cu(_inputs(name, n)["active"]).bool()))
        for spp in SPPS:
            m = n - n % spp
            for weighted in (False, True):
                case = f"spp{spp}" + ("w" if weighted else "")
                inp = _inputs(f"{name}/{case}", m, (H, W))
                common = dict(spp=spp, num_rays=LS.K, seed=LS.SEED)
                api_row(f"{name}/sky/{case}", lambda s, r, w, e: hf.sky_lighting(shape, s, r, radiance=1.3, albedo=ALBEDO, weight=w,
                                                                                  return_visibility=True, **common), si, ray, m, spp, inp, weighted)
                api_row(f"{name}/bounce/{case}", lambda s, r, w, e: hf.bounce_lighting(shape, s, r, lights, albedo=ALBEDO, weight=w,
                                                                                        return_records=True, **common), si, ray, m, spp, inp, weighted)
                api_row(f"{name}/envmap/{case}", lambda s, r, w, e: hf.envmap_lighting(shape, s, r, e, albedo=ALBEDO, weight=w,
                                                                                        return_visibility=True, **common), si, ray, m, spp, inp, weighted, env_of)
                abi_row(f"{name}/reflect/{case}", "reflect", shape, si, ray, m, spp, inp, weighted)
                abi_row(f"{name}/glossy/{case}", "glossy", shape, si, ray, m, spp, inp, weighted)
        torch.cuda.synchronize()
        print("dumped", name, flush=True)
    # hf_envmap_eval and its adjoint: seeded directions, both poles and the seam among them
    d, act, go = _eval_inputs(W)
    envg = env_of(dat[:, :-1].contiguous().requires_grad_(True))
    val = envg.eval(cu(d), active=cu(act))
    R["eval/value"] = npy(val)
    (val * cu(go)).sum().backward()
    R["eval/grad_data.atomic"] = npy(envg.data.grad)
    torch.cuda.synchronize()
    np.savez_compressed(out, **R)
    print("wrote", out, len(R), "arrays", flush=True)


def _eval_inputs(W):
    rng = np.random.default_rng(2)
    v = rng.normal(size=(3, 8192))
    v /= np.linalg.norm(v, axis=0)
    v[:, 0], v[:, 1] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)                        # the poles of the default rotation (+Y -> +Z)
    v[:, 2] = (np.sin(np.pi / (W - 1)), -np.cos(np.pi / (W - 1)), 0.0)        # on the seam
    return v.astype(np.float32), rng.uniform(size=8192) < 0.9, rng.normal(size=8192).astype(np.float32)


# ---- the parent: the comparison -----------------------------------------------------------------------------------------
def _fold(x):
    return np.concatenate([x[:, :1] + x[:, -1:], x[:, 1:-1]], 1)


def compare(out):
    import envmap_ref as E
    import lighting_scenes as LS
    import sky_ref as S
    import test_gpu_glossy as TG
    import test_gpu_reflect as TR
    old, new = np.load(os.path.join(out, "old.npz")), np.load(os.path.join(out, "new.npz"))
    lines, ok = [], True
    if sorted(old.files) != sorted(new.files):
        lines.append("the two libraries wrote different sets of outputs"); ok = False
    full = E.MAPS[MAP]()
    H, W = full.shape
    exact = [k for k in old.files if not k.endswith(".atomic") and k in new.files]
    words = bad = 0
    for k in sorted(exact):
        a, b = old[k], new[k]
        same = a.shape == b.shape and a.dtype == b.dtype
        diff = int((a.view(np.uint8) != b.view(np.uint8)).reshape(-1, a.itemsize).any(1).sum()) if same else a.size
        words += a.size; bad += diff
        if diff:
            lines.append(f"{k:64s} {a.size:8d} values, {diff:6d} differ bitwise: FAIL"); ok = False
    head = (f"Outputs computed without float atomics: {len(exact)} arrays, {words} words compared, {bad} differ bitwise.")
    drs = {}
    for k in sorted(set(old.files) - set(exact)):
        if k not in new.files:
            continue
        a, b = old[k].astype(np.float64), new[k].astype(np.float64)
        diff, nbits = np.abs(a - b), int((old[k].view(np.uint32) != new[k].view(np.uint32)).sum())
        parts = k.split("/")
        what = parts[-1][:-len(".atomic")]
        if parts[0] == "eval":
            d, act, go = _eval_inputs(W)
            _, cnt, ab = E.eval_adjoint(d.astype(np.float64), (H, W), go, E.DEFAULT_ROT, act)
            bound, rule = (_fold(cnt) + 5) * 2.0 ** -24 * _fold(ab), "per texel (m + 5) 2^-24 sum |terms|"
            good = bool(np.all(diff <= bound))
        elif what == "image" and parts[1] in ("sky", "bounce"):
            bound, rule = 1e-5 * np.abs(a) + 1e-7, "1e-5 |value| + 1e-7"
            good = bool(np.all(diff <= bound))
        elif what == "image" and parts[1] in ("reflect", "glossy"):
            bound, rule = 2.5e-7 * np.abs(a).max(), "2.5e-7 max |value|"
            good = bool(np.all(diff <= bound))
        elif parts[1] == "envmap":
            scene, case = parts[0], parts[2]
            weighted, spp = case.endswith("w"), int(case[3:].rstrip("w"))
            arrs = [old[f"{scene}/rows/{r}"] for r in ("sh_n", "d", "t")]
            n = arrs[2].shape[0]
            m = n - n % spp
            if scene not in drs:
                drs[scene] = E.draws(full, old[f"{scene}/table"], np.arange(n), LS.K, LS.SEED, E.DEFAULT_ROT)
            dr = {key: v[..., :m] for key, v in drs[scene].items()}
            arrs = [x[..., :m] for x in arrs]
            wgt = _inputs(f"{scene}/{case}", m, (H, W))["weight"] if weighted else None
            bits = S.unpack(old[f"{scene}/envmap/{case}/record0"], LS.K)
            if what == "image":
                _, _, S_ = E.forward(*arrs, wgt, bits, dr, ALBEDO, spp)
                bound, rule = 1e-5 * np.abs(a) + 1e-7 * S_, "1e-5 |value| + 1e-7 S"
            else:
                gi = _gimg(f"{scene}/envmap/{case}", (m // spp,))
                _, _, _, cnt, ab = E.adjoint(*arrs, wgt, bits, dr, ALBEDO, spp, gi, (H, W))
                bound, rule = (_fold(cnt) + 5) * 2.0 ** -24 * _fold(ab), "per texel (m + 5) 2^-24 sum |terms|"
            good = bool(np.all(diff <= bound))
        else:                                                # grad_data of reflect and glossy: the tests' relative L2
            tol = (TG if parts[1] == "glossy" else TR).TOL["grad_data"]
            rel = float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-300))
            good, rule = rel <= tol, f"relative L2 {rel:.3e} <= {tol:.1e}"
        ok &= good
        lines.append(f"{k:64s} {a.size:8d} values, {nbits:6d} differ bitwise, max abs diff {diff.max():.3e} "
                     f"(max |value| {np.abs(a).max():.3e}); {rule}: {'within bound' if good else 'OUT OF BOUND'}")
    ok &= bad == 0
    text = "\n".join([head, "", "Outputs accumulated with float atomics (|old - new| against the bound of the row's GPU test):"] + lines +
                     ["", "RESULT: " + ("PASS" if ok else "FAIL")])
    print(text)
    open(os.path.join(out, "ab_outputs.txt"), "w").write(text + "\n")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ab_reflection_rows"))
    ap.add_argument("--compare-only", action="store_true")
    ap.add_argument("--dump", help=argparse.SUPPRESS)        # the child: which of old / new
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.dump:
        return dump(a.old if a.dump == "old" else a.new, os.path.join(a.out, a.dump + ".npz"))
    if not a.compare_only:
        for which in ("old", "new"):                         # one process each; a fault, abort or time limit stops the call
            rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), a.old, a.new, "--out", a.out,
                                  "--dump", which], cwd=ROOT)
            if rc != 0:
                sys.exit(f"the {which} library's run ended with status {rc}: stopping")
    sys.exit(0 if compare(a.out) else 1)


if __name__ == "__main__":
    main()

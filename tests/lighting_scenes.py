"""The scenes of tests/test_lighting_scenes.py (CPU) and tests/test_gpu_lighting_scenes.py (GPU): sky and bounce lighting
under a constant affine to_world, flip_normals, 1..8 lights and rectangular grids, and the helpers the lighting tests
share (_close, _rows7, _records).  A helper module, not a conftest: nothing here is a fixture.

Every scene is a 25 x 23 x 4 orthographic wavefront (2300 samples: neither a multiple of 64 nor of 256, so the last wave
and the last workgroup are partial) drawn in object space, mapped to world with the scene's to_world, K = 4 directions
per sample, seed 5.  Lights: azimuth 0.3 + 2 pi l / L, elevation linspace(0.12, 0.55, L) rad (L = 1: 0.4) in object
space (z negated for a view from below), carried to world as a covector (inverse transpose of the linear part) and
normalised; irradiance linspace(1.0, 0.4, L).

cpu_model() runs a scene with the oracle and the float64 restatements alone (tests/sky_ref.py, tests/bounce_ref.py) and
returns the shares that make the scene a test: how many samples are eligible, how many bounce rays hit, how many lights
reach a hit, how many lanes a rounding decides.

smooth_normals() and bent_normals() give a scene shading normals that are not its geometric normals, and normals_model()
counts, again with the oracle and the restatements alone, the decisions that then separate the two (tests/
test_lighting_normals.py on the CPU, tests/test_gpu_lighting_normals.py on the GPU)."""
import types

import numpy as np

import bounce_ref as B
import common
import sky_ref as S

K, SEED = 4, 5
FILM = (25, 23, 4)
N = FILM[0] * FILM[1] * FILM[2]
SPLIT = 1148           # a pixel boundary (287 * 4) that is 60 mod 64: where the chunked tests cut the wavefront
# a mask is decided by the sign of a float32 quantity that is within 2e-6 of the restatement's: a lane whose margin is
# below this is decided by rounding and is left out of mask comparisons
MARGIN = 4e-6
MISS = 0xFFFFFFFF
IDENTITY = np.eye(4)[:3].astype(np.float32)

#            field (kind, W, H)   max_height  to_world               flip   below  L
SCENES = {
    "affine":      (("sine", 40, 25), 0.4, lambda: common.affine(4),      False, False, 8),
    "mirror_flip": (("sine", 33, 17), 0.6, lambda: common.mirror_shear(), True,  False, 3),   # mirror and flip together leave the normal up
    "flip_below":  (("sine", 40, 25), 0.4, lambda: common.affine(4),      True,  True,  1),
    "rand8":       (("rand", 17, 9),  0.5, lambda: IDENTITY.copy(),       False, False, 8),   # a light-count failure without a transform
}
NAMES = tuple(SCENES)


def lights(L, to_world, below):
    """[L, 4] float32: unit world direction towards the light, irradiance"""
    az = 0.3 + 2.0 * np.pi * np.arange(L) / L
    el = np.linspace(0.12, 0.55, L) if L > 1 else np.array([0.4])
    obj = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * (-1.0 if below else 1.0)])
    A = np.asarray(to_world, np.float64).reshape(3, 4)[:, :3]
    world = np.linalg.inv(A).T @ obj
    world /= np.linalg.norm(world, axis=0)
    return np.concatenate([world.T, np.linspace(1.0, 0.4, L)[:, None]], 1).astype(np.float32)


def wavefront(to_world, below):
    """[7, N] float32 world rays: unit directions, maxt = inf"""
    from hf_amd import workload
    r = workload.ortho_rays(*FILM, "cpu", seed=1, origin=(0.6, 0.35, -2.0 if below else 2.0), target=(0.0, 0.0, 0.2),
                            scale=(0.9, 0.9, 1.0)).numpy()
    r = common.to_world_rays(r, to_world).astype(np.float64)
    r[3:6] /= np.linalg.norm(r[3:6], axis=0)
    r[6] = np.inf
    return r.astype(np.float32)


def scene(name):
    (kind, W, H), max_height, tw, flip, below, L = SCENES[name]
    sc = types.SimpleNamespace(name=name, W=W, H=H, max_height=max_height, to_world=tw(), flip=flip, below=below, L=L)
    sc.h = common.heights(kind, W, H, np.random.default_rng(17))
    sc.h64 = sc.h.astype(np.float64)
    sc.lights = lights(L, sc.to_world, below)
    sc.rays = wavefront(sc.to_world, below)
    sc.n = sc.rays.shape[1]
    assert sc.n == N and sc.h.shape == (H, W)
    return sc


def oracle_field(sc, oracle):
    return oracle.OracleField(sc.h, max_height=sc.max_height, to_world=sc.to_world, flip_normals=sc.flip)


def normals_of(sc, prim, hit):
    """[3, n] float64: B.face_normal of the scene for the records `prim` where `hit` (elsewhere that of triangle 0)"""
    return B.face_normal(sc.h64, np.where(hit, np.asarray(prim).view(np.uint32), 0), sc.max_height, sc.flip, sc.to_world)


def _rays7(o, d):
    return np.concatenate([o, d, np.full((1, o.shape[1]), np.inf)]).astype(np.float32)


def cpu_model(sc, oracle):
    """the scene through the oracle and the restatements only; a namespace of records and of the shares the scene
    conditions are about"""
    f = oracle_field(sc, oracle)
    r = sc.rays
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)
    p, gn, sh_n, d = (x.astype(np.float64) for x in (rec["p"], rec["n"], rec["sh_n"], r[3:6]))
    ids = np.arange(sc.n)
    m = types.SimpleNamespace(field=f, t=t, prim=prim, p=p, n=gn, sh_n=sh_n)
    m.eligible, _ = S.eligible(sh_n, d, t)
    coords = [np.abs(r[0:3]).max(), np.abs(p).max()]
    undecided = total = 0
    # ---- the bounce row
    w, z = B.directions(sh_n, ids, K, SEED)
    traced = B.traced(sh_n, d, t, z)
    undecided += int((m.eligible[None] & (z <= MARGIN)).sum()); total += K * sc.n
    m.hit = np.zeros((K, sc.n), bool); m.hit_prim = np.full((K, sc.n), MISS, np.uint32)
    m.lit = np.zeros((K, sc.L, sc.n), bool); m.shadow = np.zeros((K, sc.L, sc.n), bool)
    m.nq = np.zeros((K, 3, sc.n)); m.nq_oracle = np.zeros((K, 3, sc.n))
    for k in range(K):
        tr = np.flatnonzero(traced[k])
        rk = _rays7(B.spawn_origin(p, gn, w[k])[:, tr], w[k][:, tr])
        t2, u2, v2, prim2 = f.ray_intersect_preliminary(rk)
        rec2 = f.compute_surface_interaction(rk, t2, u2, v2, prim2, oracle.RAY_ALL)
        hit = np.isfinite(t2)
        at = tr[hit]
        m.hit[k, at] = True; m.hit_prim[k, at] = prim2[hit]
        m.nq[k] = normals_of(sc, m.hit_prim[k], m.hit[k])
        m.nq_oracle[k][:, at] = rec2["n"][:, hit]
        q = np.zeros((3, sc.n)); q[:, at] = rec2["p"][:, hit]
        coords += [np.abs(rk[0:3]).max(), np.abs(q).max()]
        cw = (m.nq[k] * w[k]).sum(0)
        front = m.hit[k] & (-cw > 0)
        want, margin = B.shadow_traced(front[None], m.nq[k][None], sc.lights)
        for l in range(sc.L):
            undecided += int((m.hit[k] & ((np.abs(cw) <= MARGIN) | (margin[0, l] <= MARGIN))).sum()); total += sc.n
            st = np.flatnonzero(want[0, l])
            ll = np.broadcast_to(sc.lights[l, :3, None].astype(np.float64), (3, len(st)))
            rs = _rays7(B.spawn_origin(q[:, st], m.nq[k][:, st], ll), ll)
            coords.append(np.abs(rs[0:3]).max())
            m.shadow[k, l, st] = True
            m.lit[k, l, st] = ~f.ray_test(rs).astype(bool)
    # ---- the sky row
    ws = S.directions(ids, K, SEED)
    straced, smargin = S.traced(sh_n, d, t, ws)
    undecided += int((m.eligible[None] & (smargin <= MARGIN)).sum()); total += K * sc.n
    m.vis = np.zeros((K, sc.n), bool)
    for k in range(K):
        tr = np.flatnonzero(straced[k])
        rk = _rays7(S.spawn_origin(p, gn, ws[k])[:, tr], ws[k][:, tr])
        coords.append(np.abs(rk[0:3]).max())
        m.vis[k, tr] = ~f.ray_test(rk).astype(bool)
    m.shares = {"eligible": float(m.eligible.mean()), "bounce_hit": m.hit.sum() / traced.sum(),
                "sky_unoccluded": m.vis.sum() / straced.sum(),
                "lit": m.lit.sum((0, 2)) / np.maximum(m.shadow.sum((0, 2)), 1), "lit_records": m.lit.sum((0, 2)),
                "undecided": undecided / total, "max_coordinate": float(max(coords))}
    return m


# ---- shading normals that are not the geometric normal (tests/test_lighting_normals.py, test_gpu_lighting_normals.py) -----
KINDS = ("smooth", "bent")
ENV_SCENES = ("affine", "mirror_flip", "rand8")            # the scenes and maps of the envmap row's draws
ENV_MAPS = (("sun", 0.25), ("gradient", 0.0))
BEND = 0.5                                                 # tan of the angle between `bent` and n: 26.6 degrees


def smooth_normals(sc, rays, prim, hit):
    """[3, n] float64: sh_n of smooth_ref.surface(mode="default") (the blended vertex normals, face_normals = false) at
    the triangles `prim` of the hits; zero on misses, as the record is"""
    import torch
    import smooth_ref
    at = np.flatnonzero(hit)
    r64 = torch.from_numpy(np.asarray(rays, np.float64)[:, at])
    ref = smooth_ref.surface(torch.from_numpy(sc.h64), sc.max_height, torch.from_numpy(np.asarray(sc.to_world, np.float64)),
                             sc.flip, r64[0:3].T.contiguous(), r64[3:6].T.contiguous(),
                             torch.from_numpy(np.asarray(prim).view(np.uint32)[at].astype(np.int64)), None, "default")
    out = np.zeros((3, len(hit)))
    out[:, at] = ref["sh_n"].numpy().T
    return out


def bent_normals(n, hit):
    """[3, n] float32: normalize(n + BEND tau), tau the default_rng(3) normal draw projected off n and normalised: BEND
    is the tangent of the angle to n on every hit; misses keep n"""
    n64 = np.asarray(n, np.float64)
    tau = np.random.default_rng(3).normal(size=n64.shape)
    tau -= n64 * (n64 * tau).sum(0)
    tau /= np.linalg.norm(tau, axis=0)
    b = n64 + BEND * tau
    b /= np.linalg.norm(b, axis=0)
    return np.where(np.asarray(hit, bool)[None], b.astype(np.float32), np.asarray(n, np.float32))


def below_counts(sh_n, gn, d, t, w, valid=None):
    """what separates the two normals among the decisions of a sky-like row (directions w [K, 3, n], `valid` [K, n] draws):
    (traced [K, n] by sh_n, <gn, w> [K, n], lanes traced with <gn, w> < -MARGIN, lanes of eligible samples with a valid draw
    that are NOT traced although <gn, w> > MARGIN)"""
    el, _ = S.eligible(sh_n, d, t)
    ok = el[None] if valid is None else el[None] & valid
    co = np.einsum("cn,kcn->kn", np.asarray(sh_n, np.float64), w)
    cg = np.einsum("cn,kcn->kn", np.asarray(gn, np.float64), w)
    traced = ok & (co > 0)
    return traced, cg, traced & (cg < -MARGIN), ok & ~traced & (cg > MARGIN)


def normals_model(sc, oracle, kind, maps=()):
    """the scene with the shading normals `kind` through the oracle and the restatements only (sky_ref, bounce_ref,
    envmap_ref, smooth_ref): the populations that make (scene, kind) a test of WHICH normal a kernel uses.  Returns
    (counts of the sky and bounce rows, {(map, u): counts of the envmap row})"""
    import envmap_ref as E
    f = oracle_field(sc, oracle)
    r = sc.rays
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)
    hit = np.isfinite(t)
    p, gn, d = (x.astype(np.float64) for x in (rec["p"], rec["n"], r[3:6]))
    sh_n = smooth_normals(sc, r, prim, hit) if kind == "smooth" else bent_normals(rec["n"], hit).astype(np.float64)
    ids = np.arange(sc.n)
    el, elm = S.eligible(sh_n, d, t)
    el_n, _ = S.eligible(gn, d, t)
    angle = np.degrees(np.arccos(np.clip((sh_n * gn).sum(0)[hit], -1, 1)))
    common_ = {"hits": int(hit.sum()), "eligible": int(el.sum()), "eligibility_differs": int((el != el_n).sum()),
               "angle_deg": (float(angle.min()), float(np.median(angle)), float(angle.max())), "max_p": float(np.abs(p).max())}

    def shadow_row(w, valid, margin):
        """the counts of a row whose rays are shadow rays: sky, envmap"""
        traced, cg, below, above = below_counts(sh_n, gn, d, t, w, valid)
        seen = np.zeros(traced.shape, bool)
        for k in range(K):
            tr = np.flatnonzero(traced[k])
            seen[k, tr] = ~f.ray_test(_rays7(S.spawn_origin(p, gn, w[k])[:, tr], w[k][:, tr])).astype(bool)
        ok = hit[None] if valid is None else hit[None] & valid
        undecided = (ok & (elm[None] <= MARGIN)) | (el[None] & ok & ((margin <= MARGIN) | (np.abs(cg) <= MARGIN)))
        return {"traced": int(traced.sum()), "traced_below": int(below.sum()), "below_unoccluded": int((below & seen).sum()),
                "below_occluded": int((below & ~seen).sum()), "above_untraced": int(above.sum()),
                "undecided": float(undecided.mean())}

    # ---- the sky row
    ws = S.directions(ids, K, SEED)
    sky = shadow_row(ws, None, S.traced(sh_n, d, t, ws)[1])
    # ---- the bounce row
    w, z = B.directions(sh_n, ids, K, SEED)
    traced = B.traced(sh_n, d, t, z)
    cg = np.einsum("cn,kcn->kn", gn, w)
    below = traced & (cg < -MARGIN)
    bhit = np.zeros(traced.shape, bool); back = np.zeros(traced.shape, bool)
    for k in range(K):
        tr = np.flatnonzero(traced[k])
        t2, _, _, prim2 = f.ray_intersect_preliminary(_rays7(B.spawn_origin(p, gn, w[k])[:, tr], w[k][:, tr]))
        bhit[k, tr] = np.isfinite(t2)
        hp = np.full(sc.n, MISS, np.uint32); hp[tr[np.isfinite(t2)]] = prim2[np.isfinite(t2)]
        back[k] = bhit[k] & ((normals_of(sc, hp, bhit[k]) * w[k]).sum(0) > MARGIN)
    undecided = (hit[None] & (elm[None] <= MARGIN)) | (el[None] & ((z <= MARGIN) | (np.abs(cg) <= MARGIN)))
    bounce = {"traced": int(traced.sum()), "traced_below": int(below.sum()), "below_hit": int((below & bhit).sum()),
              "hit_from_behind": int(back.sum()), "undecided": float(undecided.mean())}
    # ---- the envmap row
    env = {}
    for name, u_ in maps:
        data = E.MAPS[name]()
        dr = E.draws(data, E.build_table(data, u_), ids, K, SEED, E.DEFAULT_ROT)
        env[(name, u_)] = shadow_row(dr["w"], dr["valid"], E.traced(sh_n, d, t, dr)[1])
    return types.SimpleNamespace(sh_n=sh_n, n=gn, common=common_, sky=sky, bounce=bounce, env=env)


# the floors of tests/test_lighting_normals.py, which the GPU tests hold their own populations to
FLOOR_BELOW, FLOOR_ABOVE, FLOOR_OUTCOME, FLOOR_BOUNCE_HIT, FLOOR_ELIGIBILITY, FLOOR_BEHIND = 200, 100, 10, 100, 40, 100


# ---- what the GPU lighting tests share ---------------------------------------------------------------------------------
def _np(x):
    return x.detach().cpu().numpy()


def _rows7(r):
    import torch
    return _np(torch.cat([r.o, r.d, r.maxt[None]]))


def _records(prim, lit, L):
    return B.unpack(_np(prim), _np(lit), L)


def _close(got, ref, absum, num_rays):
    """the derived bound: 1e-5 |ref| + 1e-7 + K 2^-24 sum |terms| (a float32 accumulation of K terms errs by no more)"""
    err = np.abs(got - ref)
    bound = 1e-5 * np.abs(ref) + 1e-7 + num_rays * 2.0 ** -24 * absum
    print("   max |ref|", np.abs(ref).max(), "max err", err.max(), "max err / bound", (err / bound).max())
    return bool(np.all(err <= bound))

"""The scenes of tests/test_row_scenes.py (CPU) and tests/test_gpu_row_scenes.py (GPU): the lighting rows that came after
the environment map, under a constant affine to_world, flip_normals, a view from below and rectangular grids that are no
power of two.  A helper module, not a conftest: nothing here is a fixture.

Scenes: `affine`, `mirror_flip` and `flip_below` of tests/lighting_scenes.py (sine fields of 40 x 25, 33 x 17 and 40 x 25
under common.affine(4), common.mirror_shear() + flip_normals, affine + flip_normals seen from below), built by
lighting_scenes.scene: its 25 x 23 x 4 film (2300 samples: the last wave and the last workgroup are partial).  Two
wavefronts per scene, drawn in object space and carried to world as lighting_scenes.wavefront does: `steep`, from
(0.6, 0.35, +-2.0), and `oblique`, from (1.2, 0.3, +-1.2), both towards (0, 0, 0.2); the minus signs are the view from below.

Emitters are defined once in OBJECT space, from each row's own rig (directional_ref.RIG, spot_ref.RIG), and carried to
world: points through to_world, vectors through its linear part, z negated first for the view from below, a spot light's
pose as the rigid look_at of the carried origin and target (the carried `up` only picks the roll).  On a scene whose world
is not its object space a kernel that took an object-space p or n for a world-space one gives other numbers.

Rows: `directional` (rays with maxt = inf, the steep view), `spot` (rays that END at the emitter, the steep view) and
`caustic` (rays that END at the receiver, the oblique view), `rect` (rays that END on the lamp, the steep view) and
`projector` (rays that END at the projector, the steep view) and `reflect` (rays with maxt = inf whose direction and masks
depend on the view, the oblique view), `refract` (the caustic row's rays onto a textured receiver) and `glossy` (4 mirror
rays per sample about drawn microfacet normals, the oblique view); the sections of the last six are at the end of this
file.  All eight rows that came after the environment map are here, and the two that came after the normal map:
`specular` (the directional row's byte, masks and cosines from sh_n and -d, the steep view) and `medium` (shadow rays that
START in free space, on the primary ray, under a world-space top plane; the steep view and, for the medium that holds the
camera, the oblique one): ten rows, the last two sections of this file.  The
spot rig here is spot_ref.RIG without `above` -- on `affine` it put the union of the samples that rounding may decide over
row_helpers.UNSURE_CAP -- and with `inside` in its place: a point-like cone whose origin lies INSIDE the field's object-space
bounding box, over the lowest vertex of the field, so that shadow rays end inside the bound: replacing their maxt by +inf
changes the oracle's answer, which is what catches a wrong ray end under the transform.

model() runs a (row, scene, mode) with the oracle and the float64 restatements alone and returns the records, the
visibility and the shares that make the triple a test; conditions() asserts them (on the CPU for the oracle's records, on
the GPU for the GPU's own)."""
import types

import numpy as np

import directional_ref as D
import lighting_scenes as LS
import spot_ref as P
from row_helpers import UNSURE_CAP
from sensor_ref import look_at

SCENES = ("affine", "mirror_flip", "flip_below")
TARGET = (0.0, 0.0, 0.2)
VIEWS = {"steep": (0.6, 0.35, 2.0), "oblique": (1.2, 0.3, 1.2)}
# (scene, face_normals): both shading modes on `affine`; smooth normals under flip_normals are held against smooth_ref by
# tests/test_gpu_smooth_shading.py and tests/test_gpu_lighting_normals.py
CASES = (("affine", True), ("affine", False), ("mirror_flip", True), ("flip_below", True))
ROWS = ("directional", "spot")
VIEW_OF = {"directional": "steep", "spot": "steep"}
SPP = LS.FILM[2]
SPOT_NAMES = ("inside",) + tuple(k for k in P.NAMES if k != "above")
# the scenes on which the chain row -> loss -> backward() -> dL/dheight is checked: (scene, face_normals)
CHAINS = (("mirror_flip", True), ("affine", False))


def wavefront(sc, view):
    """[7, N] float32 world rays of the view `view`.  lighting_scenes.wavefront has its origin written into it and, being
    part of the existing tests, stays as it is; this is its body with the origin as a parameter, and scene() asserts that
    for `steep` it gives that function's rays bit for bit, so the two cannot drift apart"""
    from hf_amd import workload
    import common
    o = VIEWS[view]
    r = workload.ortho_rays(*LS.FILM, "cpu", seed=1, origin=(o[0], o[1], -o[2] if sc.below else o[2]), target=TARGET,
                            scale=(0.9, 0.9, 1.0)).numpy()
    r = common.to_world_rays(r, sc.to_world).astype(np.float64)
    r[3:6] /= np.linalg.norm(r[3:6], axis=0)
    r[6] = np.inf
    return r.astype(np.float32)


def scene(name, view):
    sc = LS.scene(name)
    if view == "steep":
        assert np.array_equal(sc.rays, wavefront(sc, "steep"))           # (the scene's own wavefront IS the steep one)
    else:
        sc.rays = wavefront(sc, view)
    sc.view = view
    return sc


# ---- object space -> world --------------------------------------------------------------------------------------------
def _obj(sc, x):
    x = np.array(x, np.float64).reshape(3)
    if sc.below:
        x[2] = -x[2]
    return x


def vector(sc, v):
    return np.asarray(sc.to_world, np.float64)[:, :3] @ _obj(sc, v)


def point(sc, x):
    return vector(sc, x) + np.asarray(sc.to_world, np.float64)[:, 3]


def pose(sc, origin, target, up):
    """[3, 4]: the rigid look_at of the carried origin and target"""
    return look_at(point(sc, origin), point(sc, target), vector(sc, up))[:3]


def extreme_vertex(sc):
    """object-space (x, y, z) of the lowest vertex that is not on the border (the highest for the view from below): the
    field spans [-1, 1]^2 x [0, max_height]"""
    inner = sc.h64[1:-1, 1:-1]
    j, i = np.unravel_index(np.argmax(inner) if sc.below else np.argmin(inner), inner.shape)
    return (2.0 * (i + 1) / (sc.W - 1) - 1.0, 2.0 * (j + 1) / (sc.H - 1) - 1.0, float(inner[j, i]) * sc.max_height)


INSIDE_Z = 0.6


def inside_pose(sc):
    """the pose of the spot light `inside`: its origin over the lowest inner vertex at INSIDE_Z max_height (under the highest
    one at (1 - INSIDE_Z) max_height for the view from below), inside the box on every scene, looking along the object z
    axis at the surface.  Object coordinates as they are: nothing is negated here"""
    x, y, _ = extreme_vertex(sc)
    A = np.asarray(sc.to_world, np.float64)
    w = lambda q: A[:, :3] @ np.asarray(q, np.float64) + A[:, 3]
    z = (1.0 - INSIDE_Z if sc.below else INSIDE_Z) * sc.max_height
    return look_at(w((x, y, z)), w((x, y, sc.max_height if sc.below else 0.0)), A[:, :3] @ np.array((0.0, 1.0, 0.0)))[:3]


def in_bound(sc, x_world):
    """is the world point inside the field's object-space bounding box"""
    T = np.eye(4)
    T[:3] = np.asarray(sc.to_world, np.float64)
    q = (np.linalg.inv(T) @ np.append(x_world, 1.0))[:3]
    return bool(abs(q[0]) < 1 and abs(q[1]) < 1 and 0 < q[2] < sc.max_height)


def rig(row, sc):
    """(names, the restatement's lights in world space)"""
    if row == "directional":
        return D.NAMES, [D.light(vector(sc, D.RIG[k][0]), D.RIG[k][1]) for k in D.NAMES]
    out = []
    for k in SPOT_NAMES:
        if k == "inside":
            out.append(P.light(inside_pose(sc), 0.3, 180, 180))
        else:
            o, t, up, cutoff, beam, intensity = P.RIG[k]
            out.append(P.light(pose(sc, o, t, up), intensity, cutoff, beam))
    return SPOT_NAMES, out


REF = {"directional": D, "spot": P}
# the maxima of profiles/row_scenes/f32_error.json (scripts/row_scenes_f32_error.py: the restatement in float32 against
# itself in float64 on these scenes), cut off after three digits; the GPU is allowed four times that, the factor every row's
# own file gives it for another operation order and fused multiply-adds.  tests/test_row_scenes.py holds them to the record
F32 = {"directional": {"image": 1.45e-7, "value": 1.84e-7, "dimage": 1.24e-7, "dvalue": 1.29e-7, "grad_sh_n": 1.55e-7,
                       "grad4": 1.70e-7, "grad_weight": 1.57e-7},
       "spot": {"image": 2.05e-7, "value": 5.27e-7, "dimage": 4.02e-7, "dvalue": 6.70e-7, "grad_sh_n": 4.84e-7, "grad_p": 5.40e-7,
                "grad15": 5.11e-7, "grad_weight": 4.43e-7},
       # (tests/test_gpu_caustic.py's measures: pos in pixels, value absolute, the derivatives relative L2; the maxima come
       # from eta = 1 / 1.33, whose lanes near the critical angle carry a factor 1 / cos_theta_t)
       "caustic": {"pos": 2.87e-4, "value": 1.96e-5, "grad_sh_n": 8.28e-5, "grad_p": 7.09e-7, "grad_weight": 5.07e-7, "dpos": 6.01e-5,
                   "dvalue": 1.03e-4,
                   # the rays: maxt relative to itself (near the critical angle a quotient of two small numbers), and the
                   # distance of the ray's end from the receiver's plane in world units
                   "maxt": 9.01e-3, "end": 3.14e-7},
       # (tests/test_gpu_rect.py's measures: image and value absolute -- `side` is close to the surface, its values reach
       # 26 --, the derivatives relative L2)
       "rect": {"image": 1.52e-5, "value": 6.27e-5, "dimage": 1.43e-6, "grad_sh_n": 5.50e-7, "grad_p": 1.05e-6, "grad_weight": 3.64e-7,
                "grad_tex": 4.75e-7},
       # (projector_ref.errors())
       "projector": {"image": 1.17e-7, "value": 4.66e-7, "uv": 3.43e-7, "dimage": 1.07e-6, "dvalue": 1.82e-6, "grad_sh_n": 7.02e-7,
                     "grad_p": 1.30e-6, "grad_weight": 4.15e-7, "grad14": 1.56e-6, "grad_tex": 1.16e-6},
       # (tests/test_gpu_reflect.py's measures: value and image absolute -- the sun of map_sun is bright --, the derivatives
       # relative L2)
       "reflect": {"value": 5.46e-5, "image": 3.15e-5, "grad_sh_n": 3.94e-6, "grad_weight": 6.55e-7, "grad_data": 1.24e-6,
                   "dimage": 3.20e-6, "dvalue": 3.43e-6},
       # (tests/test_gpu_refract.py's measures; `pos`: the landing position in texels, which REFRACT_BORDER rests on)
       "refract": {"value": 2.86e-5, "image": 7.15e-6, "grad_tex": 2.04e-6, "dvalue": 1.06e-4, "dimage": 1.06e-4, "grad_sh_n": 7.91e-5,
                   "grad_p": 1.76e-6, "grad_weight": 7.49e-7, "pos": 6.05e-5},
       # (tests/test_gpu_glossy.py's measures; ray_d, ray_h: the directions and microfacet normals, relative L2)
       "glossy": {"value": 2.44e-4, "image": 6.13e-5, "grad_data": 6.20e-6, "dimage": 1.60e-5, "dvalue": 1.64e-5, "grad_sh_n": 1.26e-5,
                  "grad_weight": 3.76e-6, "grad_alpha": 2.28e-5, "ray_d": 8.49e-7, "ray_h": 4.24e-7},
       # (specular_ref.errors(), per roughness row as in tests/test_gpu_specular.py: float32 cancels in s^2 / a^2 + c_h^2,
       # which the kernels form in double)
       "specular": {"row": {"image": 3.66e-5, "value": 9.73e-5, "dimage": 8.55e-5, "dvalue": 8.85e-5, "grad_sh_n": 1.11e-4,
                            "grad_alpha": 1.62e-4, "grad4": 4.20e-5, "grad_weight": 5.87e-5},
                    "sharp": {"image": 6.01e-4, "value": 6.89e-4, "dimage": 2.58e-4, "dvalue": 2.64e-4, "grad_sh_n": 9.98e-4,
                              "grad_alpha": 1.78e-3, "grad4": 1.05e-3, "grad_weight": 6.89e-4}},
       # (scripts/medium_f32_error.py's measure: the largest distance, per component, of the origin formed as the kernel
       # forms it from the exact point; values, gradients and tangents keep the row's own rule, MEDIUM_RTOL and MEDIUM_ATOL)
       "medium": {"origin": 5.76e-7}}
TOL = {row: {k: ({a: 4 * b for a, b in v.items()} if isinstance(v, dict) else 4 * v) for k, v in d.items()} for row, d in F32.items()}
# the relative L2 error the rows' own files allow their chain to the heights (tests/test_gpu_spot.py, test_gpu_directional.py)
CHAIN = 4 * 3.62e-7 + 1e-5


# ---- a (row, scene, mode) through the oracle and the restatements alone ---------------------------------------------
def oracle_records(sc, oracle, face_normals):
    """(field, rec: p, n, sh_n float32, t, prim): the oracle's records of the scene's wavefront; smooth shading normals
    from smooth_ref (lighting_scenes.smooth_normals)"""
    f = LS.oracle_field(sc, oracle)
    t, u, v, prim = f.ray_intersect_preliminary(sc.rays)
    rec = f.compute_surface_interaction(sc.rays, t, u, v, prim, oracle.RAY_ALL)
    sh = rec["sh_n"] if face_normals else LS.smooth_normals(sc, sc.rays, prim, np.isfinite(t)).astype(np.float32)
    return f, {"p": rec["p"], "n": rec["n"], "sh_n": sh}, t, prim


def shadow_rays(row, L, rec, d, t):
    """[7, n] float32 shadow rays of the light L and the traced mask, from the restatement"""
    M = REF[row]
    o, w, maxt, tr = M.rays(L, rec["p"], rec["n"], rec["sh_n"], d, t)
    return np.concatenate([o, w, maxt[None]]).astype(np.float32), tr


def populations(row, sc, names, lights, rec, d, t, vis, field=None):
    """the shares of a (row, scene) from records and a [K, n] visibility: per light traced, occluded of traced; the union of
    unsure samples; for the spot row the rays that end inside the bound and -- with the oracle's field -- how many of the
    oracle's answers +inf in place of maxt changes"""
    M = REF[row]
    el, _ = M.eligible(rec["sh_n"], d, t)
    q = types.SimpleNamespace(eligible=el, shares={}, union=np.zeros(len(t), bool), inside=0, changed=None)
    q.traced, q.unsure = [], []
    for k, (name, L) in enumerate(zip(names, lights)):
        tr, un = (M.traced(L, rec["sh_n"], d, t) if row == "directional" else M.traced(L, rec["p"], rec["sh_n"], d, t))
        q.traced.append(tr); q.unsure.append(un)
        q.union |= un
        occ = tr & ~vis[k]
        q.shares[name] = {"traced": int(tr.sum()), "occluded": int(occ.sum()), "traced_of_eligible": float(tr[el].mean()),
                          "occluded_of_traced": float(occ[tr].mean()) if tr.any() else 0.0}
        if row == "spot" and in_bound(sc, L.to_world[:, 3]):
            q.inside += int(tr.sum())
            if field is not None:
                r7, _ = shadow_rays(row, L, rec, d, t)
                r7 = r7[:, tr]
                ended = field.ray_test(r7).astype(bool)
                r7[6] = np.inf
                q.changed = (q.changed or 0) + int((field.ray_test(r7).astype(bool) != ended).sum())
    q.traced, q.unsure = np.stack(q.traced), np.stack(q.unsure)
    q.unsure_share = float(q.union.mean())
    return q


def model(row, sc, oracle, face_normals):
    """the triple through the oracle and the restatement only: a namespace with field, rec, t, names, lights, vis [K, n] and
    pop (populations())"""
    f, rec, t, prim = oracle_records(sc, oracle, face_normals)
    names, lights = rig(row, sc)
    d = sc.rays[3:6]
    vis = []
    for L in lights:
        r7, tr = shadow_rays(row, L, rec, d, t)
        v = np.zeros(sc.n, bool)
        v[tr] = ~f.ray_test(r7[:, tr]).astype(bool)
        vis.append(v)
    m = types.SimpleNamespace(field=f, rec=rec, t=t, prim=prim, names=names, lights=lights, vis=np.stack(vis))
    m.pop = populations(row, sc, names, lights, rec, d, t, m.vis, f)
    return m


def conditions(row, sc, pop):
    """what makes (row, scene) a test; asserted before anything is compared.  The cap on the samples that rounding may decide
    is row_helpers.UNSURE_CAP and is never raised; the floors keep both outcomes of the visibility populated"""
    sh = pop.shares
    assert pop.unsure_share <= UNSURE_CAP, (row, sc.name, pop.unsure_share)
    if row == "directional":
        # (`below` traces nothing on `affine` and `flip_below`: directional_ref.assert_shares does not carry over)
        # fully visible: every eligible sample is traced and none is occluded.  On `mirror_flip` the oracle shadows exactly
        # one sample of 2126 under `zenith` and `high`: its spawned origin leaves the footprint of its own triangle at a
        # sharp ridge and starts under the neighbour (a hit at distance 6e-5).  That one sample is allowed there and
        # nowhere else, so that a second one is noticed
        allowed = 1 if sc.name == "mirror_flip" else 0
        clear = [k for k, v in sh.items() if v["traced_of_eligible"] == 1.0 and v["occluded"] <= allowed]
        mixed = [k for k, v in sh.items() if v["traced"] >= 100 and 0.2 <= v["occluded_of_traced"] <= 0.9]
        assert len(clear) >= 1 and len(mixed) >= 3, (sc.name, clear, mixed, sh)
    else:
        for k in ("side", "graze"):
            assert sh[k]["traced"] >= 100 and 0.2 <= sh[k]["occluded_of_traced"] <= 0.9, (sc.name, k, sh[k])
        assert sh["inside"]["traced"] >= 100 and 0.01 <= sh["inside"]["occluded_of_traced"] <= 0.99, (sc.name, sh["inside"])
        assert pop.inside >= 100, (sc.name, pop.inside)                    # rays that end inside the bound
        assert pop.changed is None or pop.changed >= 10, (sc.name, pop.changed)   # ... and whose end decides the answer


def describe(pop):
    return "unsure %.2e inside %d changed by +inf %s | " % (pop.unsure_share, pop.inside, pop.changed) + ", ".join(
        "%s %d/%.2f" % (k, v["traced"], v["occluded_of_traced"]) for k, v in pop.shares.items())


# ---- the GPU's side ---------------------------------------------------------------------------------------------------
def device_scene(hf, oracle, name, view, face_normals):
    """the scene on the device: the Heightfield with the scene's to_world and flip_normals, the records of
    shape.ray_intersect, the records as numpy and the oracle's field.  Asserts first that prim_index and the hit mask are
    the oracle's"""
    import torch
    sc = scene(name, view)
    sc.face_normals = face_normals
    sc.ht = torch.from_numpy(sc.h).cuda()
    sc.tw64 = np.asarray(sc.to_world, np.float64)
    sc.shape = hf.Heightfield(heightfield=sc.ht, max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                              face_normals=face_normals)
    rt = torch.from_numpy(sc.rays).cuda()
    sc.rt = rt
    sc.ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
    sc.field = LS.oracle_field(sc, oracle)
    sc.pi_oracle = sc.field.ray_intersect_preliminary(sc.rays)
    t, _, _, prim = sc.pi_oracle
    pi = sc.shape.ray_intersect_preliminary(sc.ray)
    hit = LS._np(pi.is_valid())
    assert np.array_equal(hit, np.isfinite(t)) and hit.any(), sc.name
    assert np.array_equal(LS._np(pi.prim_index).view(np.uint32)[hit], np.asarray(prim).view(np.uint32)[hit]), sc.name
    sc.si = si = sc.shape.ray_intersect(sc.ray, hf.RayFlags.All)
    sc.np = {k: LS._np(v) for k, v in (("p", si.p), ("n", si.n), ("sh_n", si.sh_frame.n), ("d", sc.ray.d), ("t", si.t))}
    sc.hit = hit
    return sc


# ---- the caustic row: rays that END at the receiver, the oblique view ------------------------------------------------
# From the steep view refracted rays are almost never occluded; from the oblique one they are, and the receiver that cuts
# the relief decides answers by where the ray ends.  The receivers are the images of the object planes z = -0.5 (z =
# max_height + 0.5 for the view from below: the far side of the field) and z = 0.4 max_height, a film of CAUSTIC_FILM^2
# pixels over [-1, 1]^2: the origin carried as a point, ex and ey as vectors.  hf.Receiver refuses the non-orthogonal pair
# that a shear or an anisotropic scale produces, so ey is orthogonalised against ex after carrying (the plane stays the
# image of the object plane); the values are rounded to float32, which is what hf_receiver_t holds.
CAUSTIC_ETAS = (1.33, 1 / 1.33)
CAUSTIC_FILM = 32
CAUSTIC_MARGIN = 1e-5          # tests/test_gpu_caustic.py's MARGIN
CAUSTIC_PLANES = ("far", "cut")
CAUSTIC_RUNS = tuple((eta, plane) for eta in CAUSTIC_ETAS for plane in CAUSTIC_PLANES)
# answers of the oracle that +inf in place of maxt = s changes, on the cutting receiver: the floor the rows' issue sets.
# On `flip_below` at eta 1.33 the count is exactly 10 on the oracle's records and on the GPU's: there is no margin there, and
# a single record that differed between the two would fail the condition without any kernel being wrong (the other runs
# count 22 to 55)
FLOOR_CHANGED = 10
# the caustic rays' maxt is held to tests/test_gpu_caustic.py's absolute bound (the landing point moves by at most
# TOL[pos] pixels) on the lanes with |<wo, N>| and cos_theta_t at least this: there the restatement's own float32 error is at
# most 0.65 of a quarter of that bound on these scenes; below it maxt is a quotient of two small numbers and is held
# relative to itself (F32[caustic][maxt]) together with the ray's end on the receiver's plane (F32[caustic][end]).  The same holds on the
# refract row's receivers with that row's tolerance of a position
CAUSTIC_WELL = 0.2


def caustic_runs(face_normals):
    """the (eta, plane) pairs of a shading mode.  With smooth normals on `affine` no ray refracted at eta = 1.33 is occluded
    at all (the oracle's answer on 1751 and 1413 rays), so neither outcome floor can be met: that eta is dropped there, in
    the CPU and in the GPU file"""
    return tuple(r for r in CAUSTIC_RUNS if face_normals or r[0] < 1)


def caustic_plane_z(sc, plane):
    if plane == "cut":
        return 0.4 * sc.max_height
    return sc.max_height + 0.5 if sc.below else -0.5


def caustic_receiver(sc, plane):
    """(origin, ex, ey) as float32 arrays, world space"""
    import caustic_ref as C
    A = np.asarray(sc.to_world, np.float64)
    obj = C.plane_z(caustic_plane_z(sc, plane), (-1.0, 1.0), (-1.0, 1.0), CAUSTIC_FILM, CAUSTIC_FILM)
    o, ex, ey = A[:, :3] @ obj.origin + A[:, 3], A[:, :3] @ obj.ex, A[:, :3] @ obj.ey
    ey = ey - ex * (ex @ ey) / (ex @ ex)
    return tuple(np.asarray(v, np.float32) for v in (o, ex, ey))


def caustic_inputs(n):
    """the weights, upstream gradients and tangents of tests/test_gpu_caustic.py's _inputs"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    gpos, gv = rng.normal(size=(2, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dn, dp, dw = (rng.normal(size=s).astype(np.float32) for s in ((3, n), (3, n), (n,)))
    return w, gpos, gv, dn, dp, dw


def caustic_run(sc, rec, d, t, eta, plane, field, vis=None, rcv3=None):
    """one (eta, receiver) on the records rec: the restatement's rays and masks, the oracle's answer on those rays (`vis` =
    None: the visibility IS the oracle's) and the counts the conditions are about"""
    import caustic_ref as C
    r = types.SimpleNamespace(eta=eta, plane=plane)
    r.rcv3 = caustic_receiver(sc, plane) if rcv3 is None else rcv3
    r.rref = C.receiver(*r.rcv3)
    r.a = (rec["p"], rec["n"], rec["sh_n"], d, t)
    r.traced, r.o, r.wo, r.maxt, r.v = C.rays(*r.a, None, eta, r.rref)
    hit = np.isfinite(t)
    r.sure = (r.v.margin > CAUSTIC_MARGIN) | ~hit
    rows = np.concatenate([r.o, r.wo, r.maxt[None]]).astype(np.float32)
    occ = np.zeros(len(t), bool)
    occ[r.traced] = field.ray_test(rows[:, r.traced]).astype(bool)
    rows[6] = np.where(r.traced, np.inf, -1)
    occ_inf = np.zeros(len(t), bool)
    occ_inf[r.traced] = field.ray_test(rows[:, r.traced]).astype(bool)
    r.vis = (r.traced & ~occ) if vis is None else np.asarray(vis, bool)
    r.counts = {"hits": int(hit.sum()), "eligible": int(r.v.eligible.sum()), "tir": int((r.v.eligible & r.v.tir).sum()),
                "traced": int(r.traced.sum()), "occluded": int((r.traced & ~r.vis).sum()), "deposited": int(r.vis.sum()),
                "changed_by_inf": int((occ != occ_inf).sum()), "unsure": float((~r.sure).mean())}
    return r


def caustic_end(r, wo, s):
    """[n]: how far the end p + wo s of every ray is from the receiver's plane, world units"""
    X = np.asarray(r.a[0], np.float64) + wo * s - r.rref.origin[:, None]
    return np.abs((X * r.rref.N[:, None]).sum(0))


def caustic_conditions(sc, runs):
    """what makes (caustic, scene) a test; runs: {(eta, plane): caustic_run}.  Total internal reflection at 1 / 1.33 and
    deposition decide at least 1 % of the hits both ways on every run they can occur on, occlusion decides at least 1 % of
    the traced rays both ways on the far receiver of at least one eta (from below the far receiver of the other eta
    shadows a handful only), and on the cutting receiver +inf in place of maxt changes at least FLOOR_CHANGED answers"""
    far = []
    for (eta, plane), r in runs.items():
        c = r.counts
        assert c["unsure"] <= UNSURE_CAP, (sc.name, eta, plane, c)
        assert c["traced"] >= 300 and c["hits"] >= 1000, (sc.name, eta, plane, c)
        for count in (c["deposited"], c["hits"] - c["deposited"]):
            assert count >= 0.01 * c["hits"], (sc.name, eta, plane, c)
        if eta < 1:
            assert min(c["tir"], c["hits"] - c["tir"]) >= 0.01 * c["hits"], (sc.name, eta, plane, c)
        if plane == "cut":
            assert c["changed_by_inf"] >= FLOOR_CHANGED, (sc.name, eta, plane, c)
        else:
            far.append(min(c["occluded"], c["traced"] - c["occluded"]) >= 0.01 * c["traced"])
    assert any(far), (sc.name, {k: r.counts for k, r in runs.items()})


def caustic_model(sc, oracle, face_normals):
    """{(eta, plane): caustic_run} through the oracle and the restatement only"""
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return {(eta, plane): caustic_run(sc, rec, sc.rays[3:6], t, eta, plane, f) for eta, plane in caustic_runs(face_normals)}


# ---- the rect row: rays that END on the lamp, the steep view ---------------------------------------------------------
# rect_ref.LAMPS carried to world: the centre as a point, ex and ey as vectors (a parallelogram after a shear, which
# hf_rect_light_t allows), the normal turned again towards the carried target.  `side` is placed where the spot light
# `inside` is -- its centre over the lowest inner vertex at RECT_Z max_height (under the highest one for the view from
# below), facing the surface -- so that its draws lie INSIDE the field's bounding box with terrain
# behind them: the shadow rays end inside the bound, and +inf in place of maxt changes the oracle's answer.  `above`
# shadows almost nothing on these scenes: it is kept for the values, the floors are on `side`.
RECT_K, RECT_SEED, RECT_TEX = 8, 5, (16, 8)          # draws per sample, seed, texture (TW, TH)
RECT_LAMPS = ("above", "side")
RECT_Z = 0.7                  # the height of `side` in max_height: higher than INSIDE_Z, for a penumbra over the floor


def rect_lamp(sc, lname):
    import rect_ref as A
    obj = A.LAMPS[lname](A.RADIANCE)
    if lname != "side":
        return A.lamp(point(sc, obj.center), vector(sc, obj.ex), vector(sc, obj.ey), A.RADIANCE, point(sc, A.TARGET))
    x, y, _ = extreme_vertex(sc)
    w = np.asarray(sc.to_world, np.float64)
    z, floor = ((1.0 - RECT_Z) * sc.max_height, sc.max_height) if sc.below else (RECT_Z * sc.max_height, 0.0)
    return A.lamp(w[:, :3] @ np.array((x, y, z)) + w[:, 3], vector(sc, obj.ex), vector(sc, obj.ey), A.RADIANCE,
                  w[:, :3] @ np.array((x, y, floor)) + w[:, 3])


def rect_run(sc, rec, d, t, lname, field, bits=None):
    """one lamp on the records rec: the restatement's draws, masks and shadow rays, the oracle's answer on those rays
    (`bits` = None: the visibility IS the oracle's) and the counts the conditions are about"""
    import rect_ref as A
    r = types.SimpleNamespace(lname=lname, lm=rect_lamp(sc, lname), rec=rec, t=t, field=field)
    n = len(t)
    r.ids = np.arange(n, dtype=np.uint32)
    r.draws = A.draws(r.ids, RECT_K, RECT_SEED)
    r.g = A.geometry(rec["p"], rec["sh_n"], r.draws, r.lm)
    r.eligible, front = A.eligible(rec["sh_n"], d, t)
    r.traced, r.margin = A.traced(rec["sh_n"], d, t, r.g)
    hit = np.isfinite(t)
    r.sure = (front > A.MARGIN) | ~hit                                      # the samples whose values are compared
    r.sure_k = r.sure[None] & ((r.margin > A.MARGIN) | ~r.eligible[None])   # the draws whose masks are compared
    T = np.eye(4)
    T[:3] = np.asarray(sc.to_world, np.float64)
    qo = np.einsum("ij,kjn->kin", np.linalg.inv(T)[:3, :3], r.g.q - T[:3, 3][None, :, None])
    r.ends_inside = r.traced & (np.abs(qo[:, 0]) < 1) & (np.abs(qo[:, 1]) < 1) & (qo[:, 2] > 0) & (qo[:, 2] < sc.max_height)
    occ, occ_inf, r.rays = np.zeros((RECT_K, n), bool), np.zeros((RECT_K, n), bool), []
    for k in range(RECT_K):
        o, w, maxt, tr = A.rays(rec["p"], rec["n"], rec["sh_n"], d, t, r.ids, k, RECT_SEED, r.lm)
        assert np.array_equal(tr, r.traced[k])
        r.rays.append((o, w, maxt))
        r7 = np.concatenate([o, w, maxt[None]]).astype(np.float32)[:, tr]
        occ[k, tr] = field.ray_test(r7).astype(bool)
        r7[6] = np.inf
        occ_inf[k, tr] = field.ray_test(r7).astype(bool)
    r.bits = (r.traced & ~occ) if bits is None else np.asarray(bits, bool)
    some, every = r.bits.any(0), (r.bits == r.traced).all(0)
    r.counts = {"eligible": int(r.eligible.sum()), "traced": int(r.traced.sum()),
                "occluded_of_traced": float(1.0 - (r.bits & r.traced).sum() / r.traced.sum()),
                "penumbra_of_eligible": float((some & ~every)[r.eligible].mean()), "ends_inside": int(r.ends_inside.sum()),
                "changed_by_inf": int((occ != occ_inf).sum()), "changed_by_inf_inside": int(((occ != occ_inf) & r.ends_inside).sum()),
                "unsure": float((~r.sure_k.all(0)).mean())}
    return r


def rect_conditions(sc, runs):
    """what makes (rect, scene) a test; runs: {lname: rect_run}.  The floors are those of tests/test_gpu_rect.py, on `side`"""
    for lname, r in runs.items():
        assert r.counts["unsure"] <= UNSURE_CAP and r.counts["eligible"] >= 1000, (sc.name, lname, r.counts)
    c = runs["side"].counts
    assert 0.03 <= c["occluded_of_traced"] <= 0.8 and c["penumbra_of_eligible"] >= 0.05, (sc.name, c)
    assert c["ends_inside"] >= 100 and c["changed_by_inf_inside"] >= FLOOR_CHANGED, (sc.name, c)


def rect_errors(got, ref, sure, pix):
    """tests/test_gpu_rect.py's measures: image and value absolute on the pixels and samples that no rounding decides, every
    derivative as the L2 norm of the difference over the L2 norm of ref; got, ref: dicts"""
    from row_helpers import _rel
    out = {"image": float(np.abs(got["image"] - ref["image"])[pix].max()), "value": float(np.abs(got["value"] - ref["value"])[sure].max()),
           "dimage": _rel(got["dimage"][pix], ref["dimage"][pix])}
    for k in ("grad_sh_n", "grad_p", "grad_weight"):
        out[k] = _rel(got[k][..., sure], ref[k][..., sure])
    if ref.get("grad_tex") is not None:
        out["grad_tex"] = _rel(got["grad_tex"], ref["grad_tex"])
    return out


def rect_evaluate(r, rec, d, t, x, tex, dtype=np.float64):
    """forward, adjoint and tangent of the restatement on the run r under the inputs x (rect_ref.inputs): the dict
    rect_errors takes"""
    import rect_ref as A
    args = (rec["p"], rec["sh_n"], d, t, x.w, r.bits, r.ids, RECT_SEED, r.lm, tex, A.ALBEDO)
    image, value = A.forward(*args, SPP, dtype)
    gn, gp, gw, gt = A.adjoint(*args, SPP, x.gi, dtype)
    dimage, _ = A.tangent(*args, SPP, x.dn, x.dp, x.dw, None if tex is None else x.dtex, dtype)
    return {"image": image, "value": value, "grad_sh_n": gn, "grad_p": gp, "grad_weight": gw, "grad_tex": gt, "dimage": dimage}


def rect_model(sc, oracle, face_normals):
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return {lname: rect_run(sc, rec, sc.rays[3:6], t, lname, f) for lname in RECT_LAMPS}


# ---- the projector row: rays that END at the projector, its pinhole mapping in world space, the steep view -----------
# projector_ref.PROJECTORS carried to world as the spot lights are: the rigid look_at of the carried origin and of a carried
# point on the axis, the carried `up` picking the roll; fov, scale and the 16 x 8 texture as they are.
PROJ_NAMES = ("above", "side")
PROJ_VARIANTS = (("clamp", True), ("repeat", True), ("repeat", False))     # (wrap, textured): tests/test_gpu_projector.py's


def projector_of(sc, name):
    import projector_ref as PR
    obj = PR.PROJECTORS[name]()
    o, axis, up = obj.to_world[:, 3], obj.to_world[:, 2], obj.to_world[:, 1]
    return PR.projector(pose(sc, o, o + axis, up), obj.fov, obj.scale)


def projector_run(sc, rec, d, t, name, field, vis=None):
    """one projector on the records rec: the restatement's masks and shadow rays, the oracle's answer on those rays (`vis` =
    None: the visibility IS the oracle's) and the counts the conditions are about"""
    import projector_ref as PR
    r = types.SimpleNamespace(name=name, pr=projector_of(sc, name))
    r.eligible, _ = PR.eligible(rec["sh_n"], d, t)
    r.traced, r.unsure = PR.traced(r.pr, rec["p"], rec["sh_n"], d, t)
    r.sure = ~r.unsure
    r.pix = r.sure.reshape(-1, SPP).all(1)
    r.o, r.w, r.maxt, _ = PR.rays(r.pr, rec["p"], rec["n"], rec["sh_n"], d, t)
    r7 = np.concatenate([r.o, r.w, r.maxt[None]]).astype(np.float32)[:, r.traced]
    occ = np.zeros(len(t), bool)
    occ[r.traced] = field.ray_test(r7).astype(bool)
    r.vis = (r.traced & ~occ) if vis is None else np.asarray(vis, bool)
    r.m = PR.mapping(r.pr, rec["p"])
    with np.errstate(invalid="ignore"):
        r.lanes = np.isfinite(t) & (r.m.ref[2] > 0)
    r.steady = PR.steady(r.pr, rec["p"], r.vis) & r.sure
    n_el = max(int(r.eligible.sum()), 1)
    r.counts = {"eligible": int(r.eligible.sum()), "lit_of_eligible": float(r.m.lit[r.eligible].mean()), "traced": int(r.traced.sum()),
                "visible_of_eligible": float(r.vis.sum() / n_el), "occluded_of_eligible": float((r.traced & ~r.vis).sum() / n_el),
                "unsure": float(r.unsure.mean()), "at_a_cell_border": float((r.vis & ~r.steady).sum() / max(r.vis.sum(), 1))}
    return r


def projector_conditions(sc, runs):
    """what makes (projector, scene) a test; runs: {name: projector_run}.  Under `side` both outcomes of the visibility decide
    at least 1 % of the eligible samples; `above` shadows nothing here (as on the scene of tests/test_gpu_projector.py): it
    is kept for the mapping, and the floor on it is that file's: its frustum cuts the wavefront"""
    for name, r in runs.items():
        c = r.counts
        assert c["unsure"] <= UNSURE_CAP and c["eligible"] >= 1000 and c["visible_of_eligible"] >= 0.01, (sc.name, name, c)
    assert runs["side"].counts["occluded_of_eligible"] >= 0.01, (sc.name, runs["side"].counts)
    assert 0.15 <= runs["above"].counts["lit_of_eligible"] <= 0.95, (sc.name, runs["above"].counts)


def projector_model(sc, oracle, face_normals):
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return {name: projector_run(sc, rec, sc.rays[3:6], t, name, f) for name in PROJ_NAMES}, rec, t


# ---- the reflect row: rays with maxt = inf whose direction and whose masks depend on the view, the oblique view ------
# The environment map is a world-space emitter: nothing is carried.  What the scenes add over tests/test_gpu_reflect.py is
# the specular vertex's sign tests (c = <sh_n, wi>, <g, wi>, <g, wr>) and the side of the spawn_ray offset when flip_normals
# turns the geometric normal over, alone (`flip_below`) and together with a negative-determinant to_world (`mirror_flip`).
REFLECT_ETAS = (0.0, 1.5)
REFLECT_MAPS = {"sun": (17, 9), "gradient": (9, 5)}          # tests/test_gpu_reflect.py's maps (W, H)
REFLECT_PAIRS = (("sun", "rotated"), ("gradient", "identity"))
REFLECT_MARGIN, REFLECT_BORDER, REFLECT_LEFT_OUT_CAP = 1e-5, 1e-4, 2e-3     # that file's


def reflect_rots():
    import envmap_ref as E
    c, s = np.cos(0.7), np.sin(0.7)
    return {"identity": np.eye(3), "rotated": E.DEFAULT_ROT @ np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])}


def reflect_run(sc, rec, d, t, field, vis=None):
    """the reflected rays of the records rec from the restatement, the oracle's answer on them (`vis` = None: the visibility
    IS the oracle's) and the counts the conditions are about"""
    import reflect_ref as RR
    r = types.SimpleNamespace()
    r.a = (rec["n"], rec["sh_n"], d, t)
    r.traced, r.o, r.wr, r.maxt, r.v = RR.rays(rec["p"], *r.a)
    hit = np.isfinite(t)
    r.sure = (r.v.margin > REFLECT_MARGIN) | ~hit
    r7 = np.concatenate([r.o, r.wr, r.maxt[None]]).astype(np.float32)[:, r.traced]
    occ = np.zeros(len(t), bool)
    occ[r.traced] = field.ray_test(r7).astype(bool)
    r.vis = (r.traced & ~occ) if vis is None else np.asarray(vis, bool)
    r.counts = {"hits": int(hit.sum()), "eligible": int(r.v.eligible.sum()), "inconsistent": int((r.v.eligible & ~r.v.consistent).sum()),
                "traced": int(r.traced.sum()), "visible": int(r.vis.sum()), "occluded": int((r.traced & ~r.vis).sum()),
                "unsure": float((~r.sure).mean())}
    return r


def reflect_conditions(sc, r):
    """what makes (reflect, scene) a test: both outcomes of the visibility decide at least 1 % of the eligible samples"""
    c = r.counts
    assert c["unsure"] <= UNSURE_CAP and c["eligible"] >= 1000, (sc.name, c)
    assert c["visible"] >= 0.01 * c["eligible"] and c["occluded"] >= 0.01 * c["eligible"], (sc.name, c)


def reflect_model(sc, oracle, face_normals):
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return reflect_run(sc, rec, sc.rays[3:6], t, f), rec, t


def reflect_inputs(n, shape):
    """the weights, upstream gradients and tangents of tests/test_gpu_reflect.py's _inputs"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    gi, gv = rng.normal(size=n // SPP).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dn, dw = rng.normal(size=(3, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    dd = rng.normal(size=shape).astype(np.float32)
    return w, gi, gv, dn, dw, dd


def reflect_keep(r, full, rot):
    """the lanes whose derivatives are compared: sure, traced by both sides where visible, and their lookup at least
    REFLECT_BORDER of a cell away from a cell border and not at a pole (tests/test_gpu_reflect.py's)"""
    import reflect_ref as RR
    return r.sure & (r.vis == (r.traced & r.vis)) & RR.smooth_lanes(r.v.wr, full.shape[1], full.shape[0], rot, REFLECT_BORDER)


def reflect_evaluate(r, eta, full, rot, x, keep, dtype=np.float64):
    """forward, adjoint and tangent of the restatement under the inputs x = reflect_inputs(): a dict in the names of
    reflect_errors; ddata's seam column is column 0's, as Envmap.full() copies it"""
    import reflect_ref as RR
    w, gi, gv, dn, dw, dd = x
    args = (*r.a, None, w, eta, full, rot, r.vis, SPP)
    image, value = RR.forward(*args, dtype=dtype)
    gm, gw, gd = RR.adjoint(*args, gi, gv, dtype=dtype)
    dimage, dvalue = RR.tangent(*args, dn * keep, dw, np.concatenate([dd[:, :-1], dd[:, :1]], 1), dtype=dtype)
    return {"image": image, "value": value, "grad_sh_n": gm, "grad_weight": gw, "grad_data": gd, "dimage": dimage, "dvalue": dvalue}


def reflect_errors(got, ref, keep, vis):
    """tests/test_gpu_reflect.py's measures: value and image absolute, every derivative relative L2"""
    from row_helpers import _rel
    return {"value": float(np.abs(got["value"] - ref["value"])[keep | ~vis].max()), "image": float(np.abs(got["image"] - ref["image"]).max()),
            "grad_sh_n": _rel(got["grad_sh_n"][:, keep], ref["grad_sh_n"][:, keep]),
            "grad_weight": _rel(got["grad_weight"][keep], ref["grad_weight"][keep]), "grad_data": _rel(got["grad_data"], ref["grad_data"]),
            "dimage": _rel(got["dimage"], ref["dimage"]), "dvalue": _rel(got["dvalue"][keep], ref["dvalue"][keep])}


# ---- the refract row: the caustic row's rays, landing on a textured receiver whose film is laid out in world space ------
# The receivers are the caustic row's planes; the film is the 16 x 8 texture over the image of the object square [-1, 1]^2:
# ex = (TW / 2) A e_x / |A e_x|^2, ey likewise from A e_y made orthogonal to ex (hf.Receiver refuses another pair), so that
# a point A x of the plane lands near (TW (x + 1) / 2, TH (y + 1) / 2) and a good share of the samples reads the texture's
# inside.  What the scenes add over tests/test_gpu_refract.py: the landing position, its texel and the slopes of the
# lookup come from a world-space p, wo and s under a transform; the texel gradient and the chain follow them.
REFRACT_TEX = (16, 8)                               # TW, TH
REFRACT_BORDER, REFRACT_LEFT_OUT_CAP = 5e-3, 3e-2   # tests/test_gpu_refract.py's: texels, share of the lit lanes
REFRACT_VARIANTS = ((0.0, "smooth", "clamp"), (0.7, "random", "repeat"))        # (sigma_t, texture, wrap)


def refract_receiver(sc, plane):
    """(origin, ex, ey) as float32 arrays, world space"""
    A = np.asarray(sc.to_world, np.float64)
    TW, TH = REFRACT_TEX
    o = A[:, :3] @ np.array((-1.0, -1.0, caustic_plane_z(sc, plane))) + A[:, 3]
    ax, ay = A[:, 0], A[:, 1]
    ay = ay - ax * (ax @ ay) / (ax @ ax)
    return tuple(np.asarray(v, np.float32) for v in (o, ax * (TW / 2) / (ax @ ax), ay * (TH / 2) / (ay @ ay)))


def refract_run(sc, rec, d, t, eta, plane, field, vis=None):
    """caustic_run with the textured receiver, and the lanes the comparisons keep (tests/test_gpu_refract.py's _run)"""
    import refract_ref as RR
    r = caustic_run(sc, rec, d, t, eta, plane, field, vis, refract_receiver(sc, plane))
    TW, TH = REFRACT_TEX
    sure = r.sure & (r.vis == (r.traced & r.vis))
    _, _, pos64 = RR.forward(*r.a, None, None, eta, 0.0, r.rref, RR.textures(TW, TH)["smooth"], RR.CLAMP, r.vis)
    r.keep = sure & r.vis & ~RR.near_border(pos64, REFRACT_BORDER)
    r.pix = RR.whole_pixels(r.keep | (sure & ~r.vis), SPP)
    inside = r.vis & (pos64[0] >= 0) & (pos64[0] <= TW) & (pos64[1] >= 0) & (pos64[1] <= TH)
    r.counts["left_out"] = float((r.vis & ~r.keep).sum() / max(r.vis.sum(), 1))
    r.counts["inside"] = float(inside.sum() / max(r.vis.sum(), 1))
    return r


def refract_conditions(sc, runs):
    """the caustic row's conditions (the rays and the visibility are that row's) and the lookup's: at most
    REFRACT_LEFT_OUT_CAP of the lit lanes lie within REFRACT_BORDER of a cell border, and both the inside of the texture
    and its outside (where the wrap decides) are read by at least 0.5 % of the lit lanes"""
    caustic_conditions(sc, runs)
    for k, r in runs.items():
        assert r.counts["left_out"] <= REFRACT_LEFT_OUT_CAP and 0.3 < r.counts["inside"] <= 0.995, (sc.name, k, r.counts)


def refract_model(sc, oracle, face_normals):
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return {(eta, plane): refract_run(sc, rec, sc.rays[3:6], t, eta, plane, f) for eta, plane in caustic_runs(face_normals)}


def refract_evaluate(r, eta, sigma_t, tex, wrap, x, dtype=np.float64):
    """forward, adjoint and tangent of the restatement under x = refract_ref.inputs(): a dict in refract_errors' names"""
    import refract_ref as RR
    args = (*r.a, None, x.w, eta, sigma_t, r.rref, tex, wrap, r.vis)
    value, image, _ = RR.forward(*args, SPP, dtype)
    gm, gp, gw, gt = RR.adjoint(*args, x.gi, x.gv, SPP, dtype)
    dvalue, dimage = RR.tangent(*args, x.dn, x.dp, x.dw, x.dtex, SPP, dtype)
    return {"value": value, "image": image, "grad_sh_n": gm, "grad_p": gp, "grad_weight": gw, "grad_tex": gt, "dvalue": dvalue,
            "dimage": dimage}


def refract_errors(got, ref, keep, pix):
    """tests/test_gpu_refract.py's measures: value and image absolute, every derivative relative L2"""
    from row_helpers import _rel
    out = {"value": float(np.abs(got["value"] - ref["value"])[keep].max()), "image": float(np.abs(got["image"] - ref["image"])[pix].max()),
           "grad_tex": _rel(got["grad_tex"], ref["grad_tex"]), "dvalue": _rel(got["dvalue"][keep], ref["dvalue"][keep]),
           "dimage": _rel(got["dimage"][pix], ref["dimage"][pix])}
    for k in ("grad_sh_n", "grad_p", "grad_weight"):
        out[k] = _rel(got[k][..., keep], ref[k][..., keep])
    return out


# ---- the glossy row: GLOSSY_K mirror rays per sample about drawn microfacet normals, maxt = inf, the oblique view --------
# What the scenes add over tests/test_gpu_glossy.py: every draw's masks (<wi, h>, c_o, <g, wo>) and the side of its
# spawn_ray offset when flip_normals turns the geometric normal over, the frame about a world-space sh_n, the roughness
# and texel gradients and the chain on a transformed shape.  The environment map is a world-space emitter.
GLOSSY_K, GLOSSY_SEED, GLOSSY_MARGIN = 4, 5, 1e-5
GLOSSY_ETAS = (0.0, 1.5)
GLOSSY_COMBOS = (("row", "sun", "rotated"), (0.3, "gradient", "identity"))      # (alpha, map, rotation) of glossy_ref


def glossy_run(sc, rec, d, t, akind, field, bits=None):
    """the GLOSSY_K mirror rays of the records rec from the restatement, the oracle's answer on them (`bits` = None: the
    visibility IS the oracle's) and the counts the conditions are about"""
    import glossy_ref as G
    n = len(t)
    r = types.SimpleNamespace(alpha=G.alpha_row(akind, n), a=(rec["n"], rec["sh_n"], d, t))
    ref = [G.rays(rec["p"], *r.a, r.alpha, k, GLOSSY_SEED) for k in range(GLOSSY_K)]
    r.traced, r.o, r.wo, r.maxt, r.h, r.margin = (np.stack(x) for x in zip(*[q[:6] for q in ref]))
    hit = np.isfinite(t)
    r.eligible, _ = G.eligible(*r.a, None, r.alpha)
    r.sure_k = (r.margin > GLOSSY_MARGIN) | ~hit[None]
    r.sure = r.sure_k.all(0)
    occ = np.zeros((GLOSSY_K, n), bool)
    for k in range(GLOSSY_K):
        r7 = np.concatenate([r.o[k], r.wo[k], r.maxt[k][None]]).astype(np.float32)[:, r.traced[k]]
        occ[k, r.traced[k]] = field.ray_test(r7).astype(bool)
    r.bits = (r.traced & ~occ) if bits is None else np.asarray(bits, bool)
    r.keep = r.sure & ~(r.bits & ~r.traced).any(0)
    r.counts = {"eligible": int(r.eligible.sum()), "traced": int(r.traced.sum()), "untraced_of_eligible_draws":
                int((r.eligible[None] & ~r.traced).sum()), "visible": int(r.bits.sum()), "occluded": int((r.traced & ~r.bits).sum()),
                "unsure": float((~r.sure).mean())}
    return r


def glossy_conditions(sc, r):
    """what makes (glossy, scene) a test: both outcomes of the visibility decide at least 1 % of the eligible draws"""
    c = r.counts
    assert c["unsure"] <= UNSURE_CAP and c["eligible"] >= 1000, (sc.name, c)
    assert min(c["visible"], c["occluded"]) >= 0.01 * GLOSSY_K * c["eligible"], (sc.name, c)


def glossy_model(sc, oracle, face_normals, akind):
    f, rec, t, _ = oracle_records(sc, oracle, face_normals)
    return glossy_run(sc, rec, sc.rays[3:6], t, akind, f)


def glossy_evaluate(r, eta, full, rot, x, dtype=np.float64):
    """forward, adjoint and tangent of the restatement under x = glossy_ref.test_inputs() masked to the kept samples, as
    tests/test_gpu_glossy.py masks them: a dict in glossy_errors' names"""
    import glossy_ref as G
    w, gi, gv, dn, dw, da, dd = x
    kp = r.keep.reshape(-1, SPP).all(1)
    args = (*r.a, None, w, r.alpha, eta, GLOSSY_K, GLOSSY_SEED, None, full, rot, r.bits, SPP)
    image, value = G.forward(*args, dtype=dtype)
    gm, gw, ga, gd = G.adjoint(*args, gi * kp, gv * r.keep, dtype=dtype)
    dimage, dvalue = G.tangent(*args, dn * r.keep, dw * r.keep, da * r.keep, np.concatenate([dd[:, :-1], dd[:, :1]], 1), dtype=dtype)
    return {"image": image, "value": value, "grad_sh_n": gm, "grad_weight": gw, "grad_alpha": ga, "grad_data": gd, "dimage": dimage,
            "dvalue": dvalue}


def glossy_errors(got, ref, keep):
    """tests/test_gpu_glossy.py's measures: value and image absolute, every derivative relative L2"""
    from row_helpers import _rel
    kp = keep.reshape(-1, SPP).all(1)
    out = {"value": float(np.abs(got["value"] - ref["value"])[keep].max()), "image": float(np.abs(got["image"] - ref["image"])[kp].max()),
           "grad_data": _rel(got["grad_data"], ref["grad_data"]), "dimage": _rel(got["dimage"][kp], ref["dimage"][kp]),
           "dvalue": _rel(got["dvalue"][keep], ref["dvalue"][keep])}
    for k in ("grad_sh_n", "grad_weight", "grad_alpha"):
        out[k] = _rel(got[k][..., keep], ref[k][..., keep])
    return out


def glossy_ray_errors(d, h, r, k, lanes):
    """(sum |d - wo|^2, sum |wo|^2, sum |h - h_ref|^2, sum |h_ref|^2) of draw k on `lanes`: the terms of the relative L2
    error of the ray directions and microfacet normals"""
    return (((d - r.wo[k])[:, lanes] ** 2).sum(), (r.wo[k][:, lanes] ** 2).sum(), ((h - r.h[k])[:, lanes] ** 2).sum(),
            (r.h[k][:, lanes] ** 2).sum())


# ---- the specular row: traces nothing; the directional row's byte, masks and cosines from sh_n and -d, the steep view ---
# The lights are rig("directional", sc) and the byte is the directional row's on the same scene.  What the scenes add over
# tests/test_gpu_specular.py: sh_n changes sign under flip_normals (an unflipped one zeroes every sample), -d and l are
# world-space directions (the object-space ones give another half vector), and the chain to the heights runs through the
# flat or smooth normal's adjoint under to_world.  Roughness: specular_ref.alpha_row("row") on every case and "sharp" on
# SPECULAR_SHARP_ON as well; eta = specular_ref.ETA; the inputs are specular_ref.inputs.  No sample is left out of a
# comparison: every mask comes from the byte and from cosines both sides form in double from the same float32 rows.
SPECULAR_SHARP_ON = ("affine", False)
SPECULAR_BRIGHT = ("zenith", "high", "unnorm")      # the lights under which more than SPECULAR_BRIGHT_SHARE of the samples
SPECULAR_BRIGHT_SHARE = 0.3                         # carry a highlight (tests/test_gpu_specular.py's floor)


def specular_kinds(name, face_normals):
    return ("row", "sharp") if (name, face_normals) == SPECULAR_SHARP_ON else ("row",)


def specular_lit(names, value):
    """{light: the share of samples with a value > 0} of a [K, n] value under the "row" roughness"""
    return {k: float((np.asarray(value)[j] > 0).mean()) for j, k in enumerate(names)}


def specular_evaluate(lights, rec, d, x, akind, vis, dtype=np.float64, weighted=True):
    """forward, tangent and adjoint of the restatement on the records rec under x = specular_ref.inputs(): the namespace
    specular_ref.errors takes"""
    import specular_ref as SP
    return SP.evaluate(lights, rec["sh_n"], d, x, SP.alpha_row(akind, rec["sh_n"].shape[1]), SP.ETA, vis, SPP, dtype, weighted)


def specular_model(sc, oracle, face_normals):
    """model("directional") of the scene with m.lit on it: specular_lit of the restatement's weighted value, the "row" roughness"""
    import specular_ref as SP
    m = model("directional", sc, oracle, face_normals)
    x = SP.inputs(sc.n, SPP, len(m.lights))
    _, value = SP.forward(m.lights, m.rec["sh_n"], sc.rays[3:6], x.w, SP.alpha_row("row", sc.n), SP.ETA, m.vis, SPP)
    m.lit = specular_lit(m.names, value)
    return m


def specular_conditions(sc, pop, lit):
    """what makes (specular, scene) a test: the directional row's conditions as they are, a highlight on more than
    SPECULAR_BRIGHT_SHARE of the samples under the three high lights and on some sample under every light but `below`"""
    conditions("directional", sc, pop)
    for k in SPECULAR_BRIGHT:
        assert lit[k] > SPECULAR_BRIGHT_SHARE, (sc.name, k, lit)
    for k, v in lit.items():
        assert v > 0 or k == "below", (sc.name, k, lit)


def object_direction(sc, d):
    """[3, n]: the unit object-space direction of the world directions d (what a kernel that forgot to_world would use)"""
    q = np.linalg.inv(np.asarray(sc.to_world, np.float64)[:, :3]) @ np.asarray(d, np.float64)
    return q / np.linalg.norm(q, axis=0)


# ---- the medium row: shadow rays that START in free space, on the primary ray, under a world-space top plane -------------
# Three media, defined once in OBJECT space and carried to world: the top origin as a point (for the view from below object
# z becomes max_height - z: the mirror image about the middle of the slab), the top normal as a COVECTOR, through the
# inverse transpose of to_world's linear part, as lighting_scenes.lights carries its lights (object z negated first for
# the view from below).  Under common.affine(4) and common.mirror_shear() a normal carried as a vector is another plane.
# The lights are rig("directional", sc), carried as vectors: <l, N> keeps its object-space sign, so `below` shines into no
# medium and `graze` not into `tilted`.
#   skim    a layer that just covers the relief (object z = max_height): the points lie close over it, raking lights
#           shadow them; the steep view, camera above the plane (u_in > 0, D = 0)
#   tilted  the plane through object (0, 0, 1.15 max_height) with the normal (0.3, -0.2, 2.0); the steep view
#   inside  object z = 3.0 (absolute), over the camera of the oblique view (u_in = 0, D > 0): about a quarter of that view's
#           rays miss the terrain and go on beside and below the sheet, so shadow rays meet it from outside and from underneath
MEDIUM_K, MEDIUM_SEED = 4, 11
MEDIA = {"skim": dict(view="steep", z=1.0, relative=True, normal=(0.0, 0.0, 1.0), sigma_t=1.0, albedo=0.75, g=0.3),
         "tilted": dict(view="steep", z=1.15, relative=True, normal=(0.3, -0.2, 2.0), sigma_t=1.0, albedo=0.6, g=0.5),
         "inside": dict(view="oblique", z=3.0, relative=False, normal=(0.0, 0.0, 1.0), sigma_t=0.5, albedo=0.9, g=-0.2)}
MEDIUM_NAMES = tuple(MEDIA)
MEDIUM_RTOL, MEDIUM_ATOL = 1e-5, 1e-7          # tests/test_gpu_medium.py's rule; the atol times max(1, largest |reference|)


def medium_plane(sc, mname, covector=True):
    """(top_origin, top_normal) of a medium in world space; covector=False carries the normal as a vector: the mistake the
    scenes must tell apart"""
    spec = MEDIA[mname]
    A = np.asarray(sc.to_world, np.float64)
    z = spec["z"] * sc.max_height if spec["relative"] else spec["z"]
    o, nrm = np.array((0.0, 0.0, z)), np.array(spec["normal"], np.float64)
    if sc.below:
        o[2], nrm[2] = sc.max_height - z, -nrm[2]
    return A[:, :3] @ o + A[:, 3], (np.linalg.inv(A[:, :3]).T if covector else A[:, :3]) @ nrm


def medium_of(sc, mname, covector=True):
    """the restatement's medium (medium_ref.medium) of the scene"""
    import medium_ref as MR
    spec = MEDIA[mname]
    o, nrm = medium_plane(sc, mname, covector)
    return MR.medium(spec["sigma_t"], spec["albedo"], spec["g"], o, nrm)


def medium_run(sc, mname, o, d, t, field, words=None, origins=None):
    """one medium on the primary rays (o, d, t) under the rig: the restatement's segment and masks, the K float32 origins
    (`origins` [K, 3, n] = None: the restatement's, formed as the kernel forms them), the oracle's answer on those rays
    (`words` [J, n] = None: the visibility IS the oracle's) and the counts the conditions are about"""
    import medium_ref as MR
    r = types.SimpleNamespace(mname=mname, M=medium_of(sc, mname), K=MEDIUM_K, field=field)
    r.names, r.lights = rig("directional", sc)
    J, n = len(r.lights), len(t)
    o, d, t = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(t)
    r.o, r.d, r.t = o, d, t
    r.q = MR.segment(r.M, o, d, t)
    r.hit = np.isfinite(t)
    r.nu = np.array([MR.nu(r.M, L) for L in r.lights])
    r.shines = r.nu > 0
    first = r.lights[int(np.argmax(r.shines))]
    r.origins64 = np.stack([MR.rays(r.M, first, o, d, t, k, MEDIUM_SEED)[0] for k in range(MEDIUM_K)])
    r.origins32 = np.stack([MR.rays(r.M, first, o, d, t, k, MEDIUM_SEED, dtype=np.float32)[0] for k in range(MEDIUM_K)])
    r.origins = r.origins32 if origins is None else np.asarray(origins, np.float64)
    with np.errstate(invalid="ignore"):
        p = o + np.where(r.hit, t, 0.0).astype(np.float64)[None] * d
        r.near = (r.q.elig & r.hit)[None] & (np.sqrt(((r.origins - p[None]) ** 2).sum(1)) < MR.spawn_offset(p)[None])
    r.p = p
    r.traced = r.shines[:, None] & r.q.elig[None]                                   # [J, n]: the same for every k
    r.oracle = np.zeros((J, MEDIUM_K, n), bool)                                     # visible by the oracle's ray_test
    for j, L in enumerate(r.lights):
        if not r.shines[j]:
            continue
        lf = MR.unit(L)[0].astype(np.float32)
        tr = r.traced[j]
        for k in range(MEDIUM_K):
            r7 = np.concatenate([r.origins[k][:, tr], np.repeat(lf[:, None], int(tr.sum()), 1), np.full((1, int(tr.sum())), np.inf)])
            r.oracle[j, k, tr] = ~field.ray_test(r7.astype(np.float32)).astype(bool)
    r.bits = r.oracle if words is None else np.stack([MR.unpack(w, MEDIUM_K) for w in np.asarray(words)])
    r.words = np.stack([MR.pack(b) for b in r.bits])
    occ = r.traced[:, None] & ~r.bits                                               # [J, K, n]
    r.shares = {}
    for j, name in enumerate(r.names):
        tr = MEDIUM_K * int(r.traced[j].sum())
        r.shares[name] = {"traced": tr, "occluded": int(occ[j].sum()), "occluded_of_traced": float(occ[j].sum() / tr) if tr else 0.0,
                          "occluded_on_misses": int(occ[j][:, ~r.hit].sum())}
    r.counts = {"hit": float(r.hit.mean()), "eligible": float(r.q.elig.mean()), "near": float(r.near.mean()),
                "near_lanes": int(r.near.sum())}
    return r


def medium_conditions(sc, r):
    """what makes (medium, scene) a test; asserted before anything is compared.  The cap on the lanes left out of the
    comparison with the oracle is row_helpers.UNSURE_CAP and is never raised"""
    c, sh, name = r.counts, r.shares, (sc.name, r.mname)
    assert c["near"] <= UNSURE_CAP, (name, c)
    assert 0.05 <= c["hit"] <= 0.95, (name, c)
    assert sh["below"]["traced"] == 0 and (r.mname != "tilted" or sh["graze"]["traced"] == 0), (name, sh)
    lit = {k: v for k, v in sh.items() if v["traced"]}
    assert len(lit) >= 6 and all(0 < v["occluded"] < v["traced"] for v in lit.values()), (name, sh)   # both outcomes
    assert any(v["occluded_of_traced"] <= 0.03 for v in lit.values()), (name, sh)
    if r.mname == "inside":
        assert (r.q.u_in == 0).all() and (r.q.D > 0).all(), name
        assert all(v["occluded_on_misses"] >= 40 for v in lit.values()), (name, sh)
    else:
        assert (r.q.u_in > 0).all(), name
        mixed = [k for k, v in lit.items() if v["traced"] >= 1000 and 0.08 <= v["occluded_of_traced"] <= 0.9]
        assert len(mixed) >= 2, (name, mixed, sh)


def medium_describe(r):
    return "hit %.2f eligible %.2f near %.2e (%d) | " % (r.counts["hit"], r.counts["eligible"], r.counts["near"], r.counts["near_lanes"]) \
        + ", ".join("%s %d/%.3f/%d" % (k, v["traced"], v["occluded_of_traced"], v["occluded_on_misses"]) for k, v in r.shares.items())


def medium_model(sc, oracle, mname):
    """(the scene's medium through the oracle and the restatement only, the oracle's field): the scene must be of the
    medium's view"""
    assert sc.view == MEDIA[mname]["view"]
    f = LS.oracle_field(sc, oracle)
    t = f.ray_intersect_preliminary(sc.rays)[0]
    return medium_run(sc, mname, sc.rays[0:3], sc.rays[3:6], t, f)


def medium_close(got, ref):
    """the row's own rule (tests/test_gpu_medium.py): |got - ref| <= rtol |ref| + atol max(1, largest |ref|); returns the
    largest (|got - ref| - rtol |ref|) / (atol max(1, largest |ref|)): within the rule when <= 1"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) - MEDIUM_RTOL * np.abs(ref)).max() / (MEDIUM_ATOL * max(1.0, np.abs(ref).max())))

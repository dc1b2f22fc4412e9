"""The inputs of tests/test_gpu_row_scenes.py, on the CPU with the oracle and the float64 restatements only
(tests/row_scenes.py and the rows' own directional_ref, spot_ref, caustic_ref, refract_ref, rect_ref, projector_ref,
reflect_ref, glossy_ref): for every (row, scene, shading mode) the conditions that make the triple a test -- the share of
samples that rounding may decide is at most row_helpers.UNSURE_CAP, both outcomes of the visibility are populated -- and
that the emitters were carried to world at all: on these scenes an emitter, lamp, projector or receiver left in object
space gives another answer.  Per row:
  directional, spot: a fully visible light and mixed ones; the spot light `inside` ends its shadow rays inside the field's
      bound, and +inf in place of their maxt changes the oracle's answer on some of them;
  caustic: total internal reflection, occlusion and deposition decide both ways, and on the receiver that cuts the relief
      +inf in place of maxt = s changes at least row_scenes.FLOOR_CHANGED of the oracle's answers;
  refract: the caustic row's conditions on its textured receiver, the shares of lanes inside the texture and near a cell
      border, and the float32 error of a landing position against the border that is left out;
  rect: the floors of its own file on the `side` lamp, whose draws lie inside the field's bound;
  projector: both outcomes under `side`, the frustum of `above` cutting the wavefront;
  reflect: both outcomes of the visibility from the oblique view;
  glossy: both outcomes over its 4 draws, and draws that the row's own masks reject;
  specular: the directional row's conditions and the shares of samples with a highlight; an unflipped sh_n zeroes every
      sample where flip_normals is set, and the object-space ray direction gives another value on `affine`;
  medium, per (scene, medium of row_scenes.MEDIA): at most UNSURE_CAP of the points within the spawn offset of the primary
      hit, occluded shares per light, the camera above or inside the medium, shadow rays of samples that missed the terrain
      occluded from beside and below; the top normal carried as a vector is another plane, and the field under an identity
      to_world answers the shadow rays otherwise.
Last, row_scenes.F32 against the record of scripts/row_scenes_f32_error.py.  Each test prints its shares."""
import json
import math
import os

import numpy as np
import pytest

import row_scenes as RS


@pytest.fixture(scope="module")
def models(oracle):
    cache = {}

    def get(row, name, face_normals):
        key = (row, name, face_normals)
        if key not in cache:
            sc = RS.scene(name, RS.VIEW_OF[row])
            cache[key] = (sc, RS.model(row, sc, oracle, face_normals))
        return cache[key]
    return get


@pytest.mark.parametrize("name,face_normals", RS.CASES)
@pytest.mark.parametrize("row", RS.ROWS)
def test_the_scene_meets_the_conditions_of_the_row(models, row, name, face_normals):
    sc, m = models(row, name, face_normals)
    print(row, name, "face" if face_normals else "smooth", "hits %d eligible %d |" % (np.isfinite(m.t).sum(), m.pop.eligible.sum()),
          RS.describe(m.pop))
    assert m.pop.eligible.sum() >= 1000 and np.abs(m.rec["p"]).max() < 4
    RS.conditions(row, sc, m.pop)


@pytest.mark.parametrize("name", RS.SCENES)
def test_the_spot_light_inside_ends_its_rays_inside_the_bound_over_the_surface(models, oracle, name):
    """the origin of `inside` is in the object-space box, above the surface (a vertical ray from it towards the field hits
    at the extreme vertex), and no other light of the rig is inside the box"""
    sc, m = models("spot", name, True)
    for k, L in zip(m.names, m.lights):
        assert RS.in_bound(sc, L.to_world[:, 3]) == (k == "inside"), k
    c = m.lights[0].to_world[:, 3]
    x, y, z = RS.extreme_vertex(sc)
    A = np.asarray(sc.to_world, np.float64)
    down = A[:, :3] @ np.array((x, y, sc.max_height if sc.below else 0.0)) + A[:, 3] - c
    dist = np.linalg.norm(down)
    r = np.concatenate([c, down / dist, [np.inf]]).astype(np.float32)[:, None]
    t = m.field.ray_intersect_preliminary(r)[0][0]
    gap = (sc.max_height - z) if sc.below else z                    # from the plane the ray aims at to the vertex
    want = dist * (1.0 - gap / (RS.INSIDE_Z * sc.max_height))
    print(name, "`inside` is", t, "over the surface; the lowest vertex says", want)
    assert np.isfinite(t) and abs(t - want) <= 1e-4 and 0.05 < t < dist


@pytest.mark.parametrize("name", RS.SCENES)
@pytest.mark.parametrize("row", RS.ROWS)
def test_an_emitter_left_in_object_space_gives_another_visibility(models, oracle, row, name):
    """the scenes' world is not their object space: the rig as the row's own file has it (object space, not carried) lights
    other samples, on most lights (an unoccluded directional light stays unoccluded: `zenith` and `high` shadow nothing
    either way)"""
    sc, m = models(row, name, True)
    ident = type(sc)(**{**vars(sc), "to_world": RS.LS.IDENTITY, "below": False})
    _, lights = RS.rig(row, ident)
    d = sc.rays[3:6]
    differ = []
    for L in lights:
        r7, tr = RS.shadow_rays(row, L, m.rec, d, m.t)
        v = np.zeros(sc.n, bool)
        v[tr] = ~m.field.ray_test(r7[:, tr]).astype(bool)
        differ.append(v)
    differ = (np.stack(differ) != m.vis).sum(1)
    print(row, name, "samples whose visibility differs per light", differ)
    assert (differ >= 20).sum() >= len(lights) // 2 + 1, differ


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_caustic_row(oracle, name, face_normals):
    sc = RS.scene(name, "oblique")
    runs = RS.caustic_model(sc, oracle, face_normals)
    for (eta, plane), r in runs.items():
        print("caustic", name, "face" if face_normals else "smooth", "eta %.3f %s" % (eta, plane), r.counts)
    assert len(runs) == (4 if face_normals else 2)
    RS.caustic_conditions(sc, runs)
    # a receiver left in object space is another plane: other rays are traced, to another end
    import caustic_ref as C
    ident = type(sc)(**{**vars(sc), "to_world": RS.LS.IDENTITY})
    for (eta, plane), r in runs.items():
        tr, _, _, maxt, _ = C.rays(*r.a, None, eta, C.receiver(*RS.caustic_receiver(ident, plane)))
        both = tr & r.traced
        moved = int((np.abs(maxt - r.maxt)[both] > 1e-3).sum()) + int((tr != r.traced).sum())
        assert moved >= 0.5 * r.counts["traced"], (name, eta, plane, moved)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_rect_row(oracle, name, face_normals):
    sc = RS.scene(name, "steep")
    runs = RS.rect_model(sc, oracle, face_normals)
    for lname, r in runs.items():
        print("rect", name, "face" if face_normals else "smooth", lname, r.counts)
    RS.rect_conditions(sc, runs)
    # a lamp left in object space is seen by other draws
    import rect_ref as A
    d, t = sc.rays[3:6], runs["side"].t
    for lname, r in runs.items():
        lm = A.LAMPS[lname](A.RADIANCE)
        tr, _ = A.traced(r.rec["sh_n"], d, t, A.geometry(r.rec["p"], r.rec["sh_n"], r.draws, lm))
        bits = np.zeros_like(tr)
        for k in range(RS.RECT_K):
            o, w, maxt, _ = A.rays(r.rec["p"], r.rec["n"], r.rec["sh_n"], d, t, r.ids, k, RS.RECT_SEED, lm)
            r7 = np.concatenate([o, w, maxt[None]]).astype(np.float32)[:, tr[k]]
            bits[k, tr[k]] = ~r.field.ray_test(r7).astype(bool)
        print("rect", name, lname, "draws whose visibility differs with the lamp left in object space", int((bits != r.bits).sum()))
        assert (bits != r.bits).sum() >= 0.05 * r.counts["traced"], (name, lname, int((bits != r.bits).sum()))
    # every draw of `side` lies inside the field's box or next to it; none of `above` does
    assert runs["above"].counts["ends_inside"] == 0 and runs["side"].counts["ends_inside"] >= 0.5 * runs["side"].counts["traced"]


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_projector_row(oracle, name, face_normals):
    sc = RS.scene(name, "steep")
    runs, rec, t = RS.projector_model(sc, oracle, face_normals)
    for pname, r in runs.items():
        print("projector", name, "face" if face_normals else "smooth", pname, {k: round(v, 4) for k, v in r.counts.items()})
    RS.projector_conditions(sc, runs)
    # a projector left in object space sees other samples
    import projector_ref as PR
    for pname, r in runs.items():
        tr, _ = PR.traced(PR.PROJECTORS[pname](), rec["p"], rec["sh_n"], sc.rays[3:6], t)
        assert (tr != r.traced).sum() >= 100, (name, pname, int((tr != r.traced).sum()))


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_reflect_row(oracle, name, face_normals):
    sc = RS.scene(name, "oblique")
    r, rec, t = RS.reflect_model(sc, oracle, face_normals)
    print("reflect", name, "face" if face_normals else "smooth", r.counts)
    RS.reflect_conditions(sc, r)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_refract_row(oracle, name, face_normals):
    sc = RS.scene(name, "oblique")
    runs = RS.refract_model(sc, oracle, face_normals)
    for (eta, plane), r in runs.items():
        print("refract", name, "face" if face_normals else "smooth", "eta %.3f %s" % (eta, plane), r.counts)
    RS.refract_conditions(sc, runs)
    assert 4 * RS.F32["refract"]["pos"] < RS.REFRACT_BORDER            # (what leaving out the lanes within BORDER rests on)
    # a receiver left in object space reads other texels
    import refract_ref as RR
    tex = RR.textures(*RS.REFRACT_TEX)["random"]
    ident = type(sc)(**{**vars(sc), "to_world": RS.LS.IDENTITY})
    for (eta, plane), r in runs.items():
        v0 = RR.forward(*r.a, None, None, eta, 0.0, r.rref, tex, RR.REPEAT, r.vis)[0]
        v1 = RR.forward(*r.a, None, None, eta, 0.0, RR.receiver(*RS.refract_receiver(ident, plane)), tex, RR.REPEAT, r.vis)[0]
        assert (np.abs(v0 - v1) > 1e-3).sum() >= 0.5 * r.counts["deposited"], (name, eta, plane)


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_glossy_row(oracle, name, face_normals):
    sc = RS.scene(name, "oblique")
    for akind, _, _ in RS.GLOSSY_COMBOS:
        r = RS.glossy_model(sc, oracle, face_normals, akind)
        print("glossy", name, "face" if face_normals else "smooth", "alpha", akind, r.counts)
        RS.glossy_conditions(sc, r)
        assert r.counts["untraced_of_eligible_draws"] >= 100            # the draws' own masks decide both ways too


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_scene_meets_the_conditions_of_the_specular_row(oracle, name, face_normals):
    """the directional row's conditions, the shares of samples with a highlight, and what the scene adds: an unflipped sh_n
    zeroes every sample where flip_normals is set, and the object-space ray direction gives another value on `affine`"""
    import specular_ref as SP
    sc = RS.scene(name, "steep")
    m = RS.specular_model(sc, oracle, face_normals)
    print("specular", name, "face" if face_normals else "smooth", RS.describe(m.pop), "| lit", {k: round(v, 3) for k, v in m.lit.items()})
    RS.specular_conditions(sc, m.pop, m.lit)
    d, n = sc.rays[3:6], sc.n
    x = SP.inputs(n, RS.SPP, len(m.lights))
    a = lambda sh_n, dd: SP.forward(m.lights, sh_n, dd, x.w, SP.alpha_row("row", n), SP.ETA, m.vis, RS.SPP)[1]
    value = a(m.rec["sh_n"], d)
    if sc.flip:
        assert value.max() > 0.05 and not a(-m.rec["sh_n"], d).any(), name              # the unflipped sh_n: all zero
    if name == "affine":
        # The object-space direction is 2.7 degrees off the world one here.  Most highlights are faint (a median value of
        # 1e-3 to 2e-2 under a largest one of 1.5 to 2.1), so "by more than the tolerance" is taken of each lit (light,
        # sample) pair's own value: that holds on 99 % of them.  In the row's own measure -- the largest difference over
        # max(1, the largest value), which is what tests/test_gpu_row_scenes.py holds the kernel to -- the mistake is a
        # thousand tolerances; 20 % (flat) and 28 % (smooth) of the lit pairs move by more than the tolerance in that
        # absolute sense, which is printed and not asserted as "most"
        tol = RS.TOL["specular"]["row"]["value"]
        lit = value > 0
        other = a(m.rec["sh_n"], RS.object_direction(sc, d))
        moved = np.abs(other - value) > tol * value
        far = np.abs(other - value) > tol * max(1.0, value.max())
        measure = SP.err_abs(other, value)
        print("specular", name, "the object-space direction moves %d of %d lit (light, sample) pairs by more than the tolerance of their own "
              "value, %d by more than the tolerance of the largest; in the row's measure %.3g / %.3g" % (moved[lit].sum(), lit.sum(), far[lit].sum(), measure, tol))
        assert moved[lit].mean() > 0.5 and far[lit].mean() > 0.1 and measure > 100 * tol, (moved[lit].mean(), far[lit].mean(), measure)


@pytest.mark.parametrize("mname", RS.MEDIUM_NAMES)
@pytest.mark.parametrize("name", RS.SCENES)
def test_the_scene_meets_the_conditions_of_the_medium_row(oracle, name, mname):
    """the conditions of (scene, medium), and that the scene tells a plausible mistake from the right answer: the top normal
    carried as a vector is another plane, and the shadow rays traced against the field with an identity to_world give
    other bits"""
    import medium_ref as MR
    sc = RS.scene(name, RS.MEDIA[mname]["view"])
    r = RS.medium_model(sc, oracle, mname)
    print("medium", name, mname, RS.medium_describe(r))
    RS.medium_conditions(sc, r)
    # (the binade the origin's tolerance rests on: on `inside` the points of rays that miss the terrain lie up to 9.5 out)
    assert np.abs(r.origins64[:, :, r.q.elig]).max() < 16
    if mname == "tilted" and name in ("affine", "mirror_flip"):
        wrong = MR.segment(RS.medium_of(sc, mname, covector=False), r.o, r.d, r.t)
        moved = np.abs(wrong.u_in - r.q.u_in) > 1e-3
        print("medium", name, mname, "samples whose u_in the normal carried as a vector moves by more than 1e-3: %d of %d" % (moved.sum(), sc.n))
        assert moved.mean() > 0.5, moved.mean()
    ident = oracle.OracleField(sc.h, max_height=sc.max_height, to_world=RS.LS.IDENTITY, flip_normals=sc.flip)
    other = RS.medium_run(sc, mname, r.o, r.d, r.t, ident)
    changed = int((other.bits != r.bits).sum())
    print("medium", name, mname, "bits that the field under an identity to_world changes:", changed)
    assert changed >= 100, (name, mname, changed)


def _cut(x):
    e = math.floor(math.log10(x))
    return math.floor(x / 10.0 ** (e - 2)) * 10.0 ** (e - 2)


def test_the_tolerances_are_the_recorded_float32_errors_cut_after_three_digits():
    """row_scenes.F32 against profiles/row_scenes/f32_error.json, the record of scripts/row_scenes_f32_error.py (the specular
    row has a dict per roughness row)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = json.load(open(os.path.join(root, "profiles", "row_scenes", "f32_error.json")))
    assert set(RS.F32) == set(rec), (set(RS.F32), set(rec))
    for row in RS.F32:
        pairs = [(row, RS.F32[row], rec[row]["maxima"])]
        if row == "specular":
            assert set(RS.F32[row]) == set(rec[row]["maxima"]) == {"row", "sharp"}
            pairs = [((row, kind), RS.F32[row][kind], rec[row]["maxima"][kind]) for kind in RS.F32[row]]
        for what, f32, worst in pairs:
            assert set(f32) == {k[4:] for k in worst}, what
            for k, v in f32.items():
                cut = _cut(worst["err_" + k])
                assert abs(v - cut) <= 1e-6 * cut, (what, k, v, worst["err_" + k])
    for row, tol in RS.TOL.items():                                                    # the GPU is allowed four times that
        for kind, d in (tol.items() if row == "specular" else ((None, tol),)):
            f32 = RS.F32[row] if kind is None else RS.F32[row][kind]
            assert d == {k: 4 * v for k, v in f32.items()}, (row, kind)

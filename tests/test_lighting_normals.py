"""The scenes of tests/lighting_scenes.py with a shading normal that is NOT the geometric normal, on the CPU with the
oracle and the float64 restatements only (sky_ref, bounce_ref, envmap_ref, smooth_ref): the populations that make
tests/test_gpu_lighting_normals.py a test of which of the two normals a lighting kernel uses for what.  Two kinds of sh_n:
`smooth` (smooth_ref.surface: the blended vertex normals of face_normals = false) and `bent` (n turned by 26.6 degrees
about a random tangent on every hit: lighting_scenes.bent_normals).  With sh_n = n every population below is empty.

Like test_lighting_scenes.py this is about the inputs, not the kernels.  A configuration that misses a floor is dropped
from CONFIGS / ENV_CONFIGS here and says so; the floors do not move.  None is dropped: all eight (scene, kind) and all
twelve (scene, map, kind) meet every floor, and the float32 normals of the GPU give the very same counts.

Measured (2300 samples, K = 4, seed 5, ids = position; `below`: <n, w> < -MARGIN, `above`: <n, w> > MARGIN):

  sky and bounce                  sky: traced   of those     of those   not traced | bounce: traced  of those  hits seen    | eligibility
  scene        kind    eligible        below    unoccluded   occluded   above      |         below   hit       from behind  | differs from n's
  affine       smooth  2127            569      36           533        610        |         468     455       455          | 0
  affine       bent    2041            607      237          370        638        |         402     243       243          | 86
  mirror_flip  smooth  2126            886      36           850        911        |         986     962       966          | 0
  mirror_flip  bent    2017            599      215          384        624        |         453     293       297          | 109
  flip_below   smooth  2155            546      34           512        543        |         402     384       384          | 0
  flip_below   bent    2078            612      268          344        606        |         419     266       266          | 77
  rand8        smooth  2121            895      60           835        918        |         1065    1033      1033         | 0
  rand8        bent    2045            613      248          365        599        |         402     247       247          | 76
  floor                                200      10           10         100        |         200     100       100          | 40 (bent)

  envmap                          (sun, 0.25): traced  of those    not traced | (gradient, 0.0): traced  of those    not traced
  scene        kind                            below   unoccluded  above      |                  below   unoccluded  above
  affine       smooth                          713     21          224        |                  540     26          569
  affine       bent                            452     72          737        |                  570     172         599
  mirror_flip  smooth                          1889    30          343        |                  1026    45          796
  mirror_flip  bent                            717     72          647        |                  575     162         641
  rand8        smooth                          1000    42          294        |                  979     52          837
  rand8        bent                            470     78          568        |                  576     222         616
  floor                                        200     10          100        |                  200     10          100

The angle between sh_n and n: `bent` 26.565 degrees on every hit; `smooth` 0.5 to 91 degrees, median 23 to 39.  Lanes
decided within MARGIN (eligibility, the hemisphere test, the side of the spawn offset): at most 1 of 9200 per row and
configuration (1.1e-4; the bound is 1e-3).  max |p| is at most 1.83 (the bound is 4).
"""
import numpy as np
import pytest

import lighting_scenes as LS
from lighting_scenes import MARGIN  # noqa: F401  (the margin of `undecided`)

CONFIGS = [(s, k) for s in LS.NAMES for k in LS.KINDS]
ENV_CONFIGS = [(s, m, u, k) for s in LS.ENV_SCENES for m, u in LS.ENV_MAPS for k in LS.KINDS]
_MODELS = {}


def model(oracle, scene, kind):
    """normals_model of (scene, kind) with the envmap row's maps where the scene has them, once per session"""
    if (scene, kind) not in _MODELS:
        _MODELS[scene, kind] = LS.normals_model(LS.scene(scene), oracle, kind, LS.ENV_MAPS if scene in LS.ENV_SCENES else ())
    return _MODELS[scene, kind]


def check_shadow_row(c):
    """the floors of a row of shadow rays (sky, envmap)"""
    assert c["traced_below"] >= LS.FLOOR_BELOW and c["above_untraced"] >= LS.FLOOR_ABOVE
    assert c["below_unoccluded"] >= LS.FLOOR_OUTCOME and c["below_occluded"] >= LS.FLOOR_OUTCOME
    assert c["undecided"] <= 1e-3


@pytest.mark.parametrize("scene,kind", CONFIGS, ids=lambda x: str(x))
def test_sky_and_bounce_populations(oracle, scene, kind):
    m = model(oracle, scene, kind)
    print(scene, kind, m.common, "\n   sky", m.sky, "\n   bounce", m.bounce)
    assert m.common["max_p"] < 4                                           # (what the 1e-6 on origins rests on)
    check_shadow_row(m.sky)
    b = m.bounce
    assert b["traced_below"] >= LS.FLOOR_BELOW and b["below_hit"] >= LS.FLOOR_BOUNCE_HIT
    assert b["hit_from_behind"] >= LS.FLOOR_BEHIND and b["undecided"] <= 1e-3
    if kind == "bent":
        assert m.common["eligibility_differs"] >= LS.FLOOR_ELIGIBILITY
        assert abs(m.common["angle_deg"][0] - 26.565) < 0.01 and abs(m.common["angle_deg"][2] - 26.565) < 0.01


@pytest.mark.parametrize("scene,name,u,kind", ENV_CONFIGS, ids=lambda x: str(x))
def test_envmap_populations(oracle, scene, name, u, kind):
    c = model(oracle, scene, kind).env[(name, u)]
    print(scene, name, u, kind, c)
    check_shadow_row(c)

"""The thin lens (hf_thinlens_rays, _tangent, _adjoint, hf_thinlens_project, _tangent, _adjoint) on the CPU: the entry
points are declared, exported and bound, HF_VERSION and hf_sensor_t's layout are unchanged, and every bad argument is
refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C

import pytest

import sensor_ref as R
from abi_helpers import assert_refused, assert_symbols, stand_ins

RAYS = ("hf_thinlens_rays", "hf_thinlens_rays_tangent", "hf_thinlens_rays_adjoint")
PROJECT = ("hf_thinlens_project", "hf_thinlens_project_tangent", "hf_thinlens_project_adjoint")
NAN, INF = float("nan"), float("inf")
POSE = R.look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0))[:3].reshape(-1)


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(RAYS + PROJECT + ("hf_thinlens_workspace_floats",), ("ThinLensCamera",))
    assert "hf_thinlens_t" in hdr and "HF_THINLENS_PAIR" in hdr and "0x4C454E53u" in hdr
    from hf_amd import _capi
    assert _capi.HF_THINLENS_PAIR == 0x4C454E53 and not 0 <= _capi.HF_THINLENS_PAIR < 32
    assert _capi.lib().hf_thinlens_workspace_floats() * 13 == _capi.lib().hf_sensor_workspace_floats() * 15
    assert C.sizeof(_capi.hf_sensor_t) == 4 + 6 * 4 + 4 + 15 * 8          # as before
    assert C.sizeof(_capi.hf_thinlens_t) == C.sizeof(_capi.hf_sensor_t) + 16
    assert _capi.hf_thinlens_t.aperture_radius.offset == C.sizeof(_capi.hf_sensor_t)


def _lens(type=0, film=(13, 7), crop=(3, 2, 5, 4), to_world=POSE, fov=40.0, near=1e-2, far=1e4, tw=None, radius=0.1, focus=2.0):
    from hf_amd import _capi
    m = list(to_world)
    for j, v in (tw or {}).items():
        m[j] = v
    return _capi.hf_thinlens_t(_capi.hf_sensor_t(type, *film, *crop, (C.c_double * 12)(*m), fov, near, far), radius, focus)


def _call(lib, fn, n=8, start=0, spp=2, null=(), null_row=None, **kw):
    rows, arg = stand_ins(null, null_row)
    s = None if "lens" in null else C.byref(_lens(**kw))
    head = (s, n, start, spp, 7, arg("ray_id"))
    if fn == "hf_thinlens_rays":
        return lib.hf_thinlens_rays(*head, rows("out_o"), rows("out_d"), arg("out_maxt"), rows("out_pos", 2), None)
    if fn == "hf_thinlens_rays_tangent":
        return lib.hf_thinlens_rays_tangent(*head, arg("d_to_world"), arg("d_fov"), arg("d_radius"), arg("d_focus"),
                                            rows("out_do"), rows("out_dd"), None)
    if fn == "hf_thinlens_rays_adjoint":
        return lib.hf_thinlens_rays_adjoint(*head, rows("grad_o"), rows("grad_d"), arg("grad_to_world"), arg("grad_fov"),
                                            arg("grad_radius"), arg("grad_focus"), arg("workspace"), None)
    head = (s, n, start, 7, arg("ray_id"), rows("p"), arg("active"))
    if fn == "hf_thinlens_project":
        return lib.hf_thinlens_project(*head, rows("uv", 2), arg("valid"), arg("weight"), None)
    if fn == "hf_thinlens_project_tangent":
        return lib.hf_thinlens_project_tangent(*head, rows("dp"), arg("d_to_world"), arg("d_fov"), arg("d_radius"),
                                               arg("d_focus"), rows("duv", 2), arg("dweight"), None)
    return lib.hf_thinlens_project_adjoint(*head, rows("grad_uv", 2), arg("grad_weight"), rows("grad_p"), arg("grad_to_world"),
                                           arg("grad_fov"), arg("grad_radius"), arg("grad_focus"), arg("workspace"), None)


# everything hf_sensor_rays refuses for a perspective sensor (the tables of tests/test_sensor_abi.py) ...
SENSOR = [{"null": ("lens",)}, {"type": 2}, {"type": -1}, {"n": 1 << 32},
          {"crop": (3, 2, 0, 4)}, {"crop": (3, 2, 5, 0)}, {"crop": (9, 2, 5, 4)}, {"crop": (3, 4, 5, 4)}, {"film": (0, 7)},
          {"crop": (0xFFFFFFFF, 2, 5, 4)},
          {"tw": {0: NAN}}, {"tw": {7: INF}}, {"tw": {11: -INF}}, {"near": NAN}, {"far": INF},
          {"near": 0.0}, {"near": -1.0}, {"near": 2.0, "far": 2.0}, {"near": 2.0, "far": 1.0}]
PERSP = [{"fov": NAN}, {"fov": 0.0}, {"fov": 180.0}, {"fov": -10.0}, {"fov": 200.0},
         {"tw": {0: POSE[0] * 1.01, 4: POSE[4] * 1.01, 8: POSE[8] * 1.01}},          # a scaled x axis
         {"tw": {1: POSE[1] + 0.01}}]                                                # a sheared one
WAVEFRONT = [{"spp": 0}, {"start": 0xFFFFFFFF, "n": 2, "null": ("ray_id",)},
             {"film": (1 << 16, 1 << 16), "crop": (0, 0, 1 << 16, 1 << 16), "spp": 2, "null": ("ray_id",)},
             {"film": (1 << 17, 1 << 17), "crop": (0, 0, 1 << 17, 1 << 17), "spp": 1, "null": ("ray_id",)}]
# ... and the lens's own: an orthographic base, the radius, the focus distance
LENS = [{"type": 1}, {"radius": NAN}, {"radius": INF}, {"radius": -1e-9}, {"radius": -INF},
        {"focus": NAN}, {"focus": INF}, {"focus": 0.0}, {"focus": -2.0}]
COMMON = SENSOR + PERSP + LENS
PSTART = [{"start": 0xFFFFFFFF, "n": 2, "null": ("ray_id",)}]
CASES = {
    "hf_thinlens_rays": COMMON + WAVEFRONT + [{"null": (x,)} for x in ("out_o", "out_d", "out_maxt")] +
                        [{"null_row": x} for x in ("out_o", "out_d", "out_pos")],
    "hf_thinlens_rays_tangent": COMMON + WAVEFRONT + [{"null": ("out_do",)}, {"null": ("out_dd",)}, {"null_row": "out_do"},
                                                      {"null_row": "out_dd"}],
    "hf_thinlens_rays_adjoint": COMMON + WAVEFRONT + [{"null": ("workspace",)}, {"null_row": "grad_o"}, {"null_row": "grad_d"}],
    "hf_thinlens_project": COMMON + PSTART + [{"null": ("p",)}, {"null_row": "p"}, {"null": ("uv",)}, {"null_row": "uv"},
                                              {"null": ("valid",)}],
    "hf_thinlens_project_tangent": COMMON + PSTART + [{"null": ("p",)}, {"null_row": "p"}, {"null": ("duv",)},
                                                      {"null_row": "duv"}, {"null_row": "dp"}],
    "hf_thinlens_project_adjoint": COMMON + PSTART + [{"null": ("p",)}, {"null_row": "p"}, {"null": ("workspace",)},
                                                      {"null_row": "grad_uv"}, {"null_row": "grad_p"}],
}
MESSAGE = {"null": "", "null_row": "NULL", "type": "", "n": "2^32", "crop": "crop window", "film": "", "tw": "to_world",
           "near": "near_clip", "far": "far_clip", "fov": "x_fov", "spp": "spp", "start": "2^32",
           "radius": "aperture_radius", "focus": "focus_distance"}


@pytest.mark.parametrize("fn", RAYS + PROJECT)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_optional_pointers_an_empty_wavefront_and_the_pinhole_are_not_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    opt = {"hf_thinlens_rays": ("ray_id", "out_pos"),
           "hf_thinlens_rays_tangent": ("ray_id", "d_to_world", "d_fov", "d_radius", "d_focus"),
           "hf_thinlens_rays_adjoint": ("ray_id", "grad_o", "grad_d", "grad_to_world", "grad_fov", "grad_radius", "grad_focus"),
           "hf_thinlens_project": ("ray_id", "active", "weight"),
           "hf_thinlens_project_tangent": ("ray_id", "active", "dp", "d_to_world", "d_fov", "d_radius", "d_focus", "dweight"),
           "hf_thinlens_project_adjoint": ("ray_id", "active", "grad_uv", "grad_weight", "grad_p", "grad_to_world", "grad_fov",
                                           "grad_radius", "grad_focus")}
    for fn, null in opt.items():
        assert _call(lib, fn, n=0, null=null) == _capi.HF_OK, (fn, lib.hf_last_error_string().decode())
        assert _call(lib, fn, n=0, radius=0.0) == _capi.HF_OK, (fn, lib.hf_last_error_string().decode())
    assert _call(lib, "hf_thinlens_rays", n=0, start=0xFFFFFFFF, null=("ray_id",)) == _capi.HF_OK


def test_an_unaligned_workspace_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    rows, arg = stand_ins()
    s = _lens()
    assert lib.hf_thinlens_rays_adjoint(C.byref(s), 8, 0, 2, 7, None, rows("grad_o"), rows("grad_d"), arg("g"), arg("g"), arg("g"),
                                        arg("g"), arg("workspace", 4), None) == _capi.HF_EINVAL
    assert "8-byte aligned" in lib.hf_last_error_string().decode()
    assert lib.hf_thinlens_project_adjoint(C.byref(s), 8, 0, 7, None, rows("p"), None, rows("grad_uv", 2), arg("g"), rows("grad_p"),
                                           arg("g"), arg("g"), arg("g"), arg("g"), arg("workspace", 4), None) == _capi.HF_EINVAL
    assert "8-byte aligned" in lib.hf_last_error_string().decode()


def test_the_camera_holds_what_it_is_given():
    import hf_amd
    cam = hf_amd.ThinLensCamera.look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0), 40.0, 0.25, 1.5, film=(13, 7),
                                        crop=(3, 2, 5, 4))
    s = cam._lens_struct(cam.to_world, cam.fov, cam.aperture_radius, cam.focus_distance)
    b = s.base
    assert (b.type, b.film_w, b.film_h, b.crop_x, b.crop_y, b.crop_w, b.crop_h) == (0, 13, 7, 3, 2, 5, 4)
    assert list(b.to_world[:]) == list(POSE) and (b.x_fov, b.near_clip, b.far_clip) == (40.0, 1e-2, 1e4)
    assert (s.aperture_radius, s.focus_distance) == (0.25, 1.5)

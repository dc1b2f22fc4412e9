"""The sensor (hf_sensor_rays, _tangent, _adjoint, hf_sensor_project, _tangent, _adjoint) on the CPU: the entry points are
declared, exported and bound, HF_VERSION is unchanged, the Python names are callable, and every bad argument is refused
with HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C

import numpy as np
import pytest

import sensor_ref as R
from abi_helpers import assert_refused, assert_symbols, stand_ins

RAYS = ("hf_sensor_rays", "hf_sensor_rays_tangent", "hf_sensor_rays_adjoint")
PROJECT = ("hf_sensor_project", "hf_sensor_project_tangent", "hf_sensor_project_adjoint")
NAN, INF = float("nan"), float("inf")
POSE = R.look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0))[:3].reshape(-1)


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(RAYS + PROJECT + ("hf_sensor_workspace_floats",), ("PerspectiveCamera", "OrthographicCamera"))
    assert "hf_sensor_t" in hdr and "HF_SENSOR_PERSPECTIVE" in hdr and "HF_SENSOR_ORTHOGRAPHIC" in hdr
    from hf_amd import _capi
    assert _capi.lib().hf_sensor_workspace_floats() > 0
    assert C.sizeof(_capi.hf_sensor_t) == 4 + 6 * 4 + 4 + 15 * 8   # (4 bytes of padding before the doubles)


def _sensor(type=0, film=(13, 7), crop=(3, 2, 5, 4), to_world=POSE, fov=40.0, near=1e-2, far=1e4, tw=None):
    from hf_amd import _capi
    m = list(to_world)
    for j, v in (tw or {}).items():
        m[j] = v
    return _capi.hf_sensor_t(type, *film, *crop, (C.c_double * 12)(*m), fov, near, far)


def _call(lib, fn, n=8, start=0, spp=2, null=(), null_row=None, **kw):
    rows, arg = stand_ins(null, null_row)
    s = None if "sensor" in null else C.byref(_sensor(**kw))
    head = (s, n, start, spp, 7, arg("ray_id"))
    if fn == "hf_sensor_rays":
        return lib.hf_sensor_rays(*head, rows("out_o"), rows("out_d"), arg("out_maxt"), rows("out_pos", 2), None)
    if fn == "hf_sensor_rays_tangent":
        return lib.hf_sensor_rays_tangent(*head, arg("d_to_world"), arg("d_fov"), rows("out_do"), rows("out_dd"), None)
    if fn == "hf_sensor_rays_adjoint":
        return lib.hf_sensor_rays_adjoint(*head, rows("grad_o"), rows("grad_d"), arg("grad_to_world"), arg("grad_fov"),
                                          arg("workspace"), None)
    head = (s, n, rows("p"), arg("active"))
    if fn == "hf_sensor_project":
        return lib.hf_sensor_project(*head, rows("uv", 2), arg("valid"), arg("weight"), None)
    if fn == "hf_sensor_project_tangent":
        return lib.hf_sensor_project_tangent(*head, rows("dp"), arg("d_to_world"), arg("d_fov"), rows("duv", 2), arg("dweight"), None)
    return lib.hf_sensor_project_adjoint(*head, rows("grad_uv", 2), arg("grad_weight"), rows("grad_p"), arg("grad_to_world"),
                                         arg("grad_fov"), arg("workspace"), None)


# what every entry refuses of a sensor; the perspective-only ones last
SENSOR = [{"null": ("sensor",)}, {"type": 2}, {"type": -1}, {"n": 1 << 32},
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
CASES = {
    "hf_sensor_rays": SENSOR + PERSP + WAVEFRONT + [{"null": (x,)} for x in ("out_o", "out_d", "out_maxt")] +
                      [{"null_row": x} for x in ("out_o", "out_d", "out_pos")],
    "hf_sensor_rays_tangent": SENSOR + PERSP + WAVEFRONT + [{"null": ("out_do",)}, {"null": ("out_dd",)}, {"null_row": "out_do"},
                                                            {"null_row": "out_dd"}],
    "hf_sensor_rays_adjoint": SENSOR + PERSP + WAVEFRONT + [{"null": ("workspace",)}, {"null_row": "grad_o"}, {"null_row": "grad_d"}],
    "hf_sensor_project": SENSOR + PERSP + [{"type": 1}, {"null": ("p",)}, {"null_row": "p"}, {"null": ("uv",)}, {"null_row": "uv"},
                                           {"null": ("valid",)}],
    "hf_sensor_project_tangent": SENSOR + PERSP + [{"type": 1}, {"null": ("p",)}, {"null_row": "p"}, {"null": ("duv",)},
                                                   {"null_row": "duv"}, {"null_row": "dp"}],
    "hf_sensor_project_adjoint": SENSOR + PERSP + [{"type": 1}, {"null": ("p",)}, {"null_row": "p"}, {"null": ("workspace",)},
                                                   {"null_row": "grad_uv"}, {"null_row": "grad_p"}],
}
MESSAGE = {"null": "", "null_row": "NULL", "type": "", "n": "2^32", "crop": "crop window", "film": "", "tw": "to_world",
           "near": "near_clip", "far": "far_clip", "fov": "x_fov", "spp": "spp", "start": "2^32"}


@pytest.mark.parametrize("fn", RAYS + PROJECT)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_the_orthographic_type_reads_neither_x_fov_nor_the_scale_rule():
    """an orthographic sensor's to_world scales the view and its x_fov is not read: what the perspective type refuses
    passes (the calls stop at the LAST check made on the host, a NULL output), but a to_world without a z axis does not"""
    from hf_amd import _capi
    lib = _capi.lib()
    for fn, out in zip(RAYS, ("out_maxt", "out_do", "workspace")):
        for kw in PERSP:
            assert _call(lib, fn, type=1, null=(out,), **kw) == _capi.HF_EINVAL
            assert "NULL" in lib.hf_last_error_string().decode(), (fn, kw)
        assert _call(lib, fn, type=1, tw={2: 0.0, 6: 0.0, 10: 0.0}) == _capi.HF_EINVAL
        assert "z axis" in lib.hf_last_error_string().decode()


def test_optional_pointers_and_an_empty_wavefront_are_not_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    opt = {"hf_sensor_rays": ("ray_id", "out_pos"), "hf_sensor_rays_tangent": ("ray_id", "d_to_world", "d_fov"),
           "hf_sensor_rays_adjoint": ("ray_id", "grad_o", "grad_d", "grad_to_world", "grad_fov"),
           "hf_sensor_project": ("active", "weight"), "hf_sensor_project_tangent": ("active", "dp", "d_to_world", "d_fov", "dweight"),
           "hf_sensor_project_adjoint": ("active", "grad_uv", "grad_weight", "grad_p", "grad_to_world", "grad_fov")}
    for fn, null in opt.items():
        assert _call(lib, fn, n=0, null=null) == _capi.HF_OK, (fn, lib.hf_last_error_string().decode())
    # with ray_id the wavefront's size is the caller's business
    assert _call(lib, "hf_sensor_rays", n=0, start=0xFFFFFFFF, film=(1 << 17, 1 << 17), crop=(0, 0, 1 << 17, 1 << 17)) == _capi.HF_OK
    # start + n = 2^32 exactly is the last index 2^32 - 1: legal
    assert _call(lib, "hf_sensor_rays", n=0, start=0xFFFFFFFF, null=("ray_id",)) == _capi.HF_OK


def test_an_unaligned_workspace_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    rows, arg = stand_ins()
    s = _sensor()
    assert lib.hf_sensor_rays_adjoint(C.byref(s), 8, 0, 2, 7, None, rows("grad_o"), rows("grad_d"), arg("g"), arg("g"),
                                      arg("workspace", 4), None) == _capi.HF_EINVAL
    assert "8-byte aligned" in lib.hf_last_error_string().decode()
    assert lib.hf_sensor_project_adjoint(C.byref(s), 8, rows("p"), None, rows("grad_uv", 2), arg("g"), rows("grad_p"), arg("g"),
                                         arg("g"), arg("workspace", 4), None) == _capi.HF_EINVAL
    assert "8-byte aligned" in lib.hf_last_error_string().decode()


def test_cameras_hold_what_they_are_given():
    import hf_amd
    cam = hf_amd.PerspectiveCamera.look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0), 40.0, film=(13, 7), crop=(3, 2, 5, 4))
    s = cam._struct(cam.to_world, cam.fov)
    assert (s.type, s.film_w, s.film_h, s.crop_x, s.crop_y, s.crop_w, s.crop_h) == (0, 13, 7, 3, 2, 5, 4)
    assert np.array_equal(np.asarray(s.to_world[:]), POSE) and (s.x_fov, s.near_clip, s.far_clip) == (40.0, 1e-2, 1e4)
    o = hf_amd.OrthographicCamera.look_at((1.5, 1.5, 1.5), (0.0, 0.0, 0.125), (0.0, 0.0, 1.0), scale=(1.6, 1.6, 1.0), film=(16, 8))
    s = o._struct(o.to_world, o.fov)
    want = hf_amd.workload.look_at((1.5, 1.5, 1.5), (0.0, 0.0, 0.125), (0.0, 0.0, 1.0)) @ np.diag([1.6, 1.6, 1.0, 1.0])
    assert s.type == 1 and (s.crop_x, s.crop_y, s.crop_w, s.crop_h) == (0, 0, 16, 8)
    assert np.array_equal(np.asarray(s.to_world[:]), want[:3].reshape(-1))
    assert not hasattr(o, "sample_direction")

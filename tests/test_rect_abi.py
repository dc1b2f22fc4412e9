"""Area-light lighting (hf_rect_rays, hf_rect_lighting, _adjoint, _tangent, hf_rect_light_geometry) on the CPU: the entry
points are declared, exported and bound, HF_VERSION is unchanged, the three Python names are callable, and every bad
argument is refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device
pointers)."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_rect_rays", "hf_rect_lighting", "hf_rect_lighting_adjoint", "hf_rect_lighting_tangent")
NAN, INF = float("nan"), float("inf")
LAMP = ((0.2, -0.1, 1.1), (0.0, 0.2, 0.0), (0.3, 0.0, 0.05), 1.5)


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_rect_light_geometry",), ("RectLight", "rect_lighting", "rect_rays"))
    assert "hf_rect_light_t" in hdr


def _lamp(light):
    from hf_amd import _capi
    return None if light is None else _capi.hf_rect_light_t(*((C.c_float * 3)(*v) for v in light[:3]), light[3])


def _call(lib, fn, n=8, spp=1, num_rays=8, k=0, albedo=0.8, light=LAMP, TW=16, TH=8, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    lamp = _lamp(light)
    if fn == "hf_rect_rays":
        return lib.hf_rect_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), k, 7, arg("ray_id"), lamp,
                                rows("out_o"), rows("out_d"), arg("out_maxt"), None)
    mid = (arg("weight"), num_rays, 7, arg("ray_id"), lamp, TW, TH, arg("tex"), albedo)
    if fn == "hf_rect_lighting":
        return lib.hf_rect_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                    arg("image"), arg("vis_bits"), None)
    head = (n, spp, rows("p"), rows("sh_n"), rows("d"), arg("t"))
    if fn == "hf_rect_lighting_adjoint":
        return lib.hf_rect_lighting_adjoint(*head, *mid, arg("vis_bits"), arg("grad_image"), rows("grad_sh_n"), rows("grad_p"),
                                            arg("grad_weight"), arg("grad_tex"), None)
    return lib.hf_rect_lighting_tangent(*head, *mid, arg("vis_bits"), rows("dsh_n"), rows("dp"), arg("dweight"), arg("dtex"),
                                        arg("dimage"), None)


def _with(i, j, v):
    """LAMP with component j of field i (0: center, 1: ex, 2: ey) replaced by v; i = 3: the radiance"""
    lamp = [list(f) if isinstance(f, tuple) else f for f in LAMP]
    if i == 3:
        lamp[3] = v
    else:
        lamp[i][j] = v
    return tuple(tuple(f) if isinstance(f, list) else f for f in lamp)


BAD_LAMPS = [{"light": None}] + [{"light": _with(i, j, v)} for i in range(3) for j in (0, 2) for v in (NAN, INF)] + \
            [{"light": _with(3, 0, NAN)}, {"light": _with(3, 0, -INF)},
             {"light": (LAMP[0], (0.0, 0.0, 0.0), LAMP[2], 1.0)},                      # |ex x ey| == 0: a zero edge,
             {"light": (LAMP[0], (0.1, 0.2, 0.3), (0.2, 0.4, 0.6), 1.0)}]              # parallel edges
COMMON = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("p", "sh_n", "d", "t")] + [{"null_row": x} for x in ("p", "sh_n", "d")] + BAD_LAMPS
LIGHTING = COMMON + [{"spp": 0}, {"n": 9, "spp": 2}, {"num_rays": 0}, {"num_rays": 33}, {"albedo": NAN}, {"albedo": INF},
                     {"TW": 0}, {"TH": 0}, {"TW": 0, "TH": 0}, {"TW": 1 << 16, "TH": 1 << 15}, {"TW": (1 << 31) - 1, "TH": 2}]
CASES = {
    "hf_rect_rays": COMMON + [{"k": 32}, {"k": 1 << 31}, {"null": ("nrm",)}, {"null_row": "nrm"}, {"null": ("out_o",)},
                              {"null_row": "out_o"}, {"null": ("out_d",)}, {"null_row": "out_d"}, {"null": ("out_maxt",)}],
    "hf_rect_lighting": LIGHTING + [{"null": ("hf",)}, {"null": ("nrm",)}, {"null_row": "nrm"}, {"null": ("image",)}],
    "hf_rect_lighting_adjoint": LIGHTING + [{"null": ("vis_bits",)}, {"null": ("grad_image",)}, {"null_row": "grad_sh_n"},
                                            {"null_row": "grad_p"}],
    "hf_rect_lighting_tangent": LIGHTING + [{"null": ("vis_bits",)}, {"null": ("dimage",)}, {"null_row": "dsh_n"},
                                            {"null_row": "dp"}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "num_rays": "1..32", "k": "below 32", "albedo": "albedo", "light": "",
           "TW": "texels", "TH": "texels", "null": "NULL", "null_row": "NULL"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_lamp_messages_name_the_light():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        for kw in BAD_LAMPS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "light's" in lib.hf_last_error_string().decode(), kw


def test_optional_pointers_and_an_absent_texture_are_not_refused():
    """weight, ray_id, vis_bits of the forward, every gradient and every tangent may be NULL, and without a texture TW and
    TH are not read: the call then fails on the LAST check made on the host (a NULL image or vis_bits), not before"""
    from hf_amd import _capi
    lib = _capi.lib()
    opt = {"hf_rect_lighting": ("vis_bits", "image"),
           "hf_rect_lighting_adjoint": ("grad_sh_n", "grad_p", "grad_weight", "grad_tex", "vis_bits"),
           "hf_rect_lighting_tangent": ("dsh_n", "dp", "dweight", "dtex", "vis_bits")}
    for fn, null in opt.items():
        for tex in ((), ("tex",)):
            kw = dict(TW=0, TH=0) if tex else {}
            assert _call(lib, fn, null=("weight", "ray_id") + null + tex, **kw) == _capi.HF_EINVAL
            msg = lib.hf_last_error_string().decode()
            assert "NULL" in msg and "texels" not in msg and "light's" not in msg, msg
    # n = 0 passes every check of the forward and launches nothing
    assert _call(lib, "hf_rect_lighting", n=0, null=("weight", "ray_id", "vis_bits", "tex")) == _capi.HF_OK


def test_light_geometry_is_the_rectangles():
    """A = 4 |ex x ey| and n_l = normalize(ex x ey) (rectangle.cpp:104-108, 144-146), formed in double; RectLight.geometry
    and from_to_world agree with them"""
    import hf_amd
    from hf_amd import _capi
    lib = _capi.lib()
    area, nl = C.c_float(), (C.c_float * 3)()
    assert lib.hf_rect_light_geometry(C.byref(_lamp(LAMP)), C.byref(area), C.byref(nl)) == _capi.HF_OK
    ex, ey = (np.asarray(v, np.float32).astype(np.float64) for v in LAMP[1:3])
    cr = np.cross(ex, ey)
    assert area.value == np.float32(4 * np.linalg.norm(cr))
    assert np.array_equal(np.asarray(nl[:], np.float32), (cr / np.linalg.norm(cr)).astype(np.float32))
    assert lib.hf_rect_light_geometry(C.byref(_lamp(LAMP)), None, None) == _capi.HF_OK
    for kw in BAD_LAMPS:
        lamp = _lamp(kw["light"])
        assert lib.hf_rect_light_geometry(C.byref(lamp) if lamp is not None else None, C.byref(area), C.byref(nl)) == _capi.HF_EINVAL
    M = np.array([[0.0, 0.3, 9.0, 0.2], [0.2, 0.0, 9.0, -0.1], [0.0, 0.05, 9.0, 1.1]])
    lm = hf_amd.RectLight.from_to_world(M, radiance=1.5)
    assert (lm.center, lm.ex, lm.ey, lm.radiance) == (LAMP[0], LAMP[1], LAMP[2], 1.5)
    a, n = lm.geometry()
    assert a == area.value and tuple(n) == tuple(nl[:])
    with pytest.raises(ValueError):
        hf_amd.RectLight(*LAMP[:3], texture=np.zeros((4, 4)))

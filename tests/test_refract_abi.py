"""The refraction view (hf_bitmap_eval, _adjoint, hf_refract_lighting, _adjoint, _tangent) on the CPU: the five entry points
are declared, exported and bound, HF_VERSION is unchanged, the three Python names are callable, and every bad argument is
refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_bitmap_eval", "hf_bitmap_eval_adjoint", "hf_refract_lighting", "hf_refract_lighting_adjoint",
       "hf_refract_lighting_tangent")
NAN, INF = float("nan"), float("inf")
PLANE = ((-1.0, -1.0, -0.5), (8.0, 0.0, 0.0), (0.0, 4.0, 0.0))


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS, ("Bitmap", "refraction_lighting", "dielectric_lighting"))
    assert "HF_WRAP_CLAMP 0" in hdr and "HF_WRAP_REPEAT 1" in hdr


def _call(lib, fn, n=8, spp=1, eta=1.33, sigma_t=0.5, TW=16, TH=8, wrap=0, receiver=PLANE, null=(), null_row=None):
    from hf_amd import _capi
    rows, arg = stand_ins(null, null_row)
    rcv = None if receiver is None else _capi.hf_receiver_t(*((C.c_float * 3)(*v) for v in receiver))
    tex = (TW, TH, arg("tex"), wrap)
    if fn == "hf_bitmap_eval":
        return lib.hf_bitmap_eval(n, rows("pos", 2), arg("active"), *tex, arg("out"), rows("out_grad", 2), None)
    if fn == "hf_bitmap_eval_adjoint":
        return lib.hf_bitmap_eval_adjoint(n, rows("pos", 2), arg("active"), *tex, arg("grad_out"), rows("grad_pos", 2),
                                          arg("grad_tex"), None)
    mid = (rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), arg("active"), arg("weight"), eta, sigma_t, rcv, *tex)
    if fn == "hf_refract_lighting":
        return lib.hf_refract_lighting(arg("hf"), n, spp, *mid, arg("image"), arg("value"), arg("vis"), rows("pos", 2), None)
    if fn == "hf_refract_lighting_adjoint":
        return lib.hf_refract_lighting_adjoint(n, spp, *mid, arg("vis"), arg("grad_image"), arg("grad_value"), rows("grad_sh_n"),
                                               rows("grad_p"), arg("grad_weight"), arg("grad_tex"), None)
    return lib.hf_refract_lighting_tangent(n, spp, *mid, arg("vis"), rows("dsh_n"), rows("dp"), arg("dweight"), arg("dtex"),
                                           arg("dimage"), arg("dvalue"), None)


TEXTURE = [{"n": 1 << 32}, {"TW": 0}, {"TH": 0}, {"TW": 0, "TH": 0}, {"TW": 1 << 16, "TH": 1 << 15}, {"TW": (1 << 31) - 1, "TH": 2},
           {"wrap": 2}, {"wrap": -1}, {"null": ("tex",)}]
BITMAP = TEXTURE + [{"null": ("pos",)}, {"null_row": "pos"}]
ROW = TEXTURE + [{"null": (x,)} for x in ("p", "nrm", "sh_n", "d", "t")] + [{"null_row": x} for x in ("p", "nrm", "sh_n", "d")] + \
      [{"spp": 0}, {"n": 9, "spp": 2}, {"eta": 0.0}, {"eta": -1.33}, {"eta": NAN}, {"eta": INF}, {"sigma_t": -0.1},
       {"sigma_t": NAN}, {"sigma_t": INF}, {"receiver": None}, {"receiver": ((NAN, 0, 0), (1, 0, 0), (0, 1, 0))},
       {"receiver": ((0, 0, 0), (INF, 0, 0), (0, 1, 0))}, {"receiver": ((0, 0, 0), (1, 0, 0), (2, 0, 0))},
       {"receiver": ((0, 0, 0), (0, 0, 0), (0, 1, 0))}, {"receiver": ((0, 0, 0), (1, 0, 0), (1, 1, 0))}]
CASES = {
    "hf_bitmap_eval": BITMAP + [{"null": ("out",)}, {"null_row": "out_grad"}],
    "hf_bitmap_eval_adjoint": BITMAP + [{"null": ("grad_out",)}, {"null_row": "grad_pos"}, {"null": ("grad_pos", "grad_tex")}],
    "hf_refract_lighting": ROW + [{"null": ("hf",)}, {"null_row": "pos"}, {"null": ("image", "value", "vis", "pos")}],
    "hf_refract_lighting_adjoint": ROW + [{"null": ("vis",)}, {"null_row": "grad_sh_n"}, {"null_row": "grad_p"}],
    "hf_refract_lighting_tangent": ROW + [{"null": ("vis",)}, {"null_row": "dsh_n"}, {"null_row": "dp"},
                                          {"null": ("dimage", "dvalue")}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "TW": "texels", "TH": "texels", "wrap": "wrap must be", "eta": "eta must be",
           "sigma_t": "sigma_t must be", "receiver": "", "null": "NULL", "null_row": "NULL"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_receiver_messages_name_the_receiver():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS[2:]:
        for rcv in (((NAN, 0, 0), (1, 0, 0), (0, 1, 0)), ((0, 0, 0), (1, 0, 0), (2, 0, 0)), ((0, 0, 0), (1, 0, 0), (1, 1, 0))):
            assert _call(lib, fn, receiver=rcv) == _capi.HF_EINVAL
            assert "receiver" in lib.hf_last_error_string().decode()


def test_optional_pointers_are_not_refused_for_being_null():
    """weight, active, the optional outputs, gradients and tangents may be NULL: the call then fails on the LAST check made
    on the host (a NULL vis for the derivatives, an all-NULL output set for the forward), not before"""
    from hf_amd import _capi
    lib = _capi.lib()
    opt = {"hf_refract_lighting_adjoint": ("grad_image", "grad_value", "grad_sh_n", "grad_p", "grad_weight", "grad_tex", "vis"),
           "hf_refract_lighting_tangent": ("dsh_n", "dp", "dweight", "dtex", "dimage", "vis"),
           "hf_refract_lighting": ("image", "value", "vis", "pos")}
    for fn, null in opt.items():
        assert _call(lib, fn, sigma_t=0.0, wrap=1, null=("weight", "active") + null) == _capi.HF_EINVAL
        msg = lib.hf_last_error_string().decode()
        assert "NULL" in msg and "eta" not in msg and "sigma_t" not in msg and "wrap" not in msg, msg
    # n = 0 passes every check and launches nothing (the bitmap entries need no handle)
    assert _call(lib, "hf_bitmap_eval", n=0, null=("active", "out_grad")) == _capi.HF_OK
    assert _call(lib, "hf_bitmap_eval_adjoint", n=0, null=("active", "grad_pos")) == _capi.HF_OK

"""Specular reflection of the environment map (hf_reflect_rays, hf_reflect_lighting, _adjoint, _tangent) on the CPU: the
four entry points are declared, exported and bound, HF_VERSION is unchanged, and every bad argument is refused with
HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_reflect_rays", "hf_reflect_lighting", "hf_reflect_lighting_adjoint", "hf_reflect_lighting_tangent")
NAN, INF = float("nan"), float("inf")
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS, ("reflection_lighting", "reflection_rays"))


def _call(lib, fn, n=8, spp=1, eta=1.5, W=5, H=3, rot=IDENTITY, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    R = None if rot is None else (C.c_float * 9)(*rot)
    if fn == "hf_reflect_rays":
        return lib.hf_reflect_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), arg("active"), rows("out_o"),
                                   rows("out_d"), arg("out_maxt"), None)
    mid = (arg("active"), arg("weight"), eta, W, H, arg("data"), R)
    if fn == "hf_reflect_lighting":
        return lib.hf_reflect_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                       arg("image"), arg("value"), arg("vis"), None)
    head = (n, spp, rows("sh_n"), rows("d"), arg("t"), *mid, arg("vis"))
    if fn == "hf_reflect_lighting_adjoint":
        return lib.hf_reflect_lighting_adjoint(*head, arg("grad_image"), arg("grad_value"), rows("grad_sh_n"), arg("grad_weight"),
                                               arg("grad_data"), None)
    return lib.hf_reflect_lighting_tangent(*head, rows("dsh_n"), arg("dweight"), arg("ddata"), arg("dimage"), arg("dvalue"), None)


ROWS = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("sh_n", "d", "t")] + [{"null_row": x} for x in ("sh_n", "d")]
LIGHT = ROWS + [{"spp": 0}, {"n": 9, "spp": 2}, {"W": 1}, {"H": 1}, {"W": 0, "H": 0}, {"eta": -1.5}, {"eta": -0.0 - 1e-30},
                {"eta": NAN}, {"eta": INF}, {"eta": -INF}, {"rot": (1, 0, 0, 0, NAN, 0, 0, 0, 1)},
                {"rot": (1, 0, 0, 0, 1, 0, 0, 0, INF)}, {"null": ("data",)}]
CASES = {
    "hf_reflect_rays": ROWS + [{"null": (x,)} for x in ("p", "nrm", "out_o", "out_d", "out_maxt")] +
                       [{"null_row": x} for x in ("p", "nrm", "out_o", "out_d")],
    "hf_reflect_lighting": LIGHT + [{"null": (x,)} for x in ("hf", "p", "nrm")] + [{"null_row": x} for x in ("p", "nrm")] +
                           [{"null": ("image", "value", "vis")}],
    "hf_reflect_lighting_adjoint": LIGHT + [{"null": ("vis",)}, {"null_row": "grad_sh_n"}],
    "hf_reflect_lighting_tangent": LIGHT + [{"null": ("vis",)}, {"null_row": "dsh_n"}, {"null": ("dimage", "dvalue")}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "W": "2 x 2", "H": "2 x 2", "eta": "eta must be", "rot": "rot must be finite",
           "null": "NULL", "null_row": "NULL"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_optional_pointers_are_not_refused_for_being_null():
    """weight, active, rot (the identity) and two of the three forward outputs may be NULL: the call then fails on the
    LAST check made on the host (a NULL vis for the derivatives, an all-NULL output set for the forward), not before"""
    from hf_amd import _capi
    lib = _capi.lib()
    for fn, last in (("hf_reflect_lighting_adjoint", ("vis",)), ("hf_reflect_lighting_tangent", ("vis",)),
                     ("hf_reflect_lighting", ("image", "value", "vis"))):
        assert _call(lib, fn, eta=0.0, rot=None, null=("weight", "active") + last) == _capi.HF_EINVAL
        msg = lib.hf_last_error_string().decode()
        assert "NULL" in msg and "eta" not in msg and "rot" not in msg, msg

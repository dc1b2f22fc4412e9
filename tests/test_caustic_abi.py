"""Refractive caustics (hf_caustic_rays, hf_caustic_lighting, _adjoint, _tangent) on the CPU: the four entry points are
declared, exported and bound, HF_VERSION is unchanged, and every bad argument is refused with HF_EINVAL and a message
before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_caustic_rays", "hf_caustic_lighting", "hf_caustic_adjoint", "hf_caustic_tangent")


def test_symbols_declared_exported_and_bound():
    import hf_amd
    hdr = assert_symbols(FNS, ("Receiver", "caustic_lighting", "caustic_rays", "caustic_film"))
    assert "hf_receiver_t" in hdr
    r = hf_amd.Receiver.plane_z(-0.5, (-1.0, 1.0), (-2.0, 2.0), 64, 32)
    assert r.origin == (-1.0, -2.0, -0.5) and r.ex == (32.0, 0.0, 0.0) and r.ey == (0.0, 8.0, 0.0)


def _call(lib, fn, n=8, eta=1.33, power=1.0, rcv=((0, 0, -1), (4, 0, 0), (0, 4, 0)), null=(), null_row=None):
    from hf_amd import _capi
    rows, arg = stand_ins(null, null_row)
    receiver = None if "receiver" in null else _capi.hf_receiver_t(*[(C.c_float * 3)(*v) for v in rcv])
    head = (n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), arg("active"))
    if fn == "hf_caustic_rays":
        return lib.hf_caustic_rays(*head, eta, receiver, rows("out_o"), rows("out_d"), arg("out_maxt"), None)
    if fn == "hf_caustic_lighting":
        return lib.hf_caustic_lighting(arg("hf"), *head, arg("weight"), eta, power, receiver, rows("pos", 2), arg("value"),
                                       arg("vis"), None)
    mid = (arg("weight"), eta, power, receiver, arg("vis"))
    if fn == "hf_caustic_adjoint":
        return lib.hf_caustic_adjoint(*head, *mid, rows("grad_pos", 2), arg("grad_value"), rows("grad_sh_n"), rows("grad_p"),
                                      arg("grad_weight"), None)
    return lib.hf_caustic_tangent(*head, *mid, rows("dsh_n"), rows("dp"), arg("dweight"), rows("dpos", 2), arg("dvalue"), None)


COMMON = [{"n": 1 << 32}, {"eta": 0.0}, {"eta": -1.33}, {"eta": float("nan")}, {"eta": float("inf")},
          {"rcv": ((0, 0, -1), (4, 0, 0), (8, 0, 0))}, {"rcv": ((0, 0, -1), (0, 0, 0), (0, 4, 0))},      # ex x ey = 0
          {"rcv": ((0, 0, -1), (4, 0, 0), (1e-3, 4, 0))}, {"rcv": ((0, 0, -1), (4, 0, 0), (4, 4, 0))},   # not orthogonal
          {"rcv": ((float("nan"), 0, -1), (4, 0, 0), (0, 4, 0))},
          {"null": ("receiver",)}] + \
         [{"null": (x,)} for x in ("p", "nrm", "sh_n", "d", "t")] + [{"null_row": x} for x in ("p", "nrm", "sh_n", "d")]
POWER = [{"power": float("nan")}, {"power": float("inf")}, {"power": float("-inf")}]
CASES = {
    "hf_caustic_rays": COMMON + [{"null": (x,)} for x in ("out_o", "out_d", "out_maxt")] +
                       [{"null_row": x} for x in ("out_o", "out_d")],
    "hf_caustic_lighting": COMMON + POWER + [{"null": (x,)} for x in ("hf", "pos", "value")] + [{"null_row": "pos"}],
    "hf_caustic_adjoint": COMMON + POWER + [{"null": ("vis",)}] +
                          [{"null_row": x} for x in ("grad_pos", "grad_sh_n", "grad_p")],
    "hf_caustic_tangent": COMMON + POWER + [{"null": ("vis",)}] + [{"null_row": x} for x in ("dsh_n", "dp", "dpos")],
}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


def test_orthogonality_bound_is_relative():
    """|<ex, ey>| <= 1e-5 |ex| |ey| passes the receiver check whatever the scale of the film: the call then fails on the
    next check (a NULL output), not on the receiver"""
    from hf_amd import _capi
    lib = _capi.lib()
    for s in (1e-3, 1.0, 1e3):
        rcv = ((0, 0, -1), (4 * s, 0, 0), (4e-6 * s, 4 * s, 0))
        assert _call(lib, "hf_caustic_rays", rcv=rcv, null=("out_maxt",)) == _capi.HF_EINVAL
        assert b"NULL argument" in lib.hf_last_error_string()
        rcv = ((0, 0, -1), (4 * s, 0, 0), (4e-4 * s, 4 * s, 0))
        assert _call(lib, "hf_caustic_rays", rcv=rcv, null=("out_maxt",)) == _capi.HF_EINVAL
        assert b"orthogonal" in lib.hf_last_error_string()

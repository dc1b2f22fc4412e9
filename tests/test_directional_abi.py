"""Directional lighting (hf_directional_rays, hf_directional_lighting, _adjoint, _tangent,
hf_directional_workspace_floats) on the CPU: the entry points are declared, exported and bound, HF_VERSION is unchanged,
the three Python names are callable, the struct of _capi matches the header's, and every bad argument is refused with
HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C
import re

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_directional_rays", "hf_directional_lighting", "hf_directional_lighting_adjoint", "hf_directional_lighting_tangent")
NAN, INF = float("nan"), float("inf")
LIGHT = ((2.0, 1.0, 1.5), 2.0)     # to_light (not unit), irradiance


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_directional_workspace_floats",), ("DirectionalLight", "directional_lighting", "directional_rays"))
    assert "hf_directional_light_t" in hdr and "HF_DIRECTIONAL_PARAMS 4" in hdr


def test_struct_size_and_field_order_match_the_header():
    from hf_amd import _capi
    hdr = assert_symbols((), ())
    m = re.search(r"typedef struct hf_directional_light \{(.*?)\} hf_directional_light_t;", hdr, flags=re.S)
    assert m, "hf_directional_light_t not found in include/hf.h"
    fields = [(t, name, dim) for t, name, dim in re.findall(r"(double|float)\s+(\w+)(?:\[(\d+)\])?\s*;", m.group(1))]
    assert fields == [("double", "to_light", "3"), ("float", "irradiance", "")]
    T = _capi.hf_directional_light_t
    assert [f[0] for f in T._fields_] == ["to_light", "irradiance"]
    assert T._fields_[0][1] is C.c_double * 3 and T._fields_[1][1] is C.c_float
    # three doubles, one float, padded to the alignment of a double: what a C compiler lays out
    assert C.sizeof(T) == 32 and T.to_light.offset == 0 and T.irradiance.offset == 24
    assert _capi.HF_DIRECTIONAL_PARAMS == 4


def test_workspace_holds_four_doubles_per_light_and_block():
    from hf_amd import _capi
    lib = _capi.lib()
    one = lib.hf_directional_workspace_floats(1)
    assert one * 15 == lib.hf_spot_workspace_floats(1) * 4 and one % (2 * 4) == 0 and one > 0
    assert [lib.hf_directional_workspace_floats(k) for k in range(1, 9)] == [k * one for k in range(1, 9)]
    assert lib.hf_directional_workspace_floats(0) == 0 and lib.hf_directional_workspace_floats(9) == 0
    assert lib.hf_directional_workspace_floats(1 << 31) == 0
    assert lib.hf_grid_blocks(1 << 30, 2) * 2 * 4 == one     # family 2: the slab has a row for every block it can get


def _lights(lights):
    from hf_amd import _capi
    if lights is None:
        return None
    L = (_capi.hf_directional_light_t * max(len(lights), 1))()
    for k, s in enumerate(lights):
        L[k] = _capi.hf_directional_light_t((C.c_double * 3)(*s[0]), s[1])
    return L


def _call(lib, fn, n=8, spp=1, albedo=0.8, lights=(LIGHT, LIGHT), n_lights=None, null=(), null_row=None, workspace_offset=0):
    rows, arg = stand_ins(null, null_row)
    L = _lights(lights)
    K = (len(lights) if lights is not None else 1) if n_lights is None else n_lights
    if fn == "hf_directional_rays":
        return lib.hf_directional_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), L, rows("out_o"),
                                       rows("out_d"), arg("out_maxt"), None)
    mid = (arg("weight"), K, L, albedo)
    if fn == "hf_directional_lighting":
        return lib.hf_directional_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                           arg("image"), arg("value"), arg("vis"), None)
    head = (n, spp, rows("sh_n"), rows("d"), arg("t"))
    if fn == "hf_directional_lighting_adjoint":
        return lib.hf_directional_lighting_adjoint(*head, *mid, arg("vis"), arg("grad_image"), arg("grad_value"),
                                                   rows("grad_sh_n"), arg("grad_weight"), arg("grad_lights"),
                                                   arg("workspace", workspace_offset), None)
    return lib.hf_directional_lighting_tangent(*head, *mid, arg("vis"), rows("dsh_n"), arg("dweight"), arg("d_lights"),
                                               arg("dimage"), arg("dvalue"), None)


def _v(j, x):
    v = list(LIGHT[0])
    v[j] = x
    return tuple(v)


# (the bad light stands second in a rig of two: every light is checked)
_bad = lambda s: {"lights": (LIGHT, s)}
BAD_LIGHTS = [{"lights": None}] + [_bad((_v(j, x), 1.0)) for j in range(3) for x in (NAN, INF, -INF)] + \
             [_bad((LIGHT[0], x)) for x in (NAN, INF, -INF)] + \
             [_bad(((0.0, 0.0, 0.0), 1.0)), _bad(((-0.0, 0.0, 0.0), 1.0)), _bad(((1e-200, 0.0, 1e-200), 1.0)),
              _bad(((1e200, 1e200, 0.0), 1.0))]     # |to_light| zero, underflowing to zero, overflowing
SAMPLE = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("sh_n", "d", "t")] + [{"null_row": x} for x in ("sh_n", "d")] + BAD_LIGHTS
POINT = [{"null": ("p",)}, {"null_row": "p"}, {"null": ("nrm",)}, {"null_row": "nrm"}]
LIGHTING = SAMPLE + [{"spp": 0}, {"n": 9, "spp": 2}, {"albedo": NAN}, {"albedo": INF}, {"n_lights": 0}, {"n_lights": 9},
                     {"n_lights": 1 << 31}]
ALL_OUT = ("image", "value", "vis")
CASES = {
    "hf_directional_rays": SAMPLE + POINT + [{"null": ("out_o",)}, {"null_row": "out_o"}, {"null": ("out_d",)},
                                              {"null_row": "out_d"}, {"null": ("out_maxt",)}],
    "hf_directional_lighting": LIGHTING + POINT + [{"null": ("hf",)}, {"null": ALL_OUT}],
    "hf_directional_lighting_adjoint": LIGHTING + [{"null": ("vis",)}, {"null_row": "grad_sh_n"}, {"null": ("workspace",)},
                                                   {"workspace_offset": 4}],
    "hf_directional_lighting_tangent": LIGHTING + [{"null": ("vis",)}, {"null": ("dimage", "dvalue")}, {"null_row": "dsh_n"}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "albedo": "albedo", "lights": "", "n_lights": "lights supported",
           "null": "NULL", "null_row": "NULL", "workspace_offset": "8-byte aligned"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, [kw for kw in CASES[fn] if not (fn == "hf_directional_rays" and "lights" in kw and kw["lights"])],
                   MESSAGE)
    if fn == "hf_directional_rays":    # (one light: the bad one stands alone)
        assert_refused(_call, fn, [{"lights": (kw["lights"][1],)} for kw in BAD_LIGHTS[1:]], MESSAGE)


def test_light_messages_name_the_light():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS[1:]:
        for kw in BAD_LIGHTS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "light 1" in lib.hf_last_error_string().decode(), kw


def test_legal_edges_of_a_light_are_not_refused():
    """any finite length > 0, a light from below, a zero or negative irradiance, a full rig"""
    from hf_amd import _capi
    lib = _capi.lib()
    for s in (((1e-30, 0.0, 0.0), 1.0), ((0.0, 3e30, -4e30), 1.0), ((0.3, 0.1, -0.6), 0.0), ((0.0, 0.0, 1.0), -1.0)):
        assert _call(lib, "hf_directional_lighting_adjoint", n=0, lights=(s,)) == _capi.HF_OK, s
    assert _call(lib, "hf_directional_lighting_tangent", n=0, lights=(LIGHT,) * 8) == _capi.HF_OK


def test_optional_pointers_are_not_refused():
    """weight, each output of the forward but the last, every gradient with the workspace, and every tangent may be NULL:
    the call then fails on the LAST check made on the host, not before.  n = 0 passes every check and launches nothing."""
    from hf_amd import _capi
    lib = _capi.lib()
    for keep in ALL_OUT:
        null = ("weight",) + tuple(x for x in ALL_OUT if x != keep)
        assert _call(lib, "hf_directional_lighting", n=0, null=null) == _capi.HF_OK
    grads = ("grad_image", "grad_value", "grad_sh_n", "grad_weight", "grad_lights", "workspace")
    assert _call(lib, "hf_directional_lighting_adjoint", n=0, null=("weight",) + grads) == _capi.HF_OK
    # (a workspace is asked for only with grad_lights)
    null = tuple(x for x in grads if x != "grad_lights")
    assert _call(lib, "hf_directional_lighting_adjoint", n=0, null=null) == _capi.HF_EINVAL
    assert _call(lib, "hf_directional_lighting_adjoint", n=0, null=tuple(x for x in null if x != "workspace")) == _capi.HF_OK
    tangents = ("dsh_n", "dweight", "d_lights")
    assert _call(lib, "hf_directional_lighting_tangent", n=0, null=("weight", "dvalue") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_directional_lighting_tangent", n=0, null=("weight", "dimage") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_directional_rays", n=0, lights=(LIGHT,)) == _capi.HF_OK


def test_directional_python_class_checks_its_arguments():
    import numpy as np
    import torch
    import hf_amd
    from hf_amd import directional
    s = hf_amd.DirectionalLight((2.0, 1.0, 1.5))
    assert s.irradiance == 1.0 and s.to_light.tolist() == [2.0, 1.0, 1.5] and s.to_light.dtype == torch.float64
    # the reference's `direction` is -to_light
    assert hf_amd.DirectionalLight.from_direction((-2.0, -1.0, -1.5), 2.5).to_light.tolist() == s.to_light.tolist()
    for bad in ((0.0, 0.0, 0.0), (1.0, NAN, 0.0), (INF, 0.0, 0.0), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError):
            hf_amd.DirectionalLight(bad)
    for bad in ((), (s,) * 9, (s, "sun"), torch.zeros((2, 3)), torch.zeros((9, 4)) + 1.0, np.ones(4)):
        with pytest.raises(ValueError):
            directional._rig(bad)
    assert directional._rig(s) == (s,)
    E = torch.tensor(2.5, dtype=torch.float64, requires_grad=True)
    v = torch.tensor([0.3, 0.2, 0.9], dtype=torch.float64, requires_grad=True)
    par = directional._stacked((s, hf_amd.DirectionalLight(v, E)))
    assert par.shape == (2, 4) and par.requires_grad and par.dtype == torch.float64
    L = directional._structs(par)
    assert list(L[0].to_light) == [2.0, 1.0, 1.5] and L[0].irradiance == 1.0
    assert list(L[1].to_light) == [0.3, 0.2, 0.9] and L[1].irradiance == 2.5
    par.sum().backward()
    assert float(E.grad) == 1.0 and v.grad.tolist() == [1.0, 1.0, 1.0]   # the stacked rows hand each light's own tensors their gradients
    # the [K, 4] tensor of direct_lighting: its rows are the lights, and its graph is kept
    rows = torch.tensor([[0.0, 0.0, 1.0, 3.0], [1.0, 0.1, 0.25, 1.5]], requires_grad=True)
    par = directional._stacked(directional._rig(rows))
    assert par.shape == (2, 4) and par.dtype == torch.float64 and par.tolist() == rows.double().tolist()
    par[1, 3].backward()
    assert rows.grad.tolist() == [[0.0] * 4, [0.0, 0.0, 0.0, 1.0]]

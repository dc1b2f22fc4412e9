"""The medium row (hf_medium_rays, hf_medium_lighting, _adjoint, _tangent, hf_medium_workspace_floats) on the CPU: the
entry points are declared, exported and bound, HF_VERSION is unchanged, the four Python names are callable, the struct of
_capi matches the header's, the workspace arithmetic, and every bad argument is refused with HF_EINVAL and a message
before anything touches a device (host addresses stand in for device pointers)."""
import ctypes as C
import re

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_medium_rays", "hf_medium_lighting", "hf_medium_lighting_adjoint", "hf_medium_lighting_tangent")
NAN, INF = float("nan"), float("inf")
LIGHT = ((2.0, 1.0, 1.5), 2.0)     # to_light (not unit), irradiance
MEDIUM = dict(top_origin=(0.0, 0.0, 1.5), top_normal=(0.0, 0.0, 2.0), sigma_t=0.8, albedo=0.75, g=0.3)


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_medium_workspace_floats",), ("Medium", "medium_lighting", "medium_rays", "medium_attenuation"))
    assert "hf_medium_t" in hdr and "HF_MEDIUM_PARAMS 3" in hdr
    # the row takes the directional row's light: no light struct of its own
    assert hdr.count("typedef struct hf_directional_light ") == 1 and "hf_medium_light_t" not in hdr


def test_struct_size_and_field_order_match_the_header():
    from hf_amd import _capi
    hdr = assert_symbols((), ())
    m = re.search(r"typedef struct hf_medium \{(.*?)\} hf_medium_t;", hdr, flags=re.S)
    assert m, "hf_medium_t not found in include/hf.h"
    fields = [(t, names, dim) for t, names, dim in re.findall(r"(double|float)\s+([\w, ]+?)(?:\[(\d+)\])?\s*;", m.group(1))]
    assert fields == [("double", "top_origin", "3"), ("double", "top_normal", "3"), ("float", "sigma_t, albedo, g", "")]
    T = _capi.hf_medium_t
    assert [f[0] for f in T._fields_] == ["top_origin", "top_normal", "sigma_t", "albedo", "g"]
    assert T._fields_[0][1] is C.c_double * 3 and T._fields_[1][1] is C.c_double * 3
    assert all(f[1] is C.c_float for f in T._fields_[2:])
    # six doubles, three floats, padded to the alignment of a double: what a C compiler lays out
    assert C.sizeof(T) == 64 and T.top_origin.offset == 0 and T.top_normal.offset == 24
    assert (T.sigma_t.offset, T.albedo.offset, T.g.offset) == (48, 52, 56)
    assert _capi.HF_MEDIUM_PARAMS == 3


def test_workspace_holds_a_row_of_eleven_doubles_per_block():
    from hf_amd import _capi
    lib = _capi.lib()
    one = lib.hf_medium_workspace_floats(1)
    sums = _capi.HF_MEDIUM_PARAMS + 8      # HF_MEDIUM_PARAMS + HF_MAX_LIGHTS doubles per block, whatever the rig's size
    assert one > 0 and one % (2 * sums) == 0
    assert [lib.hf_medium_workspace_floats(k) for k in range(1, 9)] == [one] * 8
    assert lib.hf_medium_workspace_floats(0) == 0 and lib.hf_medium_workspace_floats(9) == 0
    assert lib.hf_medium_workspace_floats(1 << 31) == 0
    assert lib.hf_grid_blocks(1 << 30, 2) * 2 * sums == one   # family 2: the slab has a row for every block it can get
    assert one * 4 == lib.hf_directional_workspace_floats(1) * sums


def _lights(lights):
    from hf_amd import _capi
    if lights is None:
        return None
    L = (_capi.hf_directional_light_t * max(len(lights), 1))()
    for k, s in enumerate(lights):
        L[k] = _capi.hf_directional_light_t((C.c_double * 3)(*s[0]), s[1])
    return L


def _medium(medium):
    from hf_amd import _capi
    if medium is None:
        return None
    m = dict(MEDIUM, **medium)
    return C.byref(_capi.hf_medium_t((C.c_double * 3)(*m["top_origin"]), (C.c_double * 3)(*m["top_normal"]), m["sigma_t"],
                                     m["albedo"], m["g"]))


def _call(lib, fn, n=8, spp=1, medium={}, lights=(LIGHT, LIGHT), n_lights=None, num_steps=4, k=3, null=(), null_row=None,
          workspace_offset=0):
    rows, arg = stand_ins(null, null_row)
    L, M = _lights(lights), _medium(medium)
    J = (len(lights) if lights is not None else 1) if n_lights is None else n_lights
    if fn == "hf_medium_rays":
        return lib.hf_medium_rays(n, rows("o"), rows("d"), arg("t"), M, L, k, 7, arg("ray_id"), rows("out_o"), rows("out_d"),
                                  arg("out_maxt"), None)
    mid = (arg("weight"), M, J, L, num_steps, 7, arg("ray_id"))
    if fn == "hf_medium_lighting":
        return lib.hf_medium_lighting(arg("hf"), n, spp, rows("o"), rows("d"), arg("t"), *mid, arg("image"), arg("value"),
                                      arg("vis_bits"), None)
    head = (n, spp, rows("o"), rows("d"), arg("t"), *mid, arg("vis_bits"))
    if fn == "hf_medium_lighting_adjoint":
        return lib.hf_medium_lighting_adjoint(*head, arg("grad_image"), arg("grad_value"), arg("grad_weight"), arg("grad_t"),
                                              arg("grad_params"), arg("workspace", workspace_offset), None)
    return lib.hf_medium_lighting_tangent(*head, arg("dweight"), arg("dt"), arg("d_params"), arg("dimage"), arg("dvalue"), None)


def _v(base, j, x):
    v = list(base)
    v[j] = x
    return tuple(v)


# (the bad light stands second in a rig of two: every light is checked)
_bad = lambda s: {"lights": (LIGHT, s)}
BAD_LIGHTS = [{"lights": None}] + [_bad((_v(LIGHT[0], j, x), 1.0)) for j in range(3) for x in (NAN, INF, -INF)] + \
             [_bad((LIGHT[0], x)) for x in (NAN, INF, -INF)] + \
             [_bad(((0.0, 0.0, 0.0), 1.0)), _bad(((1e-200, 0.0, 1e-200), 1.0)), _bad(((1e200, 1e200, 0.0), 1.0))]
BAD_MEDIUM = [{"medium": None}] + [{"medium": {"sigma_t": x}} for x in (0.0, -0.5, NAN, INF)] + \
             [{"medium": {"albedo": x}} for x in (NAN, INF, -INF)] + [{"medium": {"g": x}} for x in (1.0, -1.0, 1.5, NAN, INF)] + \
             [{"medium": {"top_normal": v}} for v in ((0.0, 0.0, 0.0), (1e-200, 0.0, 0.0), (1e200, 1e200, 0.0))] + \
             [{"medium": {key: _v(MEDIUM[key], j, x)}} for key in ("top_normal", "top_origin") for j in range(3) for x in (NAN, INF)]
SAMPLE = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("o", "d", "t")] + [{"null_row": x} for x in ("o", "d")] + BAD_LIGHTS + BAD_MEDIUM
LIGHTING = SAMPLE + [{"spp": 0}, {"n": 9, "spp": 2}, {"n_lights": 0}, {"n_lights": 9}, {"n_lights": 1 << 31}, {"num_steps": 0},
                     {"num_steps": 33}]
ALL_OUT = ("image", "value", "vis_bits")
CASES = {
    "hf_medium_rays": SAMPLE + [{"k": 32}, {"k": 1 << 31}, {"null": ("out_o",)}, {"null_row": "out_o"}, {"null": ("out_d",)},
                                {"null_row": "out_d"}, {"null": ("out_maxt",)}],
    "hf_medium_lighting": LIGHTING + [{"null": ("hf",)}, {"null": ALL_OUT}],
    "hf_medium_lighting_adjoint": LIGHTING + [{"null": ("vis_bits",)}, {"null": ("workspace",)}, {"workspace_offset": 4}],
    "hf_medium_lighting_tangent": LIGHTING + [{"null": ("vis_bits",)}, {"null": ("dimage", "dvalue")}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "lights": "", "medium": "", "n_lights": "lights supported", "num_steps": "1..32",
           "k": "below 32", "null": "NULL", "null_row": "NULL", "workspace_offset": "8-byte aligned"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, [kw for kw in CASES[fn] if not (fn == "hf_medium_rays" and "lights" in kw and kw["lights"])], MESSAGE)
    if fn == "hf_medium_rays":    # (one light: the bad one stands alone)
        assert_refused(_call, fn, [{"lights": (kw["lights"][1],)} for kw in BAD_LIGHTS[1:]], MESSAGE)


def test_medium_messages_name_the_field():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        for kw in BAD_MEDIUM[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert next(iter(kw["medium"])) in lib.hf_last_error_string().decode(), kw
    for fn in FNS[1:]:
        for kw in BAD_LIGHTS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "light 1" in lib.hf_last_error_string().decode(), kw


def test_legal_edges_are_not_refused():
    """any finite top_normal of length > 0, a light from below (it contributes zeros), a zero or negative albedo and
    irradiance, g close to +-1, a full rig, 1 and 32 points"""
    from hf_amd import _capi
    lib = _capi.lib()
    for s in (((1e-30, 0.0, 0.0), 1.0), ((0.3, 0.1, -0.6), 0.0), ((0.0, 0.0, 1.0), -1.0)):
        assert _call(lib, "hf_medium_lighting_adjoint", n=0, lights=(s,)) == _capi.HF_OK, s
    for m in ({"top_normal": (1e-30, 0.0, 0.0)}, {"top_normal": (0.0, 3e30, -4e30)}, {"albedo": 0.0}, {"albedo": -1.0}, {"g": 0.999},
              {"g": -0.999}, {"sigma_t": 1e-30}, {"top_origin": (1e30, -1e30, 0.0)}):
        assert _call(lib, "hf_medium_lighting_tangent", n=0, medium=m) == _capi.HF_OK, m
    assert _call(lib, "hf_medium_lighting_tangent", n=0, lights=(LIGHT,) * 8, num_steps=32) == _capi.HF_OK
    assert _call(lib, "hf_medium_lighting_tangent", n=0, num_steps=1) == _capi.HF_OK
    assert _call(lib, "hf_medium_rays", n=0, lights=(LIGHT,), k=31) == _capi.HF_OK


def test_optional_pointers_are_not_refused():
    """weight, ray_id, each output of the forward but the last, every gradient with the workspace, and every tangent may
    be NULL: the call then fails on the LAST check made on the host, not before.  n = 0 passes every check and launches
    nothing."""
    from hf_amd import _capi
    lib = _capi.lib()
    for keep in ALL_OUT:
        null = ("weight", "ray_id") + tuple(x for x in ALL_OUT if x != keep)
        assert _call(lib, "hf_medium_lighting", n=0, null=null) == _capi.HF_OK
    grads = ("grad_image", "grad_value", "grad_weight", "grad_t", "grad_params", "workspace")
    assert _call(lib, "hf_medium_lighting_adjoint", n=0, null=("weight", "ray_id") + grads) == _capi.HF_OK
    # (a workspace is asked for only with grad_params)
    null = tuple(x for x in grads if x != "grad_params")
    assert _call(lib, "hf_medium_lighting_adjoint", n=0, null=null) == _capi.HF_EINVAL
    assert _call(lib, "hf_medium_lighting_adjoint", n=0, null=tuple(x for x in null if x != "workspace")) == _capi.HF_OK
    tangents = ("dweight", "dt", "d_params")
    assert _call(lib, "hf_medium_lighting_tangent", n=0, null=("weight", "ray_id", "dvalue") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_medium_lighting_tangent", n=0, null=("weight", "ray_id", "dimage") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_medium_rays", n=0, lights=(LIGHT,), null=("ray_id",)) == _capi.HF_OK


def test_medium_python_class_checks_its_arguments():
    import torch
    import hf_amd
    from hf_amd import medium
    m = hf_amd.Medium(0.8)
    assert (m.albedo, m.g) == (0.75, 0.0) and m.top_normal.tolist() == [0.0, 0.0, 1.0] and m.unit_normal.tolist() == [0.0, 0.0, 1.0]
    for bad in (dict(sigma_t=0.0), dict(sigma_t=-1.0), dict(sigma_t=NAN), dict(sigma_t=1.0, g=1.0), dict(sigma_t=1.0, g=NAN),
                dict(sigma_t=1.0, top_normal=(0.0, 0.0, 0.0)), dict(sigma_t=1.0, top_normal=(0.0, 1.0)),
                dict(sigma_t=1.0, top_origin=(0.0, NAN, 0.0))):
        with pytest.raises(ValueError):
            hf_amd.Medium(**bad)
    s = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
    E = torch.tensor(2.5, dtype=torch.float64, requires_grad=True)
    m = hf_amd.Medium(s, 0.6, torch.tensor(0.25), top_origin=(0.0, 0.0, 1.5), top_normal=(0.0, 0.0, 3.0))
    lights = (hf_amd.DirectionalLight((2.0, 1.0, 1.5), E), hf_amd.DirectionalLight((0.0, 0.0, 1.0)))
    par = medium._stacked(m, lights)
    assert par.shape == (5,) and par.requires_grad and par.dtype == torch.float64 and par.tolist() == [0.5, 0.6, 0.25, 2.5, 1.0]
    M, L = medium._structs(par, *medium._geometry(m, lights))
    assert list(M.top_origin) == [0.0, 0.0, 1.5] and list(M.top_normal) == [0.0, 0.0, 3.0]
    assert (M.sigma_t, M.g, L[0].irradiance, L[1].irradiance) == (0.5, 0.25, 2.5, 1.0) and list(L[0].to_light) == [2.0, 1.0, 1.5]
    (par * torch.arange(1.0, 6.0, dtype=torch.float64)).sum().backward()
    assert float(s.grad) == 1.0 and float(E.grad) == 4.0     # the stacked row hands each tensor its own gradient

"""Spot lighting (hf_spot_rays, hf_spot_lighting, _adjoint, _tangent, hf_spot_workspace_floats) on the CPU: the entry
points are declared, exported and bound, HF_VERSION is unchanged, the three Python names are callable, and every bad
argument is refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device
pointers)."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_spot_rays", "hf_spot_lighting", "hf_spot_lighting_adjoint", "hf_spot_lighting_tangent")
NAN, INF = float("nan"), float("inf")
# a rotation about x by 0.3 and a translation: scale-free
_C, _S = float(np.cos(0.3)), float(np.sin(0.3))
TO_WORLD = (1.0, 0.0, 0.0, 0.3, 0.0, _C, -_S, -0.2, 0.0, _S, _C, 2.0)
LIGHT = (TO_WORLD, 2.0, 30.0, 20.0)     # to_world, intensity, cutoff_angle, beam_width


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_spot_workspace_floats",), ("SpotLight", "spot_lighting", "spot_rays"))
    assert "hf_spot_light_t" in hdr and "HF_SPOT_PARAMS 15" in hdr


def test_workspace_holds_fifteen_doubles_per_light_and_block():
    from hf_amd import _capi
    lib = _capi.lib()
    one = lib.hf_spot_workspace_floats(1)
    assert one * 14 == lib.hf_projector_workspace_floats() * 15 and one % (2 * 15) == 0
    assert [lib.hf_spot_workspace_floats(k) for k in range(1, 9)] == [k * one for k in range(1, 9)]
    assert lib.hf_spot_workspace_floats(0) == 0 and lib.hf_spot_workspace_floats(9) == 0


def _lights(lights):
    from hf_amd import _capi
    if lights is None:
        return None
    L = (_capi.hf_spot_light_t * max(len(lights), 1))()
    for k, s in enumerate(lights):
        L[k] = _capi.hf_spot_light_t((C.c_double * 12)(*s[0]), s[1], s[2], s[3])
    return L


def _call(lib, fn, n=8, spp=1, albedo=0.8, lights=(LIGHT, LIGHT), n_lights=None, null=(), null_row=None, workspace_offset=0):
    rows, arg = stand_ins(null, null_row)
    L = _lights(lights)
    K = (len(lights) if lights is not None else 1) if n_lights is None else n_lights
    if fn == "hf_spot_rays":
        return lib.hf_spot_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), L, rows("out_o"), rows("out_d"),
                                arg("out_maxt"), None)
    mid = (arg("weight"), K, L, albedo)
    if fn == "hf_spot_lighting":
        return lib.hf_spot_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid, arg("image"),
                                    arg("value"), arg("vis"), None)
    head = (n, spp, rows("p"), rows("sh_n"), rows("d"), arg("t"))
    if fn == "hf_spot_lighting_adjoint":
        return lib.hf_spot_lighting_adjoint(*head, *mid, arg("vis"), arg("grad_image"), arg("grad_value"), rows("grad_sh_n"),
                                            rows("grad_p"), arg("grad_weight"), arg("grad_lights"), arg("workspace", workspace_offset), None)
    return lib.hf_spot_lighting_tangent(*head, *mid, arg("vis"), rows("dsh_n"), rows("dp"), arg("dweight"), arg("d_lights"),
                                        arg("dimage"), arg("dvalue"), None)


def _tw(j, v):
    m = list(TO_WORLD)
    m[j] = v
    return tuple(m)


SCALED = tuple(1.01 * v if j % 4 != 3 else v for j, v in enumerate(TO_WORLD))   # |A^T A - I| = 2e-2
SHEARED = _tw(1, 0.05)
# (the bad light stands second in a rig of two: every light is checked)
_bad = lambda s: {"lights": (LIGHT, s)}
BAD_LIGHTS = [{"lights": None}] + [_bad((_tw(j, v), 1.0, 30.0, 20.0)) for j in (0, 3, 11) for v in (NAN, INF)] + \
             [_bad((TO_WORLD, v, 30.0, 20.0)) for v in (NAN, INF, -INF)] + \
             [_bad((TO_WORLD, 1.0, c, b)) for c, b in ((NAN, 20.0), (30.0, NAN), (INF, 20.0), (30.0, 0.0), (30.0, -5.0), (20.0, 30.0),
                                                       (181.0, 20.0), (270.0, 180.0), (0.0, 0.0))] + \
             [_bad((SCALED, 1.0, 30.0, 20.0)), _bad((SHEARED, 1.0, 30.0, 20.0))]
COMMON = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("p", "sh_n", "d", "t")] + [{"null_row": x} for x in ("p", "sh_n", "d")] + BAD_LIGHTS
LIGHTING = COMMON + [{"spp": 0}, {"n": 9, "spp": 2}, {"albedo": NAN}, {"albedo": INF}, {"n_lights": 0}, {"n_lights": 9},
                     {"n_lights": 1 << 31}]
ALL_OUT = ("image", "value", "vis")
CASES = {
    "hf_spot_rays": COMMON + [{"null": ("nrm",)}, {"null_row": "nrm"}, {"null": ("out_o",)}, {"null_row": "out_o"},
                              {"null": ("out_d",)}, {"null_row": "out_d"}, {"null": ("out_maxt",)}],
    "hf_spot_lighting": LIGHTING + [{"null": ("hf",)}, {"null": ("nrm",)}, {"null_row": "nrm"}, {"null": ALL_OUT}],
    "hf_spot_lighting_adjoint": LIGHTING + [{"null": ("vis",)}, {"null_row": "grad_sh_n"}, {"null_row": "grad_p"},
                                            {"null": ("workspace",)}, {"workspace_offset": 4}],
    "hf_spot_lighting_tangent": LIGHTING + [{"null": ("vis",)}, {"null": ("dimage", "dvalue")}, {"null_row": "dsh_n"},
                                            {"null_row": "dp"}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "albedo": "albedo", "lights": "", "n_lights": "lights supported",
           "null": "NULL", "null_row": "NULL", "workspace_offset": "8-byte aligned"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, [kw for kw in CASES[fn] if not (fn == "hf_spot_rays" and "lights" in kw and kw["lights"])], MESSAGE)
    if fn == "hf_spot_rays":    # (one light: the bad one stands alone)
        assert_refused(_call, fn, [{"lights": (kw["lights"][1],)} for kw in BAD_LIGHTS[1:]], MESSAGE)


def test_light_messages_name_the_light():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS[1:]:
        for kw in BAD_LIGHTS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "light 1" in lib.hf_last_error_string().decode(), kw


def test_legal_edges_of_the_angles_are_not_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    for c, b in ((180.0, 180.0), (30.0, 30.0), (180.0, 1e-3), (1e-3, 1e-3)):
        assert _call(lib, "hf_spot_lighting_adjoint", n=0, lights=((TO_WORLD, 1.0, c, b),)) == _capi.HF_OK, (c, b)
    assert _call(lib, "hf_spot_lighting_tangent", n=0, lights=(LIGHT,) * 8) == _capi.HF_OK


def test_optional_pointers_are_not_refused():
    """weight, each output of the forward but the last, every gradient with the workspace, and every tangent may be NULL:
    the call then fails on the LAST check made on the host, not before.  n = 0 passes every check and launches nothing."""
    from hf_amd import _capi
    lib = _capi.lib()
    for keep in ALL_OUT:
        null = ("weight",) + tuple(x for x in ALL_OUT if x != keep)
        assert _call(lib, "hf_spot_lighting", n=0, null=null) == _capi.HF_OK
    grads = ("grad_image", "grad_value", "grad_sh_n", "grad_p", "grad_weight", "grad_lights", "workspace")
    assert _call(lib, "hf_spot_lighting_adjoint", n=0, null=("weight",) + grads) == _capi.HF_OK
    # (a workspace is asked for only with grad_lights)
    null = tuple(x for x in grads if x != "grad_lights")
    assert _call(lib, "hf_spot_lighting_adjoint", n=0, null=null) == _capi.HF_EINVAL
    assert _call(lib, "hf_spot_lighting_adjoint", n=0, null=tuple(x for x in null if x != "workspace")) == _capi.HF_OK
    tangents = ("dsh_n", "dp", "dweight", "d_lights")
    assert _call(lib, "hf_spot_lighting_tangent", n=0, null=("weight", "dvalue") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_spot_lighting_tangent", n=0, null=("weight", "dimage") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_spot_rays", n=0, lights=(LIGHT,)) == _capi.HF_OK


def test_spot_python_class_checks_its_arguments():
    import torch
    import hf_amd
    from hf_amd import spot
    s = hf_amd.SpotLight.look_at((0.3, -0.2, 2.0), (0, 0, 0.25), (0, 1, 0))
    assert s.cutoff_angle == 20.0 and s.beam_width == 15.0 and s.intensity == 1.0 and s.to_world.shape == (4, 4)   # the reference's defaults
    assert hf_amd.SpotLight(s.to_world, 2.0, 180.0, 180.0).beam_width == 180.0
    for c, b in ((20.0, 30.0), (181.0, 20.0), (20.0, 0.0), (0.0, None), (float("nan"), 10.0)):
        with pytest.raises(ValueError):
            hf_amd.SpotLight(s.to_world, 1.0, c, b)
    for bad in ((), (s,) * 9, (s, "lamp")):
        with pytest.raises(ValueError):
            spot._rig(bad)
    assert spot._rig(s) == (s,)
    cut = torch.tensor(30.0, dtype=torch.float64, requires_grad=True)
    tw, par = spot._stacked((s, hf_amd.SpotLight(s.to_world[:3], torch.tensor(2.5), cut, 12.0)))
    assert tw.shape == (2, 12) and par.shape == (2, 3) and par.requires_grad and tw.dtype == par.dtype == torch.float64
    L = spot._structs(tw, par)
    assert (L[1].intensity, L[1].cutoff_angle, L[1].beam_width) == (2.5, 30.0, 12.0)
    assert list(L[0].to_world) == s.to_world.reshape(-1)[:12].tolist()
    par.sum().backward()
    assert float(cut.grad) == 1.0       # the stacked rows hand each light's own tensors their gradients

"""Specular highlights (hf_specular_lighting, _adjoint, _tangent, hf_specular_workspace_floats) on the CPU: the entry
points are declared, exported and bound, HF_VERSION is unchanged, the Python name is callable, and every bad argument is
refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers); the
Python function raises ValueError for each of its own."""
import ctypes as C
import types

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_specular_lighting", "hf_specular_lighting_adjoint", "hf_specular_lighting_tangent")
NAN, INF = float("nan"), float("inf")
LIGHT = ((2.0, 1.0, 1.5), 2.0)     # to_light (not unit), irradiance


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_specular_workspace_floats",), ("specular_lighting",))
    # the row takes the directional row's light: no struct of its own
    assert "hf_specular_light_t" not in hdr and "struct hf_specular" not in hdr and hdr.count("typedef struct hf_directional_light ") == 1


def test_workspace_holds_four_doubles_per_light_and_block():
    from hf_amd import _capi
    lib = _capi.lib()
    one = lib.hf_specular_workspace_floats(1)
    assert one == lib.hf_directional_workspace_floats(1) and one % (2 * 4) == 0 and one > 0
    assert [lib.hf_specular_workspace_floats(k) for k in range(1, 9)] == [k * one for k in range(1, 9)]
    assert lib.hf_specular_workspace_floats(0) == 0 and lib.hf_specular_workspace_floats(9) == 0
    assert lib.hf_specular_workspace_floats(1 << 31) == 0
    assert lib.hf_grid_blocks(1 << 30, 2) * 2 * 4 == one     # family 2: the slab has a row for every block it can get


def _lights(lights):
    from hf_amd import _capi
    if lights is None:
        return None
    L = (_capi.hf_directional_light_t * max(len(lights), 1))()
    for k, s in enumerate(lights):
        L[k] = _capi.hf_directional_light_t((C.c_double * 3)(*s[0]), s[1])
    return L


def _call(lib, fn, n=8, spp=1, eta=1.5, lights=(LIGHT, LIGHT), n_lights=None, null=(), null_row=None, workspace_offset=0):
    rows, arg = stand_ins(null, null_row)
    L = _lights(lights)
    K = (len(lights) if lights is not None else 1) if n_lights is None else n_lights
    head = (n, spp, rows("sh_n"), rows("d"), arg("weight"), arg("alpha"), eta, K, L, arg("vis"))
    if fn == "hf_specular_lighting":
        return lib.hf_specular_lighting(*head, arg("image"), arg("value"), None)
    if fn == "hf_specular_lighting_adjoint":
        return lib.hf_specular_lighting_adjoint(*head, arg("grad_image"), arg("grad_value"), rows("grad_sh_n"),
                                                arg("grad_weight"), arg("grad_alpha"), arg("grad_lights"),
                                                arg("workspace", workspace_offset), None)
    return lib.hf_specular_lighting_tangent(*head, rows("dsh_n"), arg("dweight"), arg("dalpha"), arg("d_lights"),
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
LIGHTING = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("sh_n", "d", "alpha", "vis")] + [{"null_row": x} for x in ("sh_n", "d")] + \
           BAD_LIGHTS + [{"spp": 0}, {"n": 9, "spp": 2}, {"n_lights": 0}, {"n_lights": 9}, {"n_lights": 1 << 31}] + \
           [{"eta": x} for x in (-1.0, -1e-30, NAN, INF, -INF)]
CASES = {
    "hf_specular_lighting": LIGHTING + [{"null": ("image", "value")}],
    "hf_specular_lighting_adjoint": LIGHTING + [{"null_row": "grad_sh_n"}, {"null": ("workspace",)}, {"workspace_offset": 4}],
    "hf_specular_lighting_tangent": LIGHTING + [{"null": ("dimage", "dvalue")}, {"null_row": "dsh_n"}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "eta": "eta", "lights": "", "n_lights": "lights supported",
           "null": "NULL", "null_row": "NULL", "workspace_offset": "8-byte aligned"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_light_messages_name_the_light():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        for kw in BAD_LIGHTS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "light 1" in lib.hf_last_error_string().decode(), kw


def test_legal_edges_are_not_refused():
    """any finite length > 0, a light from below, a zero or negative irradiance, a full rig, the mirror and a matched index"""
    from hf_amd import _capi
    lib = _capi.lib()
    for s in (((1e-30, 0.0, 0.0), 1.0), ((0.0, 3e30, -4e30), 1.0), ((0.3, 0.1, -0.6), 0.0), ((0.0, 0.0, 1.0), -1.0)):
        assert _call(lib, "hf_specular_lighting_adjoint", n=0, lights=(s,)) == _capi.HF_OK, s
    assert _call(lib, "hf_specular_lighting_tangent", n=0, lights=(LIGHT,) * 8) == _capi.HF_OK
    for eta in (0.0, 1.0, 1e-3, 40.0):
        assert _call(lib, "hf_specular_lighting", n=0, eta=eta) == _capi.HF_OK, eta


def test_optional_pointers_are_not_refused():
    """weight, either output of the forward, every gradient with the workspace, and every tangent may be NULL.  n = 0
    passes every check and launches nothing."""
    from hf_amd import _capi
    lib = _capi.lib()
    for drop in ("image", "value"):
        assert _call(lib, "hf_specular_lighting", n=0, null=("weight", drop)) == _capi.HF_OK
    grads = ("grad_image", "grad_value", "grad_sh_n", "grad_weight", "grad_alpha", "grad_lights", "workspace")
    assert _call(lib, "hf_specular_lighting_adjoint", n=0, null=("weight",) + grads) == _capi.HF_OK
    # (a workspace is asked for only with grad_lights)
    null = tuple(x for x in grads if x != "grad_lights")
    assert _call(lib, "hf_specular_lighting_adjoint", n=0, null=null) == _capi.HF_EINVAL
    assert _call(lib, "hf_specular_lighting_adjoint", n=0, null=tuple(x for x in null if x != "workspace")) == _capi.HF_OK
    tangents = ("dsh_n", "dweight", "dalpha", "d_lights")
    assert _call(lib, "hf_specular_lighting_tangent", n=0, null=("weight", "dvalue") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_specular_lighting_tangent", n=0, null=("weight", "dimage") + tangents) == _capi.HF_OK


def test_python_function_checks_its_arguments():
    """every bad argument of hf_amd.specular_lighting is a ValueError, raised before the library is called (host tensors
    stand in for the wavefront: nothing gets as far as a launch)"""
    import torch
    import hf_amd
    n = 6
    si = types.SimpleNamespace(sh_frame=types.SimpleNamespace(n=torch.zeros((3, n))))
    ray = types.SimpleNamespace(d=torch.zeros((3, n)))
    sun = hf_amd.DirectionalLight((0.0, 0.0, 1.0), 2.0)
    vis = torch.zeros(n, dtype=torch.uint8)
    good = dict(si=si, ray=ray, lights=sun, vis=vis, alpha=0.3)
    bad = [dict(vis=torch.zeros(n)), dict(vis=torch.zeros(n + 1, dtype=torch.uint8)), dict(vis=vis.reshape(2, 3)),
           dict(vis=vis.numpy()), dict(eta=-1.0), dict(eta=NAN), dict(eta=INF), dict(spp=0), dict(spp=4),
           dict(alpha=torch.zeros(n - 1)), dict(alpha=torch.zeros((2, n))), dict(weight=torch.zeros(n + 2)),
           dict(lights=()), dict(lights=(sun,) * 9), dict(lights=torch.zeros((2, 3))), dict(lights=(sun, "lamp")),
           dict(ray=types.SimpleNamespace(d=torch.zeros((3, n + 1))))]
    for kw in bad:
        with pytest.raises(ValueError):
            hf_amd.specular_lighting(**{**good, **kw})

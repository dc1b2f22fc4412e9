"""Projector lighting (hf_projector_rays, hf_projector_lighting, _adjoint, _tangent, hf_projector_workspace_floats) on the
CPU: the entry points are declared, exported and bound, HF_VERSION is unchanged, the three Python names are callable, and
every bad argument is refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for
device pointers)."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_projector_rays", "hf_projector_lighting", "hf_projector_lighting_adjoint", "hf_projector_lighting_tangent")
NAN, INF = float("nan"), float("inf")
# a rotation about x by 0.3 and a translation: scale-free
_C, _S = float(np.cos(0.3)), float(np.sin(0.3))
TO_WORLD = (1.0, 0.0, 0.0, 0.3, 0.0, _C, -_S, -0.2, 0.0, _S, _C, 2.0)
PROJ = (TO_WORLD, 40.0, 1.5)


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS + ("hf_projector_workspace_floats",), ("Projector", "projector_lighting", "projector_rays"))
    assert "hf_projector_t" in hdr


def test_workspace_holds_fourteen_doubles_per_block():
    from hf_amd import _capi
    lib = _capi.lib()
    assert lib.hf_projector_workspace_floats() * 13 == lib.hf_sensor_workspace_floats() * 14
    assert lib.hf_projector_workspace_floats() % (2 * 14) == 0


def _proj(pr):
    from hf_amd import _capi
    return None if pr is None else _capi.hf_projector_t((C.c_double * 12)(*pr[0]), pr[1], pr[2])


def _call(lib, fn, n=8, spp=1, albedo=0.8, projector=PROJ, TW=16, TH=8, wrap=1, null=(), null_row=None, workspace_offset=0):
    rows, arg = stand_ins(null, null_row)
    pr = _proj(projector)
    if fn == "hf_projector_rays":
        return lib.hf_projector_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), pr, TW, TH, rows("out_o"),
                                     rows("out_d"), arg("out_maxt"), None)
    mid = (arg("weight"), pr, TW, TH, arg("tex"), wrap, albedo)
    if fn == "hf_projector_lighting":
        return lib.hf_projector_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                         arg("image"), arg("value"), arg("vis"), rows("uv", 2), None)
    head = (n, spp, rows("p"), rows("sh_n"), rows("d"), arg("t"))
    if fn == "hf_projector_lighting_adjoint":
        return lib.hf_projector_lighting_adjoint(*head, *mid, arg("vis"), arg("grad_image"), arg("grad_value"), rows("grad_sh_n"),
                                                 rows("grad_p"), arg("grad_weight"), arg("grad_tex"), arg("grad_to_world"),
                                                 arg("grad_fov"), arg("grad_scale"), arg("workspace", workspace_offset), None)
    return lib.hf_projector_lighting_tangent(*head, *mid, arg("vis"), rows("dsh_n"), rows("dp"), arg("dweight"), arg("dtex"),
                                             arg("d_to_world"), arg("d_fov"), arg("d_scale"), arg("dimage"), arg("dvalue"), None)


def _tw(j, v):
    m = list(TO_WORLD)
    m[j] = v
    return tuple(m)


SCALED = tuple(1.01 * v if j % 4 != 3 else v for j, v in enumerate(TO_WORLD))   # |A^T A - I| = 2e-2
SHEARED = _tw(1, 0.05)
BAD_PROJECTORS = [{"projector": None}] + [{"projector": (_tw(j, v), 40.0, 1.0)} for j in (0, 3, 11) for v in (NAN, INF)] + \
                 [{"projector": (TO_WORLD, f, 1.0)} for f in (NAN, INF, 0.0, -10.0, 180.0, 270.0)] + \
                 [{"projector": (TO_WORLD, 40.0, s)} for s in (NAN, INF, -INF)] + \
                 [{"projector": (SCALED, 40.0, 1.0)}, {"projector": (SHEARED, 40.0, 1.0)}]
COMMON = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("p", "sh_n", "d", "t")] + [{"null_row": x} for x in ("p", "sh_n", "d")] + \
         BAD_PROJECTORS + [{"TW": 0}, {"TH": 0}, {"TW": 0, "TH": 0}, {"TW": 1 << 16, "TH": 1 << 15}, {"TW": (1 << 31) - 1, "TH": 2}]
LIGHTING = COMMON + [{"spp": 0}, {"n": 9, "spp": 2}, {"albedo": NAN}, {"albedo": INF}, {"wrap": 2}, {"wrap": -1}]
ALL_OUT = ("image", "value", "vis", "uv")
CASES = {
    "hf_projector_rays": COMMON + [{"null": ("nrm",)}, {"null_row": "nrm"}, {"null": ("out_o",)}, {"null_row": "out_o"},
                                   {"null": ("out_d",)}, {"null_row": "out_d"}, {"null": ("out_maxt",)}],
    "hf_projector_lighting": LIGHTING + [{"null": ("hf",)}, {"null": ("nrm",)}, {"null_row": "nrm"}, {"null_row": "uv"},
                                         {"null": ALL_OUT}],
    "hf_projector_lighting_adjoint": LIGHTING + [{"null": ("vis",)}, {"null_row": "grad_sh_n"}, {"null_row": "grad_p"},
                                                 {"null": ("workspace",)}, {"workspace_offset": 4}],
    "hf_projector_lighting_tangent": LIGHTING + [{"null": ("vis",)}, {"null": ("dimage", "dvalue")}, {"null_row": "dsh_n"},
                                                 {"null_row": "dp"}],
}
MESSAGE = {"n": "2^32", "spp": "multiple of spp", "albedo": "albedo", "projector": "", "TW": "texels", "TH": "texels",
           "wrap": "wrap", "null": "NULL", "null_row": "NULL", "workspace_offset": "8-byte aligned"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_projector_messages_name_the_projector():
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        for kw in BAD_PROJECTORS[1:]:
            assert _call(lib, fn, **kw) == _capi.HF_EINVAL
            assert "projector's" in lib.hf_last_error_string().decode(), kw


def test_optional_pointers_are_not_refused():
    """weight, the texture, each output of the forward but the last, every gradient with the workspace, and every tangent
    may be NULL: the call then fails on the LAST check made on the host, not before.  n = 0 passes every check and launches
    nothing."""
    from hf_amd import _capi
    lib = _capi.lib()
    for keep in ALL_OUT:   # one output is enough: the next check needs a device (here: a handle that is none)
        null = ("weight", "tex") + tuple(x for x in ALL_OUT if x != keep)
        assert _call(lib, "hf_projector_lighting", n=0, null=null) == _capi.HF_OK
    grads = ("grad_image", "grad_value", "grad_sh_n", "grad_p", "grad_weight", "grad_tex", "grad_to_world", "grad_fov", "grad_scale",
             "workspace")
    assert _call(lib, "hf_projector_lighting_adjoint", n=0, null=("weight", "tex") + grads) == _capi.HF_OK
    # (a workspace is asked for only with a reduced gradient)
    for g in ("grad_to_world", "grad_fov", "grad_scale"):
        null = tuple(x for x in grads if x != g)
        assert _call(lib, "hf_projector_lighting_adjoint", n=0, null=null) == _capi.HF_EINVAL
        assert _call(lib, "hf_projector_lighting_adjoint", n=0, null=tuple(x for x in null if x != "workspace")) == _capi.HF_OK
    tangents = ("dsh_n", "dp", "dweight", "dtex", "d_to_world", "d_fov", "d_scale")
    assert _call(lib, "hf_projector_lighting_tangent", n=0, null=("weight", "tex", "dvalue") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_projector_lighting_tangent", n=0, null=("weight", "tex", "dimage") + tangents) == _capi.HF_OK
    assert _call(lib, "hf_projector_rays", n=0) == _capi.HF_OK


def test_projector_python_class_checks_its_arguments():
    import torch
    import hf_amd
    pr = hf_amd.Projector.look_at((0.3, -0.2, 2.0), (0, 0, 0.25), (0, 1, 0), 40.0)
    assert pr.resolution == (1, 1) and pr.irradiance is None and pr.wrap == "repeat" and pr.to_world.shape == (4, 4)
    tex = torch.zeros((8, 16), dtype=torch.float32)
    assert hf_amd.Projector(pr.to_world, 40.0, tex).resolution == (16, 8)
    assert hf_amd.Projector(pr.to_world, 40.0, hf_amd.Bitmap(tex, wrap="clamp")).wrap == "clamp"
    assert hf_amd.Projector(pr.to_world, 40.0, resolution=(16, 8)).resolution == (16, 8)
    with pytest.raises(ValueError):
        hf_amd.Projector(pr.to_world, 40.0, tex, wrap="mirror")
    with pytest.raises(ValueError):
        hf_amd.Projector(pr.to_world, 40.0, np.zeros((4, 4)))
    s = pr._struct(pr.to_world, torch.tensor(40.0, dtype=torch.float64), 1.5)
    assert s.x_fov == 40.0 and s.scale == 1.5 and list(s.to_world) == pr.to_world.reshape(-1)[:12].tolist()

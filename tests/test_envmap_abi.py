"""Environment-map lighting (hf_envmap_*) on the CPU: the entry points are declared, exported and bound; every bad
argument is refused with HF_EINVAL before anything touches a device (host addresses stand in for device pointers, so a
call that got as far as a launch would not return HF_EINVAL); HF_VERSION is unchanged."""
import ctypes as C

import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_envmap_table_floats", "hf_envmap_build_table", "hf_envmap_sample_direction", "hf_envmap_eval",
       "hf_envmap_eval_adjoint", "hf_envmap_rays", "hf_envmap_lighting", "hf_envmap_lighting_adjoint",
       "hf_envmap_lighting_tangent")


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS, ("envmap_lighting", "envmap_rays", "Envmap"))


def test_table_size():
    from hf_amd import _capi
    lib = _capi.lib()
    assert lib.hf_envmap_table_floats(2, 2) == 4 + 1 + 1
    assert lib.hf_envmap_table_floats(17, 9) == 4 + 8 + 8 * 16
    assert lib.hf_envmap_table_floats(65537, 32769) == 4 + 32768 + 32768 * 65536     # no 32-bit overflow
    assert lib.hf_envmap_table_floats(1, 9) == 0 and lib.hf_envmap_table_floats(17, 1) == 0


NAN, INF = float("nan"), float("inf")


def _call(lib, fn, n=8, spp=2, num_rays=8, k=3, W=17, H=9, u=0.25, albedo=0.5, rot=None, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    R = None if rot is None else C.byref((C.c_float * 9)(*rot))
    env = (W, H, arg("data"), arg("table"), R)
    if fn == "hf_envmap_build_table":
        return lib.hf_envmap_build_table(W, H, arg("data"), u, arg("table"), None)
    if fn == "hf_envmap_sample_direction":
        return lib.hf_envmap_sample_direction(n, rows("sample", 2), *env, rows("out_d"), arg("out_weight"), arg("out_pdf"),
                                              arg("out_cell"), rows("out_frac", 2), None)
    if fn == "hf_envmap_eval":
        return lib.hf_envmap_eval(n, rows("d"), arg("active"), W, H, arg("data"), R, arg("out"), None)
    if fn == "hf_envmap_eval_adjoint":
        return lib.hf_envmap_eval_adjoint(n, rows("d"), arg("active"), W, H, R, arg("grad_out"), arg("grad_data"), None)
    if fn == "hf_envmap_rays":
        return lib.hf_envmap_rays(n, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), k, 7, arg("ray_id"), *env,
                                  rows("out_o"), rows("out_d"), arg("out_maxt"), arg("out_weight"), None)
    mid = (arg("weight"), num_rays, 7, arg("ray_id"), *env, albedo)
    if fn == "hf_envmap_lighting":
        return lib.hf_envmap_lighting(arg("hf"), n, spp, rows("p"), rows("nrm"), rows("sh_n"), rows("d"), arg("t"), *mid,
                                      arg("image"), arg("vis_bits"), None)
    head = (n, spp, rows("sh_n"), rows("d"), arg("t"), *mid, arg("vis_bits"))
    if fn == "hf_envmap_lighting_adjoint":
        return lib.hf_envmap_lighting_adjoint(*head, arg("grad_image"), rows("grad_sh_n"), arg("grad_weight"), arg("grad_data"),
                                              None)
    return lib.hf_envmap_lighting_tangent(*head, rows("dsh_n"), arg("dweight"), arg("ddata"), arg("image"), None)


BAD_ROT = [{"rot": [1, 0, 0, 0, NAN, 0, 0, 0, 1]}, {"rot": [1, 0, 0, 0, 1, 0, 0, 0, -INF]}]
MAP = [{"W": 1}, {"H": 1}, {"W": 0}, {"H": 0}, {"null": ("data",)}, {"null": ("table",)}] + BAD_ROT
LIGHTING = MAP + [{"n": 7}, {"spp": 0}, {"num_rays": 0}, {"num_rays": 33}, {"n": 1 << 32, "spp": 1},
                  {"albedo": NAN}, {"albedo": -INF}, {"null": ("sh_n",)}, {"null": ("d",)}, {"null": ("t",)},
                  {"null_row": "sh_n"}, {"null_row": "d"}]
CASES = {
    "hf_envmap_build_table": [{"W": 1}, {"H": 1}, {"null": ("data",)}, {"null": ("table",)}, {"u": -0.01}, {"u": 1.01},
                              {"u": NAN}, {"u": INF}],
    "hf_envmap_sample_direction": MAP + [{"null": (x,)} for x in ("sample", "out_d", "out_weight", "out_pdf")] +
                                  [{"null_row": x} for x in ("sample", "out_d", "out_frac")],
    "hf_envmap_eval": [{"W": 1}, {"H": 1}, {"null": ("data",)}, {"null": ("d",)}, {"null": ("out",)}, {"null_row": "d"}] + BAD_ROT,
    "hf_envmap_eval_adjoint": [{"W": 1}, {"H": 1}, {"null": ("grad_data",)}, {"null": ("d",)}, {"null": ("grad_out",)},
                               {"null_row": "d"}] + BAD_ROT,
    "hf_envmap_rays": MAP + [{"k": 32}, {"k": 0xFFFFFFFF}, {"n": 1 << 32}] +
                      [{"null": (x,)} for x in ("p", "nrm", "sh_n", "d", "t", "out_o", "out_d", "out_maxt")] +
                      [{"null_row": x} for x in ("p", "nrm", "sh_n", "d", "out_o", "out_d")],
    "hf_envmap_lighting": LIGHTING + [{"null": (x,)} for x in ("hf", "p", "nrm", "image")] +
                          [{"null_row": x} for x in ("p", "nrm")],
    "hf_envmap_lighting_adjoint": LIGHTING + [{"null": (x,)} for x in ("vis_bits", "grad_image", "grad_sh_n")] +
                                  [{"null_row": "grad_sh_n"}],
    "hf_envmap_lighting_tangent": LIGHTING + [{"null": (x,)} for x in ("vis_bits", "image")] + [{"null_row": "dsh_n"}],
}


@pytest.mark.parametrize("fn", sorted(CASES))
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


def test_python_argument_checks():
    import torch
    import hf_amd
    with pytest.raises(ValueError):
        hf_amd.Envmap(torch.ones(1, 8))
    with pytest.raises(ValueError):
        hf_amd.Envmap(torch.ones(4, 8), defensive=1.5)
    env = hf_amd.Envmap(torch.ones(4, 8))
    assert env.resolution == (9, 4) and tuple(env.full().shape) == (4, 9)
    assert torch.equal(env.to_world, torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]))

"""The normal map (hf_normalmap_eval, _tangent, _adjoint) on the CPU: the entry points are declared, exported and bound,
HF_VERSION is unchanged, hf_amd.NormalMap is callable, every bad argument is refused with HF_EINVAL and a message before
anything touches a device (host addresses stand in for device pointers), n = 0 passes every check and launches nothing,
and the Python class checks its arguments."""
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_normalmap_eval", "hf_normalmap_eval_tangent", "hf_normalmap_eval_adjoint")
CLAMP, REPEAT = 0, 1


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS, ("NormalMap",))
    assert "HF_WRAP_CLAMP 0" in hdr and "HF_WRAP_REPEAT 1" in hdr


def _call(lib, fn, n=8, TW=4, TH=3, wrap=REPEAT, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    head = (n, rows("uv", 2), rows("sh_n"), rows("dp_du"), arg("active"), TW, TH, arg("tex"), wrap)
    if fn == "hf_normalmap_eval":
        return lib.hf_normalmap_eval(*head, rows("out_n"), arg("mask"), None)
    if fn == "hf_normalmap_eval_tangent":
        return lib.hf_normalmap_eval_tangent(*head, arg("dtex"), rows("duv", 2), rows("dsh_n"), rows("ddp_du"), rows("dout_n"), None)
    return lib.hf_normalmap_eval_adjoint(*head, rows("grad_out"), arg("grad_tex"), rows("grad_uv", 2), rows("grad_sh_n"),
                                         rows("grad_dp_du"), None)


SHARED = [{"n": 1 << 32}] + [{"null": (x,)} for x in ("uv", "sh_n", "dp_du", "tex")] + \
         [{"null_row": x} for x in ("uv", "sh_n", "dp_du")] + \
         [{"TW": 0}, {"TH": 0}, {"TW": 1 << 16, "TH": 1 << 15}, {"TW": (1 << 31) - 1, "TH": 2}] + \
         [{"wrap": w} for w in (-1, 2, 7)]
GRADS = ("grad_tex", "grad_uv", "grad_sh_n", "grad_dp_du")
CASES = {
    "hf_normalmap_eval": SHARED + [{"null": ("out_n",)}, {"null_row": "out_n"}],
    "hf_normalmap_eval_tangent": SHARED + [{"null": ("dout_n",)}, {"null_row": "dout_n"}] +
                                 [{"null_row": x} for x in ("duv", "dsh_n", "ddp_du")],
    "hf_normalmap_eval_adjoint": SHARED + [{"null": ("grad_out",)}, {"null_row": "grad_out"}, {"null": GRADS}] +
                                 [{"null_row": x} for x in ("grad_uv", "grad_sh_n", "grad_dp_du")],
}
MESSAGE = {"n": "2^32", "null": "NULL", "null_row": "NULL", "TW": "texels", "TH": "texels", "wrap": "wrap"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_legal_edges_and_optional_pointers_are_not_refused():
    """n = 0 passes every check and launches nothing; the largest texture, a 1 x 1 texture and both wraps; active, mask,
    every tangent and every gradient but one may be NULL"""
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        assert _call(lib, fn, n=0) == _capi.HF_OK, fn
        assert _call(lib, fn, n=0, TW=(1 << 31) - 1, TH=1, wrap=CLAMP) == _capi.HF_OK, fn
        assert _call(lib, fn, n=0, TW=1, TH=1, null=("active",)) == _capi.HF_OK, fn
    assert _call(lib, "hf_normalmap_eval", n=0, null=("mask", "active")) == _capi.HF_OK
    assert _call(lib, "hf_normalmap_eval_tangent", n=0, null=("dtex", "duv", "dsh_n", "ddp_du")) == _capi.HF_OK
    for keep in GRADS:
        assert _call(lib, "hf_normalmap_eval_adjoint", n=0, null=tuple(g for g in GRADS if g != keep)) == _capi.HF_OK, keep


def test_normalmap_python_class_checks_its_arguments():
    import numpy as np
    import torch
    import hf_amd
    nm = hf_amd.NormalMap(torch.zeros((3, 5, 7)))
    assert nm.wrap == "repeat" and nm.resolution == (7, 5)           # the reference bitmap's default wrap
    assert hf_amd.NormalMap(np.zeros((3, 2, 2)), wrap="clamp").data.dtype == torch.float32
    for bad in (torch.zeros((5, 7)), torch.zeros((4, 5, 7)), torch.zeros((3, 0, 7)), torch.zeros((3, 5, 0)), torch.zeros((1, 3, 5, 7))):
        with pytest.raises(ValueError):
            hf_amd.NormalMap(bad)
    for bad in ("mirror", "", None, 1):
        with pytest.raises(ValueError):
            hf_amd.NormalMap(torch.zeros((3, 5, 7)), wrap=bad)
    flat = hf_amd.NormalMap.flat(4, 3, device="cpu")
    assert flat.data.shape == (3, 3, 4) and flat.data[0:2].eq(0.5).all() and flat.data[2].eq(1.0).all()
    assert torch.equal(flat.decode(), torch.tensor([0.0, 0.0, 1.0])[:, None, None].expand(3, 3, 4))
    m = torch.tensor([[0.6], [0.0], [0.8]])
    assert torch.allclose(hf_amd.NormalMap(hf_amd.NormalMap.encode(m)[:, :, None]).decode()[:, :, 0], m, atol=1e-7)
    # an interaction without dp_du, and one computed without RayFlags.dPdUV
    si = hf_amd.SurfaceInteraction3f()
    si.uv, si.sh_frame = torch.zeros((2, 4)), hf_amd.Frame3f(None, None, torch.zeros((3, 4)))
    with pytest.raises(ValueError):
        flat.normal(si)
    si.dp_du = torch.zeros((3, 4))
    si.ray_flags = int(hf_amd.RayFlags.Minimal | hf_amd.RayFlags.UV | hf_amd.RayFlags.ShadingFrame)
    with pytest.raises(ValueError):
        flat.normal(si)
    with pytest.raises(ValueError):
        flat.perturb(si)

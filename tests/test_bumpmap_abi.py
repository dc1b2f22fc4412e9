"""The bump map (hf_bumpmap_eval, _tangent, _adjoint) on the CPU: the entry points are declared, exported and bound,
HF_VERSION is unchanged, hf_amd.BumpMap is callable, every bad argument -- a scale that is not finite among them -- is
refused with HF_EINVAL and a message before anything touches a device (host addresses stand in for device pointers),
n = 0 passes every check and launches nothing, and the Python class checks its arguments."""
import pytest

from abi_helpers import assert_refused, assert_symbols, stand_ins

FNS = ("hf_bumpmap_eval", "hf_bumpmap_eval_tangent", "hf_bumpmap_eval_adjoint")
CLAMP, REPEAT = 0, 1
NAN, INF = float("nan"), float("inf")
RECORD = ("uv", "sh_n", "n_geo", "dp_du", "dp_dv")


def test_symbols_declared_exported_and_bound():
    hdr = assert_symbols(FNS, ("BumpMap",))
    assert "HF_WRAP_CLAMP 0" in hdr and "HF_WRAP_REPEAT 1" in hdr


def _call(lib, fn, n=8, TW=4, TH=3, wrap=REPEAT, scale=1.0, null=(), null_row=None):
    rows, arg = stand_ins(null, null_row)
    head = (n, rows("uv", 2), rows("sh_n"), rows("n_geo"), rows("dp_du"), rows("dp_dv"), arg("active"), TW, TH, arg("tex"), wrap, scale)
    if fn == "hf_bumpmap_eval":
        return lib.hf_bumpmap_eval(*head, rows("out_n"), arg("mask"), None)
    if fn == "hf_bumpmap_eval_tangent":
        return lib.hf_bumpmap_eval_tangent(*head, arg("dtex"), rows("duv", 2), rows("dsh_n"), rows("ddp_du"), rows("ddp_dv"),
                                           rows("dout_n"), None)
    return lib.hf_bumpmap_eval_adjoint(*head, rows("grad_out"), arg("grad_tex"), rows("grad_uv", 2), rows("grad_sh_n"),
                                       rows("grad_dp_du"), rows("grad_dp_dv"), None)


SHARED = [{"n": 1 << 32}] + [{"null": (x,)} for x in RECORD + ("tex",)] + [{"null_row": x} for x in RECORD] + \
         [{"TW": 0}, {"TH": 0}, {"TW": 1 << 16, "TH": 1 << 15}, {"TW": (1 << 31) - 1, "TH": 2}] + \
         [{"wrap": w} for w in (-1, 2, 7)] + [{"scale": s} for s in (NAN, INF, -INF)]
GRADS = ("grad_tex", "grad_uv", "grad_sh_n", "grad_dp_du", "grad_dp_dv")
CASES = {
    "hf_bumpmap_eval": SHARED + [{"null": ("out_n",)}, {"null_row": "out_n"}],
    "hf_bumpmap_eval_tangent": SHARED + [{"null": ("dout_n",)}, {"null_row": "dout_n"}] +
                               [{"null_row": x} for x in ("duv", "dsh_n", "ddp_du", "ddp_dv")],
    "hf_bumpmap_eval_adjoint": SHARED + [{"null": ("grad_out",)}, {"null_row": "grad_out"}, {"null": GRADS}] +
                               [{"null_row": x} for x in ("grad_uv", "grad_sh_n", "grad_dp_du", "grad_dp_dv")],
}
MESSAGE = {"n": "2^32", "null": "NULL", "null_row": "NULL", "TW": "texels", "TH": "texels", "wrap": "wrap", "scale": "scale"}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn], MESSAGE)


def test_legal_edges_and_optional_pointers_are_not_refused():
    """n = 0 passes every check and launches nothing; the largest texture, a 1 x 1 texture, both wraps, a zero and a
    negative scale; active, mask, every tangent and every gradient but one may be NULL"""
    from hf_amd import _capi
    lib = _capi.lib()
    for fn in FNS:
        assert _call(lib, fn, n=0) == _capi.HF_OK, fn
        assert _call(lib, fn, n=0, TW=(1 << 31) - 1, TH=1, wrap=CLAMP) == _capi.HF_OK, fn
        assert _call(lib, fn, n=0, TW=1, TH=1, null=("active",)) == _capi.HF_OK, fn
        for scale in (0.0, -2.5, 3.0e38):
            assert _call(lib, fn, n=0, scale=scale) == _capi.HF_OK, (fn, scale)
    assert _call(lib, "hf_bumpmap_eval", n=0, null=("mask", "active")) == _capi.HF_OK
    assert _call(lib, "hf_bumpmap_eval_tangent", n=0, null=("dtex", "duv", "dsh_n", "ddp_du", "ddp_dv")) == _capi.HF_OK
    for keep in GRADS:
        assert _call(lib, "hf_bumpmap_eval_adjoint", n=0, null=tuple(g for g in GRADS if g != keep)) == _capi.HF_OK, keep


def test_bumpmap_python_class_checks_its_arguments():
    import numpy as np
    import torch
    import hf_amd
    bm = hf_amd.BumpMap(torch.zeros((5, 7)))
    assert bm.wrap == "repeat" and bm.scale == 1.0 and bm.resolution == (7, 5)      # the reference's defaults
    assert hf_amd.BumpMap(np.zeros((2, 2)), scale=2, wrap="clamp").data.dtype == torch.float32
    for bad in (torch.zeros(7), torch.zeros((3, 5, 7)), torch.zeros((0, 7)), torch.zeros((5, 0))):
        with pytest.raises(ValueError):
            hf_amd.BumpMap(bad)
    for bad in ("mirror", "", None, 1):
        with pytest.raises(ValueError):
            hf_amd.BumpMap(torch.zeros((5, 7)), wrap=bad)
    for bad in (NAN, INF, -INF, None, "1", True):
        with pytest.raises(ValueError):
            hf_amd.BumpMap(torch.zeros((5, 7)), scale=bad)
    flat = hf_amd.BumpMap.flat(4, 3, device="cpu", scale=0.5)
    assert flat.data.shape == (3, 4) and not flat.data.any() and flat.scale == 0.5 and flat.resolution == (4, 3)
    # an interaction without dp_dv, one without the geometric normal, and one computed without RayFlags.dPdUV
    si = hf_amd.SurfaceInteraction3f()
    si.uv, si.sh_frame, si.n = torch.zeros((2, 4)), hf_amd.Frame3f(None, None, torch.zeros((3, 4))), torch.zeros((3, 4))
    si.dp_du = torch.zeros((3, 4))
    with pytest.raises(ValueError):
        flat.normal(si)
    si.dp_dv, si.n = torch.zeros((3, 4)), None
    with pytest.raises(ValueError):
        flat.normal(si)
    si.n, si.uv = torch.zeros((3, 4)), None
    with pytest.raises(ValueError):
        flat.normal(si)
    si.uv = torch.zeros((2, 4))
    si.ray_flags = int(hf_amd.RayFlags.Minimal | hf_amd.RayFlags.UV | hf_amd.RayFlags.ShadingFrame)
    with pytest.raises(ValueError):
        flat.normal(si)
    with pytest.raises(ValueError):
        flat.perturb(si)

"""The caustic forward kernel in the SHIPPED gfx950 code object (CPU test: reads the kernel metadata notes of libhf.so,
launches nothing): hf_caustic_kernel walks per lane at six waves per SIMD like the sky and envmap kernels, so it is held
to their budget -- at most 80 VGPRs and 15 spilled VGPRs (tests/test_code_object.py).  The whole-library guards of that
file (no call, no flat access, private segment, no dynamic stack) cover the four new kernels as they cover every other."""
from test_code_object import _kernels, code_object  # noqa: F401  (the fixture and the notes reader)

MAX_VGPRS, MAX_SPILLED = 80, 15


def test_caustic_kernels_are_in_the_code_object_and_the_forward_meets_the_wave_budget(code_object):  # noqa: F811
    ks = {k["name"]: k for k in _kernels(code_object)}
    for frag in ("hf_caustic_kernel", "hf_caustic_rays_kernel", "hf_caustic_adjoint_kernel", "hf_caustic_tangent_kernel"):
        assert [n for n in ks if frag in n], f"kernel {frag} not found in {sorted(ks)}"
    hit = [k for n, k in ks.items() if "hf_caustic_kernel" in n]
    assert len(hit) == 1
    k = hit[0]
    print(k["name"], "VGPRs", k["vgpr_count"], "spilled", k["vgpr_spill_count"], "private", k["private_segment_fixed_size"])
    assert int(k["vgpr_count"]) <= MAX_VGPRS, f"{k['name']}: {k['vgpr_count']} VGPRs (cap {MAX_VGPRS})"
    assert int(k["vgpr_spill_count"]) <= MAX_SPILLED, f"{k['name']}: {k['vgpr_spill_count']} spilled VGPRs (cap {MAX_SPILLED})"

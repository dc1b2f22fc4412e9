"""The thin lens's kernels in the SHIPPED gfx950 code object (CPU test: reads the kernel metadata notes of libhf.so,
launches nothing): all eight are there exactly once (the rays kernel in both store variants, the tangent, the adjoint, the
three of the way back and the reducer of 15 columns), none has a private segment -- no spilled register, no stack --, each
fits four waves per SIMD, and the rays, tangent and projection kernels use no LDS (only the reductions of the adjoints
do).  The whole-library guards of tests/test_code_object.py (no call -- the double divisions, square roots and the disk's
sine and cosine are inlined --, no flat access) cover them as they cover every other."""
from code_object_helpers import _kernels
from test_code_object import code_object  # noqa: F401  (the fixture)

NO_LDS = ("hf_thinlens_rays_kernel", "hf_thinlens_rays_wide_kernel", "hf_thinlens_tangent_kernel", "hf_thinlens_project_kernel",
          "hf_thinlens_project_tangent_kernel")
REDUCING = ("hf_thinlens_adjoint_kernel", "hf_thinlens_project_adjoint_kernel", "hf_thinlens_sum_kernel")


def test_thinlens_kernels_have_no_private_segment(code_object):  # noqa: F811
    ks = {k["name"]: k for k in _kernels(code_object)}
    assert sum("hf_thinlens" in n for n in ks) == len(NO_LDS + REDUCING), [n for n in ks if "hf_thinlens" in n]
    for frag in NO_LDS + REDUCING:
        hit = [k for n, k in ks.items() if frag in n]
        assert len(hit) == 1, (frag, [k["name"] for k in hit])
        k = hit[0]
        print(k["name"], "VGPRs", k["vgpr_count"], "spilled", k["vgpr_spill_count"], "LDS", k["group_segment_fixed_size"])
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0, k
        assert k.get("uses_dynamic_stack", "false") == "false"
        assert int(k["vgpr_count"]) <= 128, k          # four waves per SIMD at least
        if frag in NO_LDS:
            assert int(k["group_segment_fixed_size"]) == 0, k
        else:
            assert int(k["group_segment_fixed_size"]) > 0, k

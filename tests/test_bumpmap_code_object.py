"""The bump-map kernels in the SHIPPED gfx950 code object (CPU test: reads the kernel metadata notes of libhf.so, launches
nothing): the three kernels are there, each is held to the VGPR budget of the wave count its source declares
(HF_BUMPMAP_WAVES for the forward kernel, HF_BUMPMAP_AD_WAVES for the tangent and the adjoint: 8 -> 64, 7 -> 72, 6 -> 80,
5 -> 96, 4 -> 128) and none spills a register, has a private segment or uses LDS: these kernels walk nothing.  The
whole-library guards of tests/test_code_object.py (no call, no flat access, private segment, no dynamic stack) cover the
new kernels as they cover every other."""
from code_object_helpers import assert_wave_budget, forward_kernel
from test_code_object import code_object  # noqa: F401  (the fixture)

BUDGET = {8: 64, 7: 72, 6: 80, 5: 96, 4: 128}
MAX_SPILLED = 0
KERNELS = ("hf_bumpmap_kernel", "hf_bumpmap_tangent_kernel", "hf_bumpmap_adjoint_kernel")


def test_bumpmap_kernels_are_in_the_code_object_and_meet_their_wave_budgets(code_object):  # noqa: F811
    assert_wave_budget(code_object, "HF_BUMPMAP_WAVES", "hf_bumpmap_kernel", KERNELS, BUDGET, MAX_SPILLED)
    for k in KERNELS[1:]:
        assert_wave_budget(code_object, "HF_BUMPMAP_AD_WAVES", k, KERNELS, BUDGET, MAX_SPILLED)


def test_bumpmap_kernels_have_no_private_segment_and_no_lds(code_object):  # noqa: F811
    for name in KERNELS:
        k = forward_kernel(code_object, name, KERNELS)
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 0, k

"""The medium kernels in the SHIPPED gfx950 code object (CPU test: reads the kernel metadata notes of libhf.so, launches
nothing): hf_medium_kernel walks per lane like hf_directional_kernel, once per point and light, and is held to the VGPR
budget of the wave count its source declares (HF_MEDIUM_WAVES: 6 -> 80, 5 -> 96, 4 -> 128) and to the siblings' cap of 15
spilled VGPRs.  The whole-library guards of tests/test_code_object.py (no call, no flat access, private segment, no
dynamic stack) cover the new kernels as they cover every other."""
from code_object_helpers import assert_wave_budget
from test_code_object import code_object  # noqa: F401  (the fixture)

BUDGET = {6: 80, 5: 96, 4: 128}
MAX_SPILLED = 15


def test_medium_kernels_are_in_the_code_object_and_the_forward_meets_the_wave_budget(code_object):  # noqa: F811
    assert_wave_budget(code_object, "HF_MEDIUM_WAVES", "hf_medium_kernel",
                       ("hf_medium_kernel", "hf_medium_rays_kernel", "hf_medium_adjoint_kernel", "hf_medium_tangent_kernel",
                        "hf_medium_sum_kernel"), BUDGET, MAX_SPILLED)

"""The caustic forward kernel in the SHIPPED gfx950 code object (CPU test: reads the kernel metadata notes of libhf.so,
launches nothing): hf_caustic_kernel walks per lane at six waves per SIMD like the sky and envmap kernels, so it is held
to their budget -- at most 80 VGPRs and 15 spilled VGPRs (tests/test_code_object.py).  The whole-library guards of that
file (no call, no flat access, private segment, no dynamic stack) cover the four new kernels as they cover every other."""
from code_object_helpers import assert_registers, forward_kernel
from test_code_object import code_object  # noqa: F401  (the fixture)

MAX_VGPRS, MAX_SPILLED = 80, 15


def test_caustic_kernels_are_in_the_code_object_and_the_forward_meets_the_wave_budget(code_object):  # noqa: F811
    k = forward_kernel(code_object, "hf_caustic_kernel",
                       ("hf_caustic_kernel", "hf_caustic_rays_kernel", "hf_caustic_adjoint_kernel", "hf_caustic_tangent_kernel"))
    assert_registers(k, MAX_VGPRS, MAX_SPILLED)

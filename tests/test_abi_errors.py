"""The error path of the C ABI, pinned: every early check of the trace, reparameterisation and lighting entry points
returns its code and leaves its exact message in hf_last_error_string().  The CPU test covers the checks that return
before any HIP call (NULL handle, NULL rows, bad spp / n_lights / kappa / num_rays, missing gradient rows); the GPU test
covers those that come after the handle's device check and so need a live handle.  No call here reaches a launch."""
import ctypes as C

import pytest

from hf_amd import _capi

_fp = C.c_void_p
EINVAL, EFLAGS = _capi.HF_EINVAL, _capi.HF_EFLAGS
P = 4096  # a non-NULL device address: never dereferenced, every case fails before a launch


def f3(*rows):
    return (_fp * 3)(*rows)


def _lights(n=2):
    return (_capi.hf_dir_light_t * n)(*[_capi.hf_dir_light_t((0.0, 0.0, 1.0), 1.0) for _ in range(n)])


def _rays(o=(P, P, P), d=(P, P, P), maxt=P):
    return _capi.hf_rays_t(f3(*o), f3(*d), maxt)


def _expect(rc, code, msg):
    assert (rc, _capi.lib().hf_last_error_string().decode()) == (code, msg)


# argument names of each entry point, in order (include/hf.h)
ARGS = {
    "hf_direct_lighting_weighted": "n spp sh_n d t weight n_lights lights albedo vis image stream",
    "hf_direct_lighting": "n spp sh_n d t n_lights lights albedo vis image stream",
    "hf_direct_lighting_weighted_adjoint": "n spp sh_n d t weight n_lights lights albedo vis grad_image grad_sh_n "
                                           "grad_weight stream",
    "hf_direct_lighting_adjoint": "n spp sh_n d t n_lights lights albedo vis grad_image grad_sh_n stream",
    "hf_direct_lighting_weighted_tangent": "n spp sh_n d t weight n_lights lights albedo vis dsh_n dweight dimage stream",
    "hf_point_lighting": "n spp sh_n d t p n_lights lights albedo vis image stream",
    "hf_point_lighting_adjoint": "n spp sh_n d t p n_lights lights albedo vis grad_image grad_sh_n grad_p stream",
    "hf_point_lighting_tangent": "n spp sh_n d t p n_lights lights albedo vis dsh_n dp dimage stream",
    "hf_reparam_aux_rays": "n o d active k kappa antithetic seed ray_id aux_d aux_maxt stream",
    "hf_reparam_weights": "mode n o d active k kappa exponent antithetic seed ray_id si_t si_p si_bt Z dZ grad_dir "
                          "grad_div grad_p grad_t grad_vd stream",
    "hf_reparam_trace": "hf n o d active k kappa antithetic seed ray_id out_pi out_si stream",
    "hf_reparam_trace_all": "hf n o d active num kappa antithetic seed ray_id out_pi out_si stride stream",
    "hf_reparam_backward": "hf n o d active num kappa exponent antithetic seed ray_id pi si_bt stride grad_dir grad_div "
                           "grad_h stream",
}


def _defaults(handle):
    """a complete argument set; each case below breaks one argument of it"""
    return dict(n=64, spp=4, sh_n=f3(P, P, P), d=f3(P, P, P), t=P, weight=None, n_lights=2, lights=_lights(),
                albedo=0.5, vis=None, image=P, grad_image=P, grad_sh_n=f3(P, P, P), grad_weight=None, dsh_n=None,
                dweight=None, dimage=P, p=f3(P, P, P), grad_p=f3(P, P, P), dp=None, stream=None,
                mode=0, o=f3(P, P, P), active=None, k=0, kappa=100.0, exponent=3.0, antithetic=0, seed=1, ray_id=None,
                aux_d=f3(P, P, P), aux_maxt=P, si_t=P, si_p=f3(P, P, P), si_bt=P, Z=P, dZ=f3(P, P, P),
                grad_dir=f3(P, P, P), grad_div=P, grad_t=P, grad_vd=None, hf=handle, out_pi=None,
                out_si=C.byref(_capi.hf_si_t()), num=1, stride=64,
                pi=C.byref(_capi.hf_pi_t(P, (_fp * 2)(P, P), P)), grad_h=P)


def _call(fn, handle, **over):
    a = _defaults(handle)
    a.update(over)
    return getattr(_capi.lib(), fn)(*[a[k] for k in ARGS[fn].split()])


DIRECT = ["hf_direct_lighting_weighted", "hf_direct_lighting", "hf_direct_lighting_weighted_adjoint",
          "hf_direct_lighting_adjoint", "hf_direct_lighting_weighted_tangent"]
POINT = ["hf_point_lighting", "hf_point_lighting_adjoint", "hf_point_lighting_tangent"]
# the name each lighting entry reports (the unweighted forms report as their weighted ones do)
WHO = {"hf_direct_lighting_weighted": "hf_direct_lighting", "hf_direct_lighting": "hf_direct_lighting",
       "hf_direct_lighting_weighted_adjoint": "hf_direct_lighting_adjoint",
       "hf_direct_lighting_adjoint": "hf_direct_lighting_adjoint",
       "hf_direct_lighting_weighted_tangent": "hf_direct_lighting_weighted_tangent",
       "hf_point_lighting": "hf_point_lighting", "hf_point_lighting_adjoint": "hf_point_lighting_adjoint",
       "hf_point_lighting_tangent": "hf_point_lighting_tangent"}

LIGHTING_CASES = [  # (entries, broken arguments, message after "<who>: ")
    (DIRECT + POINT, dict(sh_n=None), "NULL argument"),
    (DIRECT + POINT, dict(t=None), "NULL argument"),
    (DIRECT + POINT, dict(lights=None), "NULL argument"),
    (DIRECT + POINT, dict(d=f3(P, None, P)), "NULL component array"),
    (DIRECT + POINT, dict(spp=0), "n (64) must be a multiple of spp (0)"),
    (DIRECT + POINT, dict(spp=5), "n (64) must be a multiple of spp (5)"),
    (DIRECT + POINT, dict(n_lights=0), "1..8 lights supported (got 0)"),
    (DIRECT + POINT, dict(n_lights=9, lights=_lights(9)), "1..8 lights supported (got 9)"),
    (DIRECT + POINT, dict(n=1 << 31, spp=1), "image too large"),
    (POINT, dict(p=None), "NULL position array"),
    (POINT, dict(p=f3(P, P, None)), "NULL position array"),
    (["hf_direct_lighting_weighted", "hf_direct_lighting", "hf_point_lighting"], dict(image=None), "NULL image"),
    (["hf_direct_lighting_weighted_tangent", "hf_point_lighting_tangent"], dict(dimage=None), "NULL image"),
    (["hf_direct_lighting_weighted_adjoint", "hf_direct_lighting_adjoint", "hf_point_lighting_adjoint"],
     dict(grad_image=None), "NULL gradient array"),
    (["hf_direct_lighting_weighted_adjoint", "hf_direct_lighting_adjoint", "hf_point_lighting_adjoint"],
     dict(grad_sh_n=None), "NULL gradient array"),
    (["hf_direct_lighting_weighted_adjoint", "hf_direct_lighting_adjoint", "hf_point_lighting_adjoint"],
     dict(grad_sh_n=f3(None, P, P)), "NULL gradient array"),
    (["hf_point_lighting_adjoint"], dict(grad_p=None), "NULL gradient array"),
    (["hf_point_lighting_adjoint"], dict(grad_p=f3(P, P, None)), "NULL gradient array"),
    (["hf_direct_lighting_weighted_tangent"], dict(dsh_n=f3(P, None, P)), "NULL dsh_n component array"),
    (["hf_point_lighting_tangent"], dict(dsh_n=f3(P, None, P)), "NULL tangent component array"),
    (["hf_point_lighting_tangent"], dict(dp=f3(None, P, P)), "NULL tangent component array"),
]


def test_lighting_and_reparam_entries_fail_early_with_their_messages():
    hf = C.create_string_buffer(4096)   # a stand-in handle: the checks below fail before anything reads it
    fake = C.cast(hf, C.c_void_p)
    for fns, over, msg in LIGHTING_CASES:
        for fn in fns:
            _expect(_call(fn, None, **over), EINVAL, f"{WHO[fn]}: {msg}")

    for over, msg in [(dict(o=None), "NULL argument"), (dict(d=f3(P, None, P)), "NULL argument"),
                      (dict(aux_d=f3(P, P, None)), "NULL argument"), (dict(aux_maxt=None), "NULL argument"),
                      (dict(kappa=0.0), "kappa must be > 0"), (dict(n=1 << 32), "more than 2^32 rays")]:
        _expect(_call("hf_reparam_aux_rays", None, **over), EINVAL, f"hf_reparam_aux_rays: {msg}")
    m1 = "mode 1 needs si_p, grad_direction, grad_divergence, grad_p, grad_t"
    for over, msg in [(dict(o=None), "NULL argument"), (dict(si_bt=None), "NULL argument"),
                      (dict(dZ=f3(P, None, P)), "NULL argument"), (dict(mode=2), "mode must be 0 or 1"),
                      (dict(mode=1, si_p=f3(None, P, P)), m1), (dict(mode=1, grad_dir=None), m1),
                      (dict(mode=1, grad_p=f3(P, P, None)), m1), (dict(mode=1, grad_t=None), m1),
                      (dict(kappa=-1.0), "kappa must be > 0"), (dict(n=1 << 32), "more than 2^32 rays")]:
        _expect(_call("hf_reparam_weights", None, **over), EINVAL, f"hf_reparam_weights: {msg}")

    for fn in ("hf_reparam_trace", "hf_reparam_trace_all"):
        _expect(_call(fn, fake, o=f3(P, None, P)), EINVAL, f"{fn}: NULL argument")
        _expect(_call(fn, fake, d=None), EINVAL, f"{fn}: NULL argument")
        _expect(_call(fn, None), EINVAL, f"{fn}: NULL argument")

    # hf_reparam_backward checks its arguments before the handle's device
    for over, code, msg in [(dict(hf=None), EINVAL, "NULL handle"), (dict(o=None), EINVAL, "NULL argument"),
                            (dict(si_bt=None), EINVAL, "NULL argument"),
                            (dict(grad_dir=f3(P, None, P)), EINVAL, "NULL argument"),
                            (dict(grad_div=None), EINVAL, "NULL argument"), (dict(grad_h=None), EINVAL, "NULL argument"),
                            (dict(pi=None), EINVAL, "NULL pi"),
                            (dict(pi=C.byref(_capi.hf_pi_t(P, (_fp * 2)(P, None), P))), EINVAL,
                             "NULL preliminary-intersection array"),
                            (dict(kappa=0.0), EINVAL, "kappa must be > 0"),
                            (dict(num=0), EINVAL, "1..32 auxiliary rays per ray (got 0)"),
                            (dict(num=33), EINVAL, "1..32 auxiliary rays per ray (got 33)"),
                            (dict(num=2, stride=63), EINVAL, "sample_stride < n"),
                            (dict(n=1 << 32, stride=1 << 32), EINVAL, "more than 2^32 rays")]:
        _expect(_call("hf_reparam_backward", fake, **over), code, f"hf_reparam_backward: {msg}")


def test_trace_entries_fail_early_with_their_messages():
    lib = _capi.lib()
    hf = C.cast(C.create_string_buffer(4096), C.c_void_p)
    pi, si = C.byref(_capi.hf_pi_t(P, (_fp * 2)(P, P), P)), C.byref(_capi.hf_si_t())
    g, tan = C.byref(_capi.hf_si_grad_t()), C.byref(_capi.hf_si_tangent_t())
    calls = {
        "hf_ray_intersect_preliminary": lambda h, r: lib.hf_ray_intersect_preliminary(h, 64, r, None, pi, None),
        "hf_ray_test": lambda h, r: lib.hf_ray_test(h, 64, r, None, P, None),
        "hf_ray_intersect": lambda h, r: lib.hf_ray_intersect(h, 64, r, 0, None, None, si, None),
        "hf_compute_surface_interaction": lambda h, r: lib.hf_compute_surface_interaction(h, 64, r, pi, 0, None, si, None),
        "hf_adjoint": lambda h, r: lib.hf_adjoint(h, 64, r, pi, 0, None, g, P, None, None, None),
        "hf_tangent": lambda h, r: lib.hf_tangent(h, 64, r, pi, 0, None, P, None, None, tan, None),
    }
    for fn, call in calls.items():
        _expect(call(None, C.byref(_rays())), EINVAL, f"{fn}: NULL argument")
        _expect(call(hf, None), EINVAL, f"{fn}: NULL argument")
        _expect(call(hf, C.byref(_rays(o=(P, None, P)))), EINVAL, f"{fn}: NULL ray component array")
        _expect(call(hf, C.byref(_rays(d=(P, P, None)))), EINVAL, f"{fn}: NULL ray component array")
        _expect(call(hf, C.byref(_rays(maxt=None))), EINVAL, f"{fn}: NULL ray maxt array")

    h3 = (C.c_float * 3)()
    rows = f3(C.addressof(h3), C.addressof(h3), C.addressof(h3))
    for fn, extra in (("hf_ray_intersect_preliminary_packet", (C.addressof(h3), None, None)),
                      ("hf_ray_test_packet", (C.addressof(h3),))):
        call = getattr(lib, fn)
        _expect(call(None, 1, rows, rows, C.addressof(h3), None, *extra), EINVAL, f"{fn}: NULL argument")
        _expect(call(hf, 17, rows, rows, C.addressof(h3), None, *extra), EINVAL, f"{fn}: packet of 17 rays (at most 16)")
        _expect(call(hf, 1, rows, f3(None, C.addressof(h3), C.addressof(h3)), C.addressof(h3), None, *extra), EINVAL,
                f"{fn}: NULL ray component array")
        _expect(call(hf, 1, rows, rows, C.addressof(h3), None, *((None,) * len(extra))), EINVAL, f"{fn}: NULL output")


@pytest.mark.gpu
def test_trace_entries_fail_after_the_device_check_with_their_messages(hf):
    """The checks behind check_rays, with a live handle.  Every pointer is a real buffer large enough for what it names,
    so that no case can touch memory it does not own."""
    import torch
    dev = torch.device("cuda", 0)
    shape = hf.Heightfield(heightfield=hf.workload.sine_heights(16, 16).to(dev), max_height=0.5)
    lib = _capi.lib()
    n, S = 64, 33 * 64
    buf = torch.zeros(32, S, device=dev)
    row = [int(buf[k].data_ptr()) for k in range(32)]
    rays = C.byref(_capi.hf_rays_t(f3(*row[0:3]), f3(*row[3:6]), row[6]))
    o, d = f3(*row[0:3]), f3(*row[3:6])
    pi_t = _capi.hf_pi_t(row[7], (_fp * 2)(row[8], row[9]), row[10])
    si_t = _capi.hf_si_t()
    si_t.t = row[11]
    pi, si = C.byref(pi_t), C.byref(si_t)
    h = shape._h

    _expect(lib.hf_ray_intersect_preliminary(h, n, rays, None, None, None), EINVAL,
            "hf_ray_intersect_preliminary: NULL output")
    _expect(lib.hf_ray_intersect_preliminary(h, n, rays, None, C.byref(_capi.hf_pi_t()), None), EINVAL,
            "hf_ray_intersect_preliminary: NULL output")
    _expect(lib.hf_ray_test(h, n, rays, None, None, None), EINVAL, "hf_ray_test: NULL output")
    _expect(lib.hf_ray_intersect(h, n, rays, 0x180, None, pi, si, None), EFLAGS,
            "hf_ray_intersect: Invalid combination of RayFlags: DetachShape | FollowShape")
    _expect(lib.hf_ray_intersect(h, n, rays, 0, None, pi, None, None), EINVAL, "hf_ray_intersect: NULL output")

    for fn, extra in (("hf_reparam_trace", ()), ("hf_reparam_trace_all", (n,))):
        call = getattr(lib, fn)

        def go(kappa=100.0, num=1, out_si=si, extra=extra):
            first = 0 if fn == "hf_reparam_trace" else num
            return call(h, n, o, d, None, first, kappa, 0, 1, None, pi, out_si, *extra, None)

        _expect(go(out_si=None), EINVAL, f"{fn}: NULL output")
        _expect(go(kappa=0.0), EINVAL, f"{fn}: kappa must be > 0")
        _expect(go(kappa=float("nan")), EINVAL, f"{fn}: kappa must be > 0")
    call = lib.hf_reparam_trace_all
    for num, stride, msg in ((0, n, "1..32 auxiliary rays per ray (got 0)"), (33, n, "1..32 auxiliary rays per ray (got 33)"),
                             (2, n - 1, "sample_stride < n")):
        _expect(call(h, n, o, d, None, num, 100.0, 0, 1, None, pi, si, stride, None), EINVAL, f"hf_reparam_trace_all: {msg}")
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0   # nothing was launched
    del shape

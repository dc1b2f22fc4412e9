"""Transform derivatives on the CPU: the four to_world entry points are declared, exported and bound; NULL handles are
refused; the float64 restatement (tests/xform_ref.py), differentiated by central differences in to_world, reproduces
the reference's test08 answers (src/shapes/tests/test_rectangle.py:176-272) on flat grids, which are the rectangle."""
import os

import numpy as np
import pytest
import torch

from abi_helpers import assert_symbols
import xform_ref as X

NEW = ("hf_adjoint_transform", "hf_tangent_transform", "hf_sample_position_adjoint_transform",
       "hf_sample_position_tangent_transform")


def test_new_symbols_declared_exported_and_bound():
    assert_symbols(NEW)


def test_null_handle_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    cases = [
        ("hf_adjoint_transform", lambda: lib.hf_adjoint_transform(None, 0, None, None, 0, None, None, None, None, None,
                                                                  None, None, None)),
        ("hf_tangent_transform", lambda: lib.hf_tangent_transform(None, 0, None, None, 0, None, None, None, None, None,
                                                                  None, None)),
        ("hf_sample_position_adjoint_transform",
         lambda: lib.hf_sample_position_adjoint_transform(None, 0, None, None, None, None, None, None, None, None)),
        ("hf_sample_position_tangent_transform",
         lambda: lib.hf_sample_position_tangent_transform(None, 0, None, None, None, None, None, None, None, None)),
    ]
    for name, call in cases:
        assert call() == _capi.HF_EINVAL, name
        assert lib.hf_last_error_string().decode().startswith(name + ":"), lib.hf_last_error_string()


def _fd_theta(case, W, H, smooth, eps=1e-6):
    """d/dtheta at 0 of the float64 SI block for one test08 case on a flat W x H grid (heights 0: the plane z = 0)"""
    name, mode, T, xy, _ = case
    o, d = X.test08_ray(xy)
    prim, b = X.test08_prim(W, H, *xy)
    h = torch.zeros((H, W), dtype=torch.float64)
    o_, d_ = torch.tensor(o)[None], torch.tensor(d)[None]
    pr = torch.tensor([prim])
    bf = (torch.tensor([b[0]], dtype=torch.float64), torch.tensor([b[1]], dtype=torch.float64))

    def blk(th):
        return X.si_block(h, 1.0, torch.from_numpy(T(th)), False, o_, d_, pr, bf, mode, smooth,
                          tw_frozen=torch.from_numpy(T(0.0)))[:, 0].numpy()
    # the ray hits the triangle at theta = 0 (a check of test08_prim)
    b0 = X.si_block(h, 1.0, torch.from_numpy(T(0.0)), False, o_, d_, pr, bf, "default", smooth)[:, 0].numpy()
    assert np.allclose(b0[1:4], [xy[0], xy[1], 0.0]) and np.isclose(b0[0], 2.0)
    return (blk(eps) - blk(-eps)) / (2 * eps)


@pytest.mark.parametrize("grid", [(2, 2), (5, 4)])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("case", X.TEST08, ids=[c[0] for c in X.TEST08])
def test_reference_test08_answers(case, grid, smooth):
    got = _fd_theta(case, *grid, smooth)
    for field, want in case[4].items():
        a, b = X.ROWS[field]
        assert np.allclose(got[a:b], want, atol=1e-6), (case[0], field, got[a:b], want)
    a, b = X.ROWS["sh_n"]
    assert np.allclose(got[a:b], 0.0, atol=1e-6)   # a flat grid's shading normal turns with n: zero in every case
    if case[1] == "detach":
        assert np.allclose(got, 0.0, atol=1e-9)


def test_fd_of_the_reference_matches_its_autograd():
    """the yardstick itself: central differences in to_world against torch autograd of the same float64 expression,
    on a rough field, a general affine, smooth shading, all three modes"""
    import common
    rng = np.random.default_rng(3)
    W, H = 7, 6
    h = torch.from_numpy(rng.uniform(0, 1, (H, W)))
    tw = common.affine(4).astype(np.float64)
    n = 16
    prim = torch.from_numpy(rng.integers(0, 2 * (W - 1) * (H - 1), n))
    b1 = torch.from_numpy(rng.uniform(0.05, 0.45, n)); b2 = torch.from_numpy(rng.uniform(0.05, 0.45, n))
    # rays through the frozen points, from above
    V = X.S.world_vertices(h, 0.6, torch.from_numpy(tw)).reshape(-1, 3)
    f = X.S.grid_faces(W, H)[prim]
    p = (1 - b1 - b2)[:, None] * V[f[:, 0]] + b1[:, None] * V[f[:, 1]] + b2[:, None] * V[f[:, 2]]
    d = torch.from_numpy(rng.normal(size=(n, 3))) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    o = p - 2.0 * d
    g = torch.from_numpy(rng.normal(size=(18, n)))
    for mode in ("default", "follow", "detach"):
        for smooth in (False, True):
            def L(t):
                return float((X.si_block(h, 0.6, t, True, o, d, prim, (b1, b2), mode, smooth,
                                         tw_frozen=torch.from_numpy(tw)) * g).sum())
            fd = X.fd_to_world(L, tw)
            t = torch.from_numpy(tw).clone().requires_grad_(True)
            out = (X.si_block(h, 0.6, t, True, o, d, prim, (b1, b2), mode, smooth) * g).sum()
            ad = torch.autograd.grad(out, t)[0].numpy() if out.requires_grad else np.zeros((3, 4))
            assert np.allclose(fd, ad, rtol=1e-5, atol=1e-6 * np.abs(ad).max() + 1e-9), (mode, smooth, fd, ad)
            if mode == "detach":
                assert np.all(ad == 0)


def test_transform_kernels_keep_to_the_code_object_guards():
    """the new instantiations: no spilled VGPRs and at most the 48-byte private segment of hf_adjoint_smooth_kernel
    (tests/test_code_object.py checks the 64-byte cap, calls and flat accesses for every kernel)"""
    import tempfile
    import test_code_object as T
    if not os.path.exists(os.path.join(T.LLVM, "llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(T._code_object()); f.flush()
        ks = [k for k in T._kernels(f.name) if "xform" in k["name"]]
    names = " ".join(k["name"] for k in ks)
    for frag in ("hf_adjoint_xform_kernel", "hf_adjoint_xform_smooth_kernel", "hf_tangent_xform_kernel",
                 "hf_tangent_xform_smooth_kernel", "hf_sample_adjoint_xform_kernel", "hf_sample_tangent_xform_kernel",
                 "hf_xform_sum_kernel"):
        assert frag in names, frag
    for k in ks:
        assert int(k["vgpr_spill_count"]) == 0, k["name"]
        assert int(k["private_segment_fixed_size"]) <= 48, k["name"]

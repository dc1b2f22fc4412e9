"""eval_parameterization on the CPU: the three entry points are declared, exported and bound; NULL handles are refused;
the float64 restatement (tests/param_ref.py) reproduces the reference's known answers (src/render/tests/test_mesh.py
test09, src/shapes/tests/test_rectangle.py test09), its closed-form lookup agrees with Mesh's way -- a float64
Moeller-Trumbore over the texcoord mesh -- on random points and on every exact border, diagonal and corner, and its
derivatives agree with central differences; the adapter overrides the method."""
import os
import re

import numpy as np
import torch

from abi_helpers import assert_symbols
import common
import param_ref as R
from si_numpy import RAY_ALL, RAY_DPDUV, RAY_SHADINGFRAME, RAY_UV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hf_eval_parameterization", "hf_eval_parameterization_adjoint", "hf_eval_parameterization_tangent")


def test_new_symbols_declared_exported_and_bound():
    assert_symbols(NEW)
    import hf_amd.shape as sh
    assert callable(getattr(sh.Heightfield, "eval_parameterization", None))


def test_null_handle_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    cases = [
        ("hf_eval_parameterization", lambda: lib.hf_eval_parameterization(None, 0, None, 0, None, None, None, None)),
        ("hf_eval_parameterization_adjoint",
         lambda: lib.hf_eval_parameterization_adjoint(None, 0, None, 0, None, None, None, None, None)),
        ("hf_eval_parameterization_tangent",
         lambda: lib.hf_eval_parameterization_tangent(None, 0, None, 0, None, None, None, None, None)),
    ]
    for name, call in cases:
        assert call() == _capi.HF_EINVAL, name
        assert lib.hf_last_error_string().decode().startswith(name + ":"), lib.hf_last_error_string()


def _rect(tw=np.eye(4)[:3]):
    """the reference rectangle: a 2x2 heightfield with zero heights"""
    return torch.zeros((2, 2), dtype=torch.float64), 1.0, np.asarray(tw, np.float64)


def test_known_answers_of_the_reference_mesh_test09():
    h, s, tw = _rect()
    u = np.array([-0.01, 1 - 1e-7, 1e-7, 0.2], np.float32)
    v = np.array([0.5, 1 - 1e-7, 1e-7, 0.3], np.float32)
    valid, prim, b1, b2 = R.lookup(u, v, 2, 2)
    assert valid.tolist() == [False, True, True, True]
    r = R.record(h, s, tw, False, u[1:], v[1:], prim[1:], b1[1:], b2[1:], RAY_ALL)
    expect = np.array([[1, 1, 0], [-1, -1, 0], [-0.6, -0.4, 0]])
    assert np.allclose(r["p"].numpy(), expect, atol=1e-6), r["p"]
    assert np.allclose(r["uv"].numpy(), np.stack([u[1:], v[1:]], -1), atol=1e-7)


def test_uv_does_not_change_with_to_world():
    """test_rectangle.py test09: the uv of a point is a property of the surface, not of its placement"""
    u = np.array([0.2, 0.7, 0.5, 0.999], np.float32)
    v = np.array([0.3, 0.1, 0.5, 0.001], np.float32)
    valid, prim, b1, b2 = R.lookup(u, v, 2, 2)
    assert valid.all()
    out = []
    for tw in (np.eye(4)[:3], common.affine(3).astype(np.float64)):
        h, s, tw = _rect(tw)
        r = R.record(h, s, tw, False, u, v, prim, b1, b2, RAY_UV | RAY_DPDUV | RAY_SHADINGFRAME)
        out.append(r["uv"].numpy())
    assert np.allclose(out[0], out[1], atol=1e-7) and np.allclose(out[0], np.stack([u, v], -1), atol=1e-7)


def test_lookup_agrees_with_brute_force_on_random_points():
    rng = np.random.default_rng(1)
    for W, H in ((2, 2), (9, 7), (13, 4)):
        u = rng.uniform(0, 1, 4000).astype(np.float32)
        v = rng.uniform(0, 1, 4000).astype(np.float32)
        # away from every edge by more than 1e-6 of a cell: cell borders and the diagonal
        fx, fy = u.astype(np.float64) * (W - 1) % 1.0, v.astype(np.float64) * (H - 1) % 1.0
        far = (np.minimum(fx, 1 - fx) > 1e-6) & (np.minimum(fy, 1 - fy) > 1e-6) & (np.abs(fx + fy - 1) > 1e-6)
        valid, prim, _, _ = R.lookup(u, v, W, H)
        ref, cnt = R.brute_force(u, v, W, H)
        assert valid.all()
        assert far.sum() > 3900
        assert np.array_equal(prim[far], ref[far]), (W, H)
        assert (cnt[far] == 1).all()


def _exact_points(W, H):
    """every vertex, every cell-border midpoint and quarter point, every diagonal point of a grid with power-of-two cell
    counts (the texcoords are exact in float32 and float64), u, v in {0, 1} included"""
    cw, ch = W - 1, H - 1
    a = np.array([0.0, 0.25, 0.5, 0.75])
    pts = []
    for cy in range(ch):
        for cx in range(cw):
            for t in a:
                pts += [((cx + t) / cw, cy / ch), (cx / cw, (cy + t) / ch), ((cx + t) / cw, (cy + 1 - t) / ch)]
    pts += [(j / cw, i / ch) for i in range(H) for j in range(W)]
    pts += [(t, 1.0) for t in np.linspace(0, 1, 17)] + [(1.0, t) for t in np.linspace(0, 1, 17)]
    p = np.array(pts, np.float64)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p[:, 0].astype(np.float32), p[:, 1].astype(np.float32)


def test_lookup_takes_the_highest_index_on_edges_diagonals_and_corners():
    for W, H in ((2, 2), (9, 5), (5, 9)):
        u, v = _exact_points(W, H)
        valid, prim, b1, b2 = R.lookup(u, v, W, H)
        ref, cnt = R.brute_force(u, v, W, H)
        assert valid.all() and (cnt >= 1).all()
        assert (cnt > 1).sum() >= 8                 # ties: the diagonals, and inner borders and corners
        assert np.array_equal(prim, ref), (W, H, u[prim != ref], v[prim != ref])
        # the barycentrics place the point where it was asked for
        T = R.texcoord_triangles(W, H)[prim]
        q = (1 - b1.astype(np.float64) - b2)[:, None] * T[:, 0] + b1[:, None] * T[:, 1] + b2[:, None] * T[:, 2]
        assert np.allclose(q, np.stack([u, v], -1), atol=1e-7)


def test_invalid_queries():
    u = np.array([np.nan, 0.5, -1e-30, 1.0000001, 0.5, -0.0, 1.0], np.float32)
    v = np.array([0.5, np.nan, 0.5, 0.5, 1.0000001, 0.0, 1.0], np.float32)
    valid, prim, b1, b2 = R.lookup(u, v, 9, 7)
    assert valid.tolist() == [False] * 5 + [True, True]
    assert prim[5] == 0 and prim[6] == 2 * 8 * 6 - 1 and (b1[6], b2[6]) == (0, 0)
    valid, _, _, _ = R.lookup(np.float32([0.5, 0.5]), np.float32([0.5, 0.5]), 9, 7, active=[True, False])
    assert valid.tolist() == [True, False]


def _case(smooth, seed=0, W=5, H=4):
    rng = np.random.default_rng(seed)
    h = torch.from_numpy(rng.uniform(0.2, 0.8, (H, W))).double()
    tw = common.affine(seed + 2).astype(np.float64)
    u = rng.uniform(0.02, 0.98, 24).astype(np.float32)
    v = rng.uniform(0.02, 0.98, 24).astype(np.float32)
    _, prim, b1, b2 = R.lookup(u, v, W, H)
    wts = torch.from_numpy(rng.normal(size=(18, 24)))
    wts[0] = 0.0   # t and uv carry no derivative
    wts[7:9] = 0.0
    return h, tw, u, v, prim, b1, b2, wts


def test_restatement_derivatives_against_central_differences():
    for smooth in (False, True):
        h, tw, u, v, prim, b1, b2, wts = _case(smooth)
        flags = RAY_ALL | (0x20 if smooth else 0)

        def loss(hh, tt):
            return (R.block(R.record(hh, 0.6, tt, False, u, v, prim, b1, b2, flags, smooth)) * wts).sum()
        hh = h.clone().requires_grad_(True)
        tt = torch.from_numpy(tw).clone().requires_grad_(True)
        loss(hh, tt).backward()
        eps = 1e-6
        for k in range(0, h.numel(), 3):
            dh = torch.zeros_like(h).reshape(-1)
            dh[k] = eps
            dh = dh.reshape(h.shape)
            fd = (loss(h + dh, torch.from_numpy(tw)) - loss(h - dh, torch.from_numpy(tw))) / (2 * eps)
            assert abs(float(fd) - float(hh.grad.reshape(-1)[k])) <= 1e-6 * (1 + abs(float(fd))), (smooth, k)
        for k in range(12):
            d = np.zeros(12); d[k] = eps
            d = d.reshape(3, 4)
            fd = (loss(h, torch.from_numpy(tw + d)) - loss(h, torch.from_numpy(tw - d))) / (2 * eps)
            assert abs(float(fd) - float(tt.grad.reshape(-1)[k])) <= 1e-6 * (1 + abs(float(fd))), (smooth, k)


def test_adapter_overrides_eval_parameterization():
    src = open(os.path.join(ROOT, "adapters", "mitsuba3", "heightfield.cpp")).read()
    assert re.search(r"SurfaceInteraction3f\s+eval_parameterization\s*\([^)]*\)\s*const\s+override", src)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
    assert "eval_parameterization" in open(os.path.join(ROOT, "INTEGRATION.md")).read()

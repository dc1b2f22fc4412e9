"""Area sampling on the CPU: the new entry points are declared, exported and bound; NULL handles are refused; the
float64 restatement (tests/area_ref.py) reproduces the reference's known answers (src/shapes/tests/test_rectangle.py
tests 01, 02, 05) and its grid enumeration equals the explicit face list; the adapter calls the new entries."""
import ctypes as C
import os
import re

import numpy as np
import torch

from abi_helpers import assert_symbols
import area_ref as A
import common
import smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hf_set_area_sampling", "hf_surface_area", "hf_area_cdf", "hf_sample_position", "hf_sample_position_adjoint",
       "hf_sample_position_tangent")


def test_new_symbols_declared_exported_and_bound():
    assert_symbols(NEW)


def test_null_handle_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    f = C.c_float()
    cases = [
        ("hf_set_area_sampling", lambda: lib.hf_set_area_sampling(None, 1, None)),
        ("hf_surface_area", lambda: lib.hf_surface_area(None, C.byref(f), None)),
        ("hf_area_cdf", lambda: lib.hf_area_cdf(None, None, None)),
        ("hf_sample_position", lambda: lib.hf_sample_position(None, 0, None, None, None, None)),
        ("hf_sample_position_adjoint", lambda: lib.hf_sample_position_adjoint(None, 0, None, None, None, None, None, None, None)),
        ("hf_sample_position_tangent", lambda: lib.hf_sample_position_tangent(None, 0, None, None, None, None, None, None, None)),
    ]
    for name, call in cases:
        assert call() == _capi.HF_EINVAL, name
        assert lib.hf_last_error_string().decode().startswith(name + ":"), lib.hf_last_error_string()


def _flat_area(tw, W=5, H=4):
    h = torch.full((H, W), 0.5, dtype=torch.float64)
    return float(A.areas(h, 0.7, np.asarray(tw, np.float64)).sum())


def test_known_answers_of_the_reference_rectangle():
    eye = np.eye(4)[:3]
    assert np.isclose(_flat_area(eye), 4.0, rtol=1e-12)                                   # test01
    for sx in (1, 2, 4):                                                                   # test02
        for tr in ((1.3, -3.0, 5.0), (-10000.0, 3.0, 31.0)):
            tw = np.diag([sx, 2.5, 1.0, 1.0])[:3].copy()
            tw[:, 3] = tr
            assert np.isclose(_flat_area(tw), 4.0 * sx * 2.5, rtol=1e-9)
    tw = np.diag([2.0, 2.0, 1.0, 1.0])[:3]                                                 # test05
    assert np.isclose(_flat_area(tw), 16.0, rtol=1e-12)
    tw = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0]], np.float64)
    assert np.isclose(_flat_area(tw), 4.0 * np.sqrt(2.0), rtol=1e-12)
    tw = np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
    assert np.isclose(_flat_area(tw), 4.0, rtol=1e-12)


def test_grid_enumeration_equals_the_explicit_face_list():
    """prim_index 2 (cy (W-1) + cx) + tri, tri 0 = (v00, v10, v01), tri 1 = (v11, v01, v10)"""
    for (W, H) in ((2, 2), (9, 7), (5, 3)):
        F = S.grid_faces(W, H).numpy()
        k = 0
        for cy in range(H - 1):
            for cx in range(W - 1):
                v00 = cy * W + cx
                assert F[k].tolist() == [v00, v00 + 1, v00 + W]
                assert F[k + 1].tolist() == [v00 + W + 1, v00 + W, v00 + 1]
                k += 2
        rng = np.random.default_rng(W * H)
        h = torch.from_numpy(rng.uniform(0, 1, (H, W)))
        tw = common.affine(W).astype(np.float64)
        V = S.world_vertices(h, 0.7, tw).reshape(-1, 3).numpy()
        explicit = [0.5 * np.linalg.norm(np.cross(V[b] - V[a], V[c] - V[a])) for a, b, c in F]
        assert np.allclose(A.areas(h, 0.7, tw).numpy(), explicit, rtol=1e-13)


def test_cdf_and_index_restatement():
    pmf = np.array([0.0, 1.0, 0.0, 2.0, 3.0, 0.0], np.float32)
    cdf, tot, s32, norm, valid = A.cdf(pmf)
    assert cdf.tolist() == [0, 1, 1, 3, 6, 6] and tot == 6.0 and valid == (1, 4)
    assert norm == np.float32(1.0 / 6.0)
    y = np.array([0.0, 1.0 / 6.0, 0.5, 0.99999994], np.float32)
    assert A.sample_index(cdf, s32, valid, y).tolist() == [1, 1, 3, 4]
    r = A.reuse(cdf, pmf, norm, np.array([3]), np.array([0.5], np.float32))
    assert np.isclose(r[0], (0.5 - 1 / 6) / (2 / 6), rtol=1e-6)
    bx, by = A.warp(np.array([0.0, 1.0, 0.75]), np.array([0.5, 0.5, 1.0]))
    assert np.allclose(bx, [0.0, 1.0, 0.5]) and np.allclose(by, [0.5, 0.0, 0.5])


def test_adapter_calls_the_new_entries():
    src = open(os.path.join(ROOT, "adapters", "mitsuba3", "heightfield.cpp")).read()
    assert 'NotImplementedError("surface_area")' not in src
    for name in ("hf_set_area_sampling", "hf_surface_area", "hf_sample_position", "hf_sample_position_adjoint"):
        assert re.search(rf"\b{name}\s*\(", src), name
    assert re.search(r"PositionSample3f\s+sample_position\s*\(", src)
    assert re.search(r"Float\s+pdf_position\s*\(", src)

"""Smooth shading on the CPU: the new entry points are declared, exported and bound; the float64 restatement
(tests/smooth_ref.py) reproduces the reference's known answer and agrees with itself between the explicit face list
and the heightfield's 1-ring enumeration; the adapter wires the property and both entry points."""
import os
import re

import numpy as np
import torch

from abi_helpers import assert_symbols
import common
import smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hf_set_face_normals", "hf_get_face_normals", "hf_shading_derivatives")


def test_new_symbols_declared_exported_and_bound():
    assert_symbols(NEW)
    from hf_amd import _capi
    assert _capi.lib().hf_get_face_normals(None) == 1      # no handle: the default mode


def test_null_handle_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    assert lib.hf_set_face_normals(None, 0, None) != 0
    assert lib.hf_shading_derivatives(None, 0, None, None, None, None, None) != 0


def test_reference_known_answer_test04_normal_weighting_scheme():
    """src/render/tests/test_mesh.py:74-97: 5 vertices, 2 faces, normals n2, n0, n0, n1, n1"""
    a, b = 1.0, 0.5
    V = torch.tensor([[0, 0, 0], [-a, 1, 0], [a, 1, 0], [-b, 0, 1], [b, 0, 1]], dtype=torch.float64)
    F = torch.tensor([[0, 1, 2], [0, 3, 4]])
    N = R.vertex_normals_faces(V, F)
    n0 = np.array([0.0, 0.0, -1.0]); n1 = np.array([0.0, 1.0, 0.0])
    n2 = n0 * (np.pi / 2) + n1 * np.arccos(3.0 / 5.0)
    n2 /= np.linalg.norm(n2)
    ref = np.stack([n2, n0, n0, n1, n1])
    assert np.allclose(N.numpy(), ref, atol=5e-4)
    assert np.allclose(N.numpy(), ref, atol=1e-12)   # (float64: the answer is exact)


def _grid_vs_faces(W, H, seed, affine):
    rng = np.random.default_rng(seed)
    h = torch.from_numpy(rng.uniform(0, 1, (H, W)))
    tw = common.affine(seed).astype(np.float64) if affine else np.eye(4)[:3]
    P = R.world_vertices(h, 0.7, tw)
    Ng = R.vertex_normals_grid(P)
    Nf = R.vertex_normals_faces(P.reshape(-1, 3), R.grid_faces(W, H)).reshape(H, W, 3)
    return Ng, Nf


def test_ring_enumeration_equals_explicit_face_list():
    for (W, H) in ((2, 2), (2, 5), (7, 3), (9, 7), (33, 17)):
        for affine in (False, True):
            Ng, Nf = _grid_vs_faces(W, H, seed=W * 31 + H, affine=affine)
            assert torch.allclose(Ng, Nf, atol=1e-12), (W, H, affine, (Ng - Nf).abs().max())
            # borders and corners included: every texel, unit length
            assert torch.allclose(torch.linalg.norm(Ng, dim=-1), torch.ones(H, W, dtype=torch.float64))


def test_anisotropic_transform_changes_the_normals():
    """angles are not affine-invariant: the world-space normals are not the transformed object-space ones"""
    W, H = 9, 7
    rng = np.random.default_rng(3)
    h = torch.from_numpy(rng.uniform(0, 1, (H, W)))
    tw = np.concatenate([np.diag([3.0, 0.5, 1.0]), np.zeros((3, 1))], 1)
    Nw = R.vertex_normals_grid(R.world_vertices(h, 0.7, tw))
    No = R.vertex_normals_grid(R.world_vertices(h, 0.7, np.eye(4)[:3]))
    Ainv_T = torch.from_numpy(np.linalg.inv(tw[:, :3]).T)
    mapped = R._normalize(No @ Ainv_T.T)
    assert (Nw - mapped).abs().max() > 1e-3


def test_planar_field_gives_the_plane_normal():
    W, H = 11, 6
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h = torch.from_numpy(0.2 + 0.03 * j + 0.05 * i)
    for tw in (np.eye(4)[:3], common.affine(4).astype(np.float64)):
        P = R.world_vertices(h, 0.8, tw)
        N = R.vertex_normals_grid(P).reshape(-1, 3)
        face = R._normalize(torch.linalg.cross(P[0, 1] - P[0, 0], P[1, 0] - P[0, 0], dim=-1))
        assert torch.allclose(N, face.expand_as(N), atol=1e-12)


def test_adapter_reads_face_normals_and_calls_both_entries():
    src = open(os.path.join(ROOT, "adapters", "mitsuba3", "heightfield.cpp")).read()
    assert re.search(r'props\.get<bool>\("face_normals",\s*true\)', src)
    assert re.search(r"\bhf_set_face_normals\s*\(", src)
    assert re.search(r"\bhf_shading_derivatives\s*\(", src)
    assert "RayFlags::dNSdUV" in src

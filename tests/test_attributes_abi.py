"""Shape attributes on the CPU: the three new entry points are declared in include/hf.h, exported by libhf.so and bound;
NULL handles are refused with the entry point's name; the float64 restatement (tests/attr_ref.py) reproduces the known
answers of the reference's mesh_attribute test01 (src/textures/tests/test_mesh_attribute.py) on the 2x2 grid, whose
vertex order, texcoords (j / (W-1), i / (H-1)) and prim_index order coincide with that test's rectangle; the adapter
implements the attribute interface through the new entries."""
import os
import re

import numpy as np
import torch

from abi_helpers import assert_symbols
import attr_ref as R
import smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hf_eval_attribute", "hf_eval_attribute_adjoint", "hf_eval_attribute_tangent")
UV = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.3, 0.4), (0.5, 0.5)]


def _strip(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_new_symbols_declared_exported_and_bound():
    from hf_amd import _capi
    hdr = assert_symbols(NEW)
    assert re.search(r"HF_ATTR_VERTEX\s*=\s*0\s*,\s*HF_ATTR_FACE\s*=\s*1", hdr)
    assert (_capi.HF_ATTR_VERTEX, _capi.HF_ATTR_FACE) == (0, 1)


def test_null_handle_is_refused():
    from hf_amd import _capi
    lib = _capi.lib()
    cases = [
        ("hf_eval_attribute", lambda: lib.hf_eval_attribute(None, 0, 0, 1, None, None, None, None, None, None, None)),
        ("hf_eval_attribute_adjoint", lambda: lib.hf_eval_attribute_adjoint(None, 0, 0, 1, None, None, None, None, None,
                                                                            None, None, None, None, None)),
        ("hf_eval_attribute_tangent", lambda: lib.hf_eval_attribute_tangent(None, 0, 0, 1, None, None, None, None, None,
                                                                            None, None, None, None, None)),
    ]
    for name, call in cases:
        assert call() == _capi.HF_EINVAL, name
        assert lib.hf_last_error_string().decode().startswith(name + ":"), lib.hf_last_error_string()


def rectangle_hits():
    """the 2x2 grid (flat, identity to_world) at the six (u, v) of test01: world p = (2u - 1, 2v - 1, 0) and the
    triangle that contains it (tri 0 = (v00, v10, v01) for u + v <= 1, else tri 1)"""
    uv = torch.tensor(UV, dtype=torch.float64)
    p = torch.stack([2 * uv[:, 0] - 1, 2 * uv[:, 1] - 1, torch.zeros(len(UV), dtype=torch.float64)], 1)
    prim = (uv.sum(1) > 1).long()
    return uv, p, prim


# the four attributes of create_rectangle(), as [count, C]
RECT = {
    "vertex_color": ("vertex", [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]),
    "vertex_mono": ("vertex", [[1.0], [2.0], [3.0], [4.0]]),
    "face_color": ("face", [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
    "face_mono": ("face", [[0.0], [1.0]]),
}


def expected(name, uv, prim):
    u, v = uv[:, 0], uv[:, 1]
    z = torch.zeros_like(u)
    return {"vertex_color": torch.stack([u, v, z], 1),
            "vertex_mono": ((1 - v) * (1 * (1 - u) + 2 * u) + v * (3 * (1 - u) + 4 * u))[:, None],
            "face_color": torch.stack([z, z, prim.double()], 1),
            "face_mono": prim.double()[:, None]}[name]


def test_known_answers_of_the_reference_rectangle():
    uv, p, prim = rectangle_hits()
    h = torch.zeros((2, 2), dtype=torch.float64)
    for name, (kind, data) in RECT.items():
        got = R.value(kind, torch.tensor(data, dtype=torch.float64), h, 1.0, np.eye(4)[:3], prim, p)
        assert torch.allclose(got, expected(name, uv, prim), atol=1e-12), name


def test_grid_matches_the_reference_rectangle():
    """vertex i W + j of the 2x2 grid sits at texcoord (j, i) = the rectangle's vertex_texcoords, and its two triangles
    are the rectangle's faces [0, 1, 2], [1, 3, 2] (tri 1 as a rotation of the latter)"""
    F = S.grid_faces(2, 2).tolist()
    assert F[0] == [0, 1, 2]
    assert F[1] in ([1, 3, 2], [3, 2, 1], [2, 1, 3])
    V = S.world_vertices(torch.zeros((2, 2), dtype=torch.float64), 1.0, np.eye(4)[:3]).reshape(-1, 3)
    tex = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
    assert torch.equal((V[:, :2] + 1) / 2, tex)


def test_restatement_on_a_general_triangle():
    """bary reproduces p exactly for points in the plane and is invariant to the vertex rotation of tri 1"""
    g = torch.Generator().manual_seed(3)
    P = torch.rand((64, 3, 3), generator=g, dtype=torch.float64)
    b = torch.rand((64, 3), generator=g, dtype=torch.float64)
    b = b / b.sum(1, keepdim=True)
    p = (P * b[:, :, None]).sum(1)
    w, u, v = R.bary(p, P[:, 0], P[:, 1], P[:, 2])
    assert torch.allclose(torch.stack([w, u, v], 1), b, atol=1e-10)
    w2, u2, v2 = R.bary(p, P[:, 1], P[:, 2], P[:, 0])
    assert torch.allclose(torch.stack([v2, w2, u2], 1), b, atol=1e-10)


def test_adapter_implements_the_attribute_interface():
    src = _strip(open(os.path.join(ROOT, "adapters", "mitsuba3", "heightfield.cpp")).read())
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", src), name
    assert re.search(r"Mask\s+has_attribute\s*\(", src)
    assert re.search(r"UnpolarizedSpectrum\s+eval_attribute\s*\(", src)
    assert re.search(r"Float\s+eval_attribute_1\s*\(", src)
    assert re.search(r"Color3f\s+eval_attribute_3\s*\(", src)
    assert re.search(r"void\s+add_attribute\s*\(", src)
    for fallback in ("Base::has_attribute", "Base::eval_attribute", "Base::eval_attribute_1", "Base::eval_attribute_3"):
        assert fallback + "(" in src.replace(" ", ""), fallback
    assert 'attribute name must start with either \\"vertex_\\" of \\"face_\\".' in src

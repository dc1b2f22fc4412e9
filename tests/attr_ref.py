"""Float64 torch restatement of the heightfield's shape attributes, the yardstick of tests/test_attributes_abi.py and
tests/test_gpu_attributes.py.

  * bary: Mesh::barycentric_coordinates (src/render/mesh.cpp:645-667): the least-squares weights (w, u, v) of a point p
    with respect to a triangle (P0, P1, P2), in the reference's formula;
  * vertex: Mesh::interpolate_attribute for a vertex attribute (include/mitsuba/render/mesh.h:409-437):
    v0 w + v1 u + v2 v over the vertices of smooth_ref.grid_faces, at world-space positions of smooth_ref.world_vertices
    (or area_ref.world_vertices_f32, the device's rounding of them);
  * face: the row of prim_index.
Everything is plain torch, so autograd and torch.func.jvp give the reverse and forward derivatives with respect to the
attribute buffer, p and the heights.
"""
import torch

import area_ref as A
import smooth_ref as S


def bary(p, P0, P1, P2):
    """(w, u, v) [n] for p, P0, P1, P2 [n, 3]"""
    rel, du, dv = p - P0, P1 - P0, P2 - P0
    b1, b2 = (du * rel).sum(-1), (dv * rel).sum(-1)
    a11, a12, a22 = (du * du).sum(-1), (du * dv).sum(-1), (dv * dv).sum(-1)
    inv_det = 1.0 / (a11 * a22 - a12 * a12)
    u = (a22 * b1 - a12 * b2) * inv_det
    v = (a11 * b2 - a12 * b1) * inv_det
    return 1.0 - u - v, u, v


def vertex(attr, V, prim, p):
    """[n, C]: attr [H W, C], V [H, W, 3] world-space vertices, prim [n] (long), p [n, 3]"""
    H, W, _ = V.shape
    F = S.grid_faces(W, H).to(prim.device)[prim]
    P = V.reshape(-1, 3)[F]
    w, u, v = bary(p, P[:, 0], P[:, 1], P[:, 2])
    a = attr[F]
    return a[:, 0] * w[:, None] + a[:, 1] * u[:, None] + a[:, 2] * v[:, None]


def face(attr, prim):
    """[n, C]: attr [2 (W-1)(H-1), C]"""
    return attr[prim]


def value(kind, attr, h, s, tw, prim, p, hit=None, device_rounding=False):
    """[n, C] of an attribute (kind 'vertex' / 'face'; attr [count, C]) at the hits (prim, p) of heights h [H, W]
    (float64); lanes where hit is False are 0"""
    if kind == "face":
        out = face(attr, prim)
    else:
        V = A.world_vertices_f32(h, s, tw) if device_rounding else S.world_vertices(h, s, tw)
        out = vertex(attr, V, prim, p)
    if hit is not None:
        out = torch.where(hit[:, None], out, torch.zeros_like(out))
    return out

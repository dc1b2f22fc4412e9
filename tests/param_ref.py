"""Float64 restatement of eval_parameterization (Shape::eval_parameterization, Mesh: src/render/mesh.cpp:503-545,
614-635), the yardstick of tests/test_parameterization_abi.py and tests/test_gpu_parameterization.py.

  * lookup: the closed-form uv -> (prim_index, b1, b2) of param_lookup (hf_device.h) in numpy.  Every step is one IEEE
    rounding that float32 numpy (or float64 rounded once) reproduces, so prim_index and b equal the device's bit for bit;
  * brute_force: what Mesh does instead, a float64 Moeller-Trumbore over the texcoord mesh for the UV-space ray
    o = (u, v, -1), d = (0, 0, 1), returning the highest prim_index among the triangles it reports as hit;
  * record: the record at frozen (prim, b) under any RayFlags set -- smooth_ref.surface in its FollowShape mode on the
    UV-space ray, with t = 1 held constant (no derivative) -- in plain torch, so autograd and torch.func.jvp give the
    derivatives with respect to the heights and to_world.
"""
import numpy as np
import torch

import smooth_ref as S
from si_numpy import RAY_ALL


def lookup(u, v, W, H, active=None):
    """(valid [n] bool, prim [n] int64, b1 [n] float32, b2 [n] float32) for float32 query rows u, v"""
    u = np.asarray(u, np.float32).reshape(-1)
    v = np.asarray(v, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    if active is not None:
        valid &= np.asarray(active, bool).reshape(-1)
    uu, vv = np.where(valid, u, np.float32(0)), np.where(valid, v, np.float32(0))
    one = np.float32(1)

    def axis(q, cells):
        c = np.float32(cells)
        x = q * c                                                           # float32 product, one rounding
        ci = np.minimum(np.floor(x), np.float32(cells - 1))
        f = (q.astype(np.float64) * cells - ci.astype(np.float64)).astype(np.float32)   # = fma(q, cells, -ci)
        return ci.astype(np.int64), np.clip(f, np.float32(0), one)

    cx, fx = axis(uu, W - 1)
    cy, fy = axis(vv, H - 1)
    tri1 = np.where(fy >= np.float32(0.5), fx >= one - fy, fy >= one - fx)   # fx + fy >= 1, exactly
    prim = 2 * (cy * (W - 1) + cx) + tri1.astype(np.int64)
    b1 = np.where(tri1, one - fx, fx).astype(np.float32)
    b2 = np.where(tri1, one - fy, fy).astype(np.float32)
    z = np.float32(0)
    return valid, np.where(valid, prim, 0), np.where(valid, b1, z), np.where(valid, b2, z)


def texcoord_triangles(W, H):
    """[M, 3, 2] float64 texcoords of the triangles in prim_index order"""
    F = S.grid_faces(W, H).numpy()
    return np.stack([(F % W) / (W - 1.0), (F // W) / (H - 1.0)], -1)


def brute_force(u, v, W, H):
    """Mesh's lookup: Moeller-Trumbore (mesh.h:357-380, inclusive tests) in float64 of the ray o = (u, v, -1),
    d = (0, 0, 1) against every texcoord triangle; the highest prim_index among the hits, -1 for none.  Also returns
    the per-query candidate count."""
    T = texcoord_triangles(W, H)
    u = np.asarray(u, np.float64).reshape(-1, 1)
    v = np.asarray(v, np.float64).reshape(-1, 1)
    p0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    # d = (0, 0, 1): pvec = d x e2 = (-e2.y, e2.x, 0), qvec = tvec x e1 with tvec = (u - p0, v - p0, -1)
    det = e1[:, 0] * -e2[:, 1] + e1[:, 1] * e2[:, 0]
    tx, ty = u - p0[:, 0], v - p0[:, 1]
    a = (tx * -e2[:, 1] + ty * e2[:, 0]) / det
    q_z = tx * e1[:, 1] - ty * e1[:, 0]                                     # d . qvec
    b = q_z / det
    hit = (a >= 0) & (a <= 1) & (b >= 0) & (a + b <= 1)
    idx = np.where(hit, np.arange(T.shape[0])[None, :], -1).max(1)
    return idx, hit.sum(1)


def uv_rays(u, v):
    """o, d [n, 3] float64 of the UV-space rays"""
    u = torch.as_tensor(u, dtype=torch.float64)
    v = torch.as_tensor(v, dtype=torch.float64)
    o = torch.stack([u, v, -torch.ones_like(u)], -1)
    d = torch.zeros_like(o)
    d[:, 2] = 1.0
    return o, d


def record(h, s, tw, flip, u, v, prim, b1, b2, flags=RAY_ALL, smooth=False):
    """the record (dict of smooth_ref.surface: t, p, n, sh_n, uv, dp_du, dp_dv, sh_s, sh_t, wi) at the frozen (prim, b)
    of the queries u, v: FollowShape on the UV-space ray with t = 1.  h [H, W], tw 3x4 may carry derivatives."""
    o, d = uv_rays(u, v)
    o, d = o.to(h.device), d.to(h.device)
    b = (torch.as_tensor(np.asarray(b1, np.float64), device=h.device), torch.as_tensor(np.asarray(b2, np.float64), device=h.device))
    prim = torch.as_tensor(np.asarray(prim, np.int64), device=h.device)
    tw = torch.as_tensor(tw, dtype=torch.float64, device=h.device).reshape(3, 4) if not isinstance(tw, torch.Tensor) else tw
    r = S.surface(h, s, tw, flip, o, d, prim, b, "follow", flags, smooth)
    r["t"] = torch.ones_like(r["t"]).detach()
    return r


def block(r):
    """[18, n] rows t, p, n, uv, sh_n, dp_du, dp_dv of a record"""
    return torch.cat([r["t"][None], r["p"].T, r["n"].T, r["uv"].T, r["sh_n"].T, r["dp_du"].T, r["dp_dv"].T])

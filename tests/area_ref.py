"""Float64 torch restatement of the heightfield's area sampling, the yardstick of tests/test_area_sampling_abi.py and
tests/test_gpu_area_sampling.py.

  * areas: Mesh::build_pmf (src/render/mesh.cpp:401-432): .5 norm(cross(p1 - p0, p2 - p0)) per triangle in prim_index
    order, on the world-space vertices of smooth_ref.world_vertices and the faces of smooth_ref.grid_faces;
  * cdf: DiscreteDistribution::compute_cdf (include/mitsuba/core/distr_1d.h:212-240): a sequential double running sum,
    each prefix rounded to float32; sum, normalization and the valid range;
  * sample_index: sample_reuse (distr_1d.h:120-130, 167-176) given a CDF: the first i in [valid.x, valid.y] with
    !(cdf[i] < y sum) -- dr::binary_search -- and the reused sample;
  * warp: square_to_uniform_triangle (include/mitsuba/core/warp.h:153-156);
  * position: p, n, uv of Mesh::sample_position (mesh.cpp:557-610) for a frozen (prim, b), differentiable in the heights
    (flat: the face normal; smooth: the blend of the vertex normals of smooth_ref.vertex_normals_grid);
  * direction / pdf_direction: Shape::sample_direction / pdf_direction (src/render/shape.cpp:363-395).
"""
import numpy as np
import torch

import smooth_ref as S


def _r32(x):
    return x.float().double()


def world_vertices_f32(h, s, tw):
    """[H, W, 3] world-space vertices as the device rounds them (float64 tensor of float32 values): object x =
    fma(j, (float) 2/(W-1), -1), y likewise, z = h * s in float32, then the fma chain of the 3x4 affine
    (m3 + m0 x, + m1 y, + m2 z), each step rounded to float32.  The areas of a field whose cells are small against its
    distance from the origin depend on these roundings (the edge vectors cancel), so the table is compared with areas
    of these vertices."""
    H, W = h.shape
    dt, dev = torch.float64, h.device
    sx = _r32(torch.tensor(2.0 / (W - 1), dtype=dt, device=dev))
    sy = _r32(torch.tensor(2.0 / (H - 1), dtype=dt, device=dev))
    x = _r32(torch.arange(W, dtype=dt, device=dev) * sx - 1.0)[None, :].expand(H, W)
    y = _r32(torch.arange(H, dtype=dt, device=dev) * sy - 1.0)[:, None].expand(H, W)
    z = _r32(_r32(h) * _r32(torch.tensor(float(s), dtype=dt, device=dev)))
    m = _r32(torch.as_tensor(np.asarray(tw, np.float64).reshape(3, 4), dtype=dt, device=dev))
    out = []
    for r in range(3):
        acc = _r32(m[r, 3] + m[r, 0] * x)
        acc = _r32(acc + m[r, 1] * y)
        out.append(_r32(acc + m[r, 2] * z))
    return torch.stack(out, -1)


def areas(h, s, tw, device_rounding=False):
    """[M] world-space triangle areas (float64) of heights h [H, W]; device_rounding: of world_vertices_f32"""
    H, W = h.shape
    V = (world_vertices_f32(h, s, tw) if device_rounding else S.world_vertices(h, s, tw)).reshape(-1, 3)
    F = S.grid_faces(W, H).to(V.device)
    c = torch.linalg.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]], dim=-1)
    return 0.5 * torch.linalg.norm(c, dim=-1)


def cdf(pmf):
    """compute_cdf of the float32 table pmf (numpy): (cdf float32, sum float64, sum float32, normalization float32,
    (valid.x, valid.y))"""
    pmf = np.asarray(pmf, np.float32).astype(np.float64)
    run = np.cumsum(pmf)   # sequential
    nz = np.nonzero(pmf > 0)[0]
    total = float(run[-1])
    return run.astype(np.float32), total, np.float32(total), np.float32(1.0 / total), (int(nz[0]), int(nz[-1]))


def sample_index(cdf32, sum32, valid, y):
    """dr::binary_search over [valid.x, valid.y] of !(cdf[i] < y * sum) (float32 product)"""
    target = (np.asarray(y, np.float32) * np.float32(sum32)).astype(np.float32)
    idx = np.searchsorted(cdf32, target, side="left")
    return np.clip(idx, valid[0], valid[1])


def reuse(cdf32, pmf32, norm32, idx, y):
    """(y - cdf[i-1] norm) / (pmf[i] norm) in float32"""
    y = np.asarray(y, np.float32)
    prev = np.where(idx > 0, cdf32[np.maximum(idx - 1, 0)], np.float32(0)).astype(np.float32)
    return ((y - prev * norm32) / (pmf32[idx] * norm32)).astype(np.float32)


def warp(x, y):
    """square_to_uniform_triangle: t = safe_sqrt(1 - x), b = (1 - t, t y)"""
    t = np.sqrt(np.maximum(1.0 - np.asarray(x, np.float64), 0.0))
    return 1.0 - t, t * np.asarray(y, np.float64)


def position(h, s, tw, flip, prim, bx, by, smooth, device_rounding=False):
    """p, n [n, 3] and uv [n, 2] (float64) of the samples (prim, b) -- differentiable in h; device_rounding: on the
    vertices of world_vertices_f32 (the face normal of a small cell depends on their rounding)"""
    H, W = h.shape
    P = world_vertices_f32(h, s, tw) if device_rounding else S.world_vertices(h, s, tw)
    V = P.reshape(-1, 3)
    f = S.grid_faces(W, H).to(V.device)[prim]
    p0, p1, p2 = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    e0, e1 = p1 - p0, p2 - p0
    bx, by = bx[:, None], by[:, None]
    b0 = 1.0 - bx - by
    p = p0 + e0 * bx + e1 * by
    if smooth:
        N = S.vertex_normals_grid(P).reshape(-1, 3)
        n = N[f[:, 0]] * b0 + N[f[:, 1]] * bx + N[f[:, 2]] * by
    else:
        n = torch.linalg.cross(e0, e1, dim=-1)
    n = n / torch.linalg.norm(n, dim=-1, keepdim=True)
    if flip:
        n = -n
    U = (f % W).to(V.dtype) / (W - 1)
    Vt = (f // W).to(V.dtype) / (H - 1)
    w = torch.cat([b0, bx, by], -1)
    uv = torch.stack([(U * w).sum(-1), (Vt * w).sum(-1)], -1)
    return p, n, uv


def direction(ref_p, p, n, pdf_pos):
    """sample_direction's d, dist, pdf for reference points ref_p [n, 3]"""
    d = p - ref_p
    dist2 = (d * d).sum(-1)
    dist = torch.sqrt(dist2)
    d = d / dist[:, None]
    dp = (d * n).sum(-1).abs()
    x = dist2 / dp
    return d, dist, pdf_pos * torch.where(torch.isfinite(x), x, torch.zeros_like(x))


def pdf_direction(d, n, dist, pdf_pos):
    dp = (d * n).sum(-1).abs()
    return pdf_pos * torch.where(dp != 0, dist * dist / dp, torch.zeros_like(dp))

"""Float64 torch restatement of smooth shading (face_normals = false), the yardstick of tests/test_smooth_abi.py and
tests/test_gpu_smooth_shading.py.

  * vertex_normals_faces: the JIT path of Mesh::recompute_vertex_normals (src/render/mesh.cpp:350-384) over an explicit
    face list: per face n = normalize(cross(v1 - v0, v2 - v0)), per corner i the angle
    safe_acos(dot(normalize(v[i+1] - v[i]), normalize(v[i+2] - v[i]))), scatter-add of n * angle, normalize;
  * vertex_normals_grid: the heightfield's enumeration of the same sum (the 1-ring of each texel, as vertex_normal in
    hf_device.h);
  * surface: the record of hits in the three AD modes (default: Moeller-Trumbore with attached vertices; follow:
    frozen barycentrics, t = |p - o| / |d|; detach: no dependence on the heights) under any RayFlags set,
    differentiable in the heights, the rays and to_world.
Everything is plain torch, so autograd / torch.func.jvp give the reverse and forward derivatives.
"""
import torch

from si_numpy import RAY_ALL, RAY_DPDUV, RAY_DNSDUV, RAY_SHADINGFRAME, RAY_UV, coordinate_system

RING = ((0, 1), (1, 0), (1, -1), (0, -1), (-1, 0), (-1, 1))  # E, N, NW, W, S, SE as (row, column) offsets


def _normalize(v):
    return v / torch.linalg.norm(v, dim=-1, keepdim=True)


def world_vertices(h, s, tw):
    """[H, W, 3] world-space vertices of heights h ([H, W] float64): object x = -1 + 2 j / (W - 1), y = -1 + 2 i / (H - 1),
    z = s h, then the 3x4 affine tw"""
    H, W = h.shape
    x = -1.0 + torch.arange(W, dtype=h.dtype, device=h.device) * (2.0 / (W - 1))
    y = -1.0 + torch.arange(H, dtype=h.dtype, device=h.device) * (2.0 / (H - 1))
    q = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), h * s], -1)
    A = torch.as_tensor(tw, dtype=h.dtype, device=h.device).reshape(3, 4)
    return q @ A[:, :3].T + A[:, 3]


def grid_faces(W, H):
    """[2 (W-1)(H-1), 3] vertex ids (i W + j) in prim_index order: tri 0 = (v00, v10, v01), tri 1 = (v11, v01, v10)"""
    cy, cx = torch.meshgrid(torch.arange(H - 1), torch.arange(W - 1), indexing="ij")
    v00 = (cy * W + cx).reshape(-1)
    v10, v01 = v00 + 1, v00 + W
    v11 = v01 + 1
    return torch.stack([torch.stack([v00, v10, v01], 1), torch.stack([v11, v01, v10], 1)], 1).reshape(-1, 3)


def vertex_normals_faces(V, F):
    """mesh.cpp:350-384 for vertices V [N, 3] and faces F [M, 3]"""
    v = [V[F[:, k]] for k in range(3)]
    n = _normalize(torch.linalg.cross(v[1] - v[0], v[2] - v[0], dim=-1))
    acc = torch.zeros_like(V)
    for i in range(3):
        d0 = _normalize(v[(i + 1) % 3] - v[i])
        d1 = _normalize(v[(i + 2) % 3] - v[i])
        ang = torch.acos(torch.clamp((d0 * d1).sum(-1), -1.0, 1.0))
        acc = acc.index_add(0, F[:, i], n * ang[:, None])
    return _normalize(acc)


def vertex_normals_grid(P):
    """the same normals from the 1-ring of every texel of P [H, W, 3] (triangles (X, R_k, R_k+1) whose two ring
    vertices exist)"""
    H, W, _ = P.shape
    I = torch.arange(H, device=P.device)[:, None].expand(H, W)
    J = torch.arange(W, device=P.device)[None, :].expand(H, W)
    R, ok = [], []
    for di, dj in RING:
        ii, jj = I + di, J + dj
        m = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
        r = P[ii.clamp(0, H - 1), jj.clamp(0, W - 1)]
        # absent neighbours: a harmless stand-in (masked out below; keeps NaN out of the backward pass)
        r = torch.where(m[..., None], r, P + torch.tensor([float(dj), float(di), 0.5], dtype=P.dtype, device=P.device))
        R.append(r); ok.append(m)
    acc = torch.zeros_like(P)
    for k in range(6):
        k1 = (k + 1) % 6
        e1, e2 = R[k] - P, R[k1] - P
        nt = _normalize(torch.linalg.cross(e1, e2, dim=-1))
        ang = torch.acos(torch.clamp((_normalize(e1) * _normalize(e2)).sum(-1), -1.0, 1.0))
        acc = acc + torch.where((ok[k] & ok[k1])[..., None], nt * ang[..., None], torch.zeros_like(nt))
    return _normalize(acc)


def surface(h, s, tw, flip, o, d, prim, b_frozen, mode, flags=RAY_ALL, smooth=True):
    """t [n], p / n / sh_n / dp_du / dp_dv / sh_s / sh_t / wi [n, 3], uv [n, 2] (float64) of hits (prim [n]; o, d [n, 3]);
    b_frozen = (b1, b2) [n] each, used by mode 'follow'; 'default' re-intersects with attached vertices; 'detach'
    detaches the heights.  `flags` (RayFlags bits) chooses the record as mesh.cpp:672-903 and interaction.h:257-267,
    475-507 do:
      * uv: the texcoords with UV or dPdUV, else the barycentrics (b1, b2);
      * dp_du, dp_dv: from the texcoords with dPdUV, else coordinate_system of the face normal before flip_normals
        (mesh.cpp:762), attached;
      * sh_n: the blended vertex normal (smooth) with ShadingFrame or dNSdUV, else the face normal;
      * sh_s, sh_t: Gram-Schmidt on dp_du with ShadingFrame (coordinate_system(sh_n) where dp_du = 0), else zero;
        wi = to_local(-d) in that frame.
    tw may be a float64 tensor that carries a derivative."""
    H, W = h.shape
    P = world_vertices(h, s, tw)
    if mode == "detach":
        P = P.detach()
    V = P.reshape(-1, 3)
    f = grid_faces(W, H).to(P.device)[prim]
    P0, P1, P2 = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    e1, e2 = P1 - P0, P2 - P0
    if mode == "follow":
        b1, b2 = b_frozen
    else:  # mesh.h:357-380
        pvec = torch.linalg.cross(d, e2, dim=-1)
        inv = 1.0 / (e1 * pvec).sum(-1)
        tvec = o - P0
        qvec = torch.linalg.cross(tvec, e1, dim=-1)
        b1 = (tvec * pvec).sum(-1) * inv
        b2 = (d * qvec).sum(-1) * inv
        t = (e2 * qvec).sum(-1) * inv
    b0 = 1.0 - b1 - b2
    p = b0[:, None] * P0 + b1[:, None] * P1 + b2[:, None] * P2
    if mode == "follow":
        t = torch.sqrt(((p - o) ** 2).sum(-1) / (d * d).sum(-1))
    sgn = -1.0 if flip else 1.0
    n0 = _normalize(torch.linalg.cross(e1, e2, dim=-1))
    n = sgn * n0
    out = {"t": t, "p": p, "n": n, "b": (b0, b1, b2)}
    if smooth:
        Nv = vertex_normals_grid(P).reshape(-1, 3)
        out["N"] = Nv[f]
    if smooth and flags & (RAY_SHADINGFRAME | RAY_DNSDUV):
        out["sh_n"] = sgn * _normalize(b0[:, None] * Nv[f[:, 0]] + b1[:, None] * Nv[f[:, 1]] + b2[:, None] * Nv[f[:, 2]])
    else:
        out["sh_n"] = n
    # the texcoords (j / (W - 1), i / (H - 1)) (mesh.cpp:764-789)
    U = (f % W).to(P.dtype) / (W - 1)
    Vt = (f // W).to(P.dtype) / (H - 1)
    if flags & (RAY_UV | RAY_DPDUV):
        out["uv"] = torch.stack([b0 * U[:, 0] + b1 * U[:, 1] + b2 * U[:, 2], b0 * Vt[:, 0] + b1 * Vt[:, 1] + b2 * Vt[:, 2]], -1)
    else:
        out["uv"] = torch.stack([b1, b2], -1)
    if flags & RAY_DPDUV:
        du0, dv0 = U[:, 1] - U[:, 0], Vt[:, 1] - Vt[:, 0]
        du1, dv1 = U[:, 2] - U[:, 0], Vt[:, 2] - Vt[:, 0]
        det = du0 * dv1 - dv0 * du1
        out["dp_du"] = (dv1[:, None] * e1 - dv0[:, None] * e2) / det[:, None]
        out["dp_dv"] = (-du1[:, None] * e1 + du0[:, None] * e2) / det[:, None]
    else:
        out["dp_du"], out["dp_dv"] = coordinate_system(n0)
    if flags & RAY_SHADINGFRAME:
        out["sh_s"], out["sh_t"], out["wi"] = shading_frame(out["sh_n"], out["dp_du"], d)
    else:
        z = torch.zeros_like(p)
        out["sh_s"], out["sh_t"] = z, z
        out["wi"] = torch.stack([z[:, 0], z[:, 0], -(d * out["sh_n"]).sum(-1)], -1)
    return out


def shading_frame(sh_n, dp_du, d):
    """sh_s, sh_t, wi of finalize_surface_interaction (interaction.h:257-267, 476-499) on the shading normal"""
    s = _normalize(dp_du - sh_n * (sh_n * dp_du).sum(-1, keepdim=True))
    zero = (dp_du == 0).all(-1, keepdim=True)     # dp_du = 0: coordinate_system(sh_n).s
    if bool(zero.any()):
        s = torch.where(zero, coordinate_system(sh_n)[0], s)
    t = torch.linalg.cross(sh_n, s, dim=-1)
    md = -d
    wi = torch.stack([(md * s).sum(-1), (md * t).sum(-1), (md * sh_n).sum(-1)], -1)
    return s, t, wi


def shading_derivatives(Nk, b1, b2):
    """dn_du, dn_dv of mesh.cpp:818-829 for the hits' vertex normals Nk [n, 3, 3] (before flip_normals)"""
    b0 = 1.0 - b1 - b2
    ns = b0[:, None] * Nk[:, 0] + b1[:, None] * Nk[:, 1] + b2[:, None] * Nk[:, 2]
    il = 1.0 / torch.linalg.norm(ns, dim=-1, keepdim=True)
    n = ns * il
    du, dv = (Nk[:, 1] - Nk[:, 0]) * il, (Nk[:, 2] - Nk[:, 0]) * il
    return du - n * (n * du).sum(-1, keepdim=True), dv - n * (n * dv).sum(-1, keepdim=True)

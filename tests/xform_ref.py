"""Float64 torch restatement of the surface interaction and of sample_position as functions of to_world, the
yardstick of tests/test_transform_grad_abi.py and tests/test_gpu_transform_grad.py.

Built on tests/smooth_ref.py (world vertices, the grid's vertex normals, prim_index order) and laid out as the kernels'
18-row differentiable block (t, p, n, uv, sh_n, dp_du, dp_dv) under any RayFlags set (smooth_ref.surface):
  * default: Moeller-Trumbore re-intersection with attached vertices (p stays on the ray);
  * follow : frozen barycentrics, t = |p - o| / |d| (p glued to the shape);
  * detach : the vertices carry no derivative.
The triangle (prim) is always held fixed, as in the kernels.  fd_to_world differentiates any scalar function of the
3x4 to_world by central differences.
"""
import numpy as np
import torch

import smooth_ref as S

ROWS = {"t": (0, 1), "p": (1, 4), "n": (4, 7), "uv": (7, 9), "sh_n": (9, 12), "dp_du": (12, 15), "dp_dv": (15, 18)}


def si_block(h, s, tw, flip, o, d, prim, b_frozen, mode, smooth, tw_frozen=None, flags=S.RAY_ALL, frame=False):
    """[18, n] float64 block of the hits (prim [n] int64; o, d [n, 3]; b_frozen = (b1, b2) [n] each, for 'follow').
    'detach' evaluates the geometry on tw_frozen (when given) and detaches it: nothing depends on tw.  `flags`: the
    RayFlags set of smooth_ref.surface; frame: the 9 rows sh_s, sh_t, wi follow (a [27, n] block)"""
    if mode == "detach" and tw_frozen is not None:
        tw = tw_frozen
    tw = torch.as_tensor(tw, dtype=torch.float64).reshape(3, 4)
    r = S.surface(h, s, tw, flip, o, d, prim, b_frozen, mode, flags, smooth)
    names = ("t", "p", "n", "uv", "sh_n", "dp_du", "dp_dv") + (("sh_s", "sh_t", "wi") if frame else ())
    return torch.cat([r[k][None] if k == "t" else r[k].T for k in names])


def sample_block(h, s, tw, flip, prim, bx, by, smooth):
    """[6, n] float64 block (p, n) of sample_position for the samples (prim, b)"""
    H, W = h.shape
    tw = torch.as_tensor(tw, dtype=torch.float64).reshape(3, 4)
    P = S.world_vertices(h, s, tw)
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
    n = S._normalize(n)
    if flip:
        n = -n
    return torch.cat([p.T, n.T])


def fd_to_world(fn, tw, eps=1e-6):
    """[3, 4] central differences of the scalar fn(tw) (tw: 3x4 float64 array)"""
    tw = np.asarray(tw, np.float64).reshape(3, 4)
    g = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            a = tw.copy(); a[r, c] += eps
            b = tw.copy(); b[r, c] -= eps
            g[r, c] = (float(fn(torch.from_numpy(a))) - float(fn(torch.from_numpy(b)))) / (2 * eps)
    return g


# ---- the reference's test08 (src/shapes/tests/test_rectangle.py:176-272): a flat grid is the rectangle ----------

def scale(x, y, z):
    return np.diag([x, y, z, 1.0])[:3]


def translate(x, y, z):
    m = np.eye(4)[:3].copy()
    m[:, 3] = (x, y, z)
    return m


def rotate_z(deg):
    a = np.deg2rad(deg)
    m = np.eye(4)[:3].copy()
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return m


# (name, mode, to_world(theta), ray origin (x, y), expected derivatives d/dtheta at theta = 0 of t, p, n, uv)
TEST08 = [
    ("scale_default", "default", lambda th: scale(1 + th, 1 + 2 * th, 1), (0.1, 0.2),
     {"t": [0.0], "p": [0, 0, 0], "n": [0, 0, 0], "uv": [-0.05, -0.2]}),
    ("translate_follow", "follow", lambda th: translate(th, 0, 0), (0.1, 0.2),
     {"p": [1, 0, 0], "n": [0, 0, 0], "uv": [0, 0]}),
    ("rotate_follow", "follow", lambda th: rotate_z(90 * th), (0.1, 0.1),
     {"p": [-np.pi * 0.1 / 2, np.pi * 0.1 / 2, 0], "n": [0, 0, 0], "uv": [0, 0]}),
    ("rotate_default", "default", lambda th: rotate_z(90 * th), (0.1, 0.1),
     {"p": [0, 0, 0], "n": [0, 0, 0], "uv": [np.pi * 0.1 / 4, -np.pi * 0.1 / 4]}),
    ("rotate_detach", "detach", lambda th: rotate_z(90 * th), (0.1, 0.1),
     {"t": [0.0], "p": [0, 0, 0], "n": [0, 0, 0], "uv": [0, 0]}),
]


def test08_ray(xy):
    return np.array([xy[0], xy[1], -2.0]), np.array([0.0, 0.0, 1.0])


def test08_prim(W, H, x, y):
    """the triangle of the flat grid (object space = world space at theta = 0) under (x, y), and its barycentrics"""
    fx, fy = (x + 1.0) * 0.5 * (W - 1), (y + 1.0) * 0.5 * (H - 1)
    cx, cy = int(np.floor(fx)), int(np.floor(fy))
    ax, ay = fx - cx, fy - cy
    cell = cy * (W - 1) + cx
    if ax + ay <= 1.0:   # tri 0 = (v00, v10, v01)
        return 2 * cell, (ax, ay)
    return 2 * cell + 1, (1.0 - ax, 1.0 - ay)   # tri 1 = (v11, v01, v10)

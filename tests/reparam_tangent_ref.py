"""Float64 restatement of hf_reparam_tangent (reparam.py:155-221 for a scene that is one heightfield), for tangents of
the heights, the ray origin, the ray direction and to_world.  The samples, the detached weights and the hit triangles
with their barycentrics come from the oracle (the same ones oracle.reparam_forward uses); everything differentiated is
evaluated here in float64.  `vdirect_sums` is the function whose directional derivative the tangent is, so that the
tests can check the analytic tangent against central differences of it."""
import numpy as np


def coordinate_system(n):
    """include/mitsuba/core/vector.h:116-136 on [3, k] float64 arrays"""
    sign = np.where(n[2] >= 0, 1.0, -1.0)
    a = -1.0 / (sign + n[2]); b = n[0] * n[1] * a
    s = np.stack([sign * n[0] * n[0] * a + 1.0, sign * b, -sign * n[0]])
    t = np.stack([b, n[1] * n[1] * a + sign, -n[1]])
    return s, t


def coordinate_system_jvp(n, dn):
    """its tangent with the sign held (the transpose of what torch autograd does over shape._coordinate_system)"""
    sign = np.where(n[2] >= 0, 1.0, -1.0)
    a = -1.0 / (sign + n[2]); da = a * a * dn[2]
    db = (dn[0] * n[1] + n[0] * dn[1]) * a + n[0] * n[1] * da
    ds = np.stack([sign * (2 * n[0] * dn[0] * a + n[0] * n[0] * da), sign * db, -sign * dn[0]])
    dt = np.stack([db, 2 * n[1] * dn[1] * a + n[1] * n[1] * da, -dn[1]])
    return ds, dt


def tri_vertices(W, prim):
    """(rows vi, columns vj) [3, n] of the primitives' vertices (prim_vertex_ids)"""
    prim = np.asarray(prim).astype(np.int64)
    cell, tri = prim >> 1, prim & 1
    cy, cx = cell // (W - 1), cell % (W - 1)
    vi = np.where(tri == 0, np.stack([cy, cy, cy + 1]), np.stack([cy + 1, cy + 1, cy]))
    vj = np.where(tri == 0, np.stack([cx, cx + 1, cx]), np.stack([cx + 1, cx, cx + 1]))
    return vi, vj


def samples(oracle, field, o, d, num_rays, kappa, exponent, antithetic=False, seed=0, active=None):
    """per sample k: (omega [3,n], hit [n], w [n], dw [3,n], vi, vj [3,n], bary [3,n]) as the kernels draw them"""
    o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
    n = o.shape[1]
    act = np.ones(n, bool) if active is None else (np.asarray(active) != 0)
    out = []
    for k in range(num_rays):
        r = oracle.reparam_aux_rays(o, d, k, kappa, antithetic, seed, active)
        t, u, v, prim = field.ray_intersect_preliminary(r)
        si = field.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL | 0x80 | 0x40)  # FollowShape, BoundaryTest
        hit, w, dw = oracle._reparam_weight(d, k, kappa, exponent, antithetic, seed, si["t"].astype(np.float64),
                                            si["boundary_test"].astype(np.float64))
        om = oracle.reparam_aux_sample(d, k, kappa, antithetic, seed)[0]
        vi, vj = tri_vertices(field.W, np.where(hit, prim, 0))
        b1, b2 = u.astype(np.float64), v.astype(np.float64)
        out.append((om, hit & act, np.where(act, w, 0.0), np.where(act, dw, 0.0), vi, vj, np.stack([1 - b1 - b2, b1, b2])))
    return out, act


def _local(field, h, vi, vj):
    """object-space vertex positions q [3 vertices][3, n] for heights h"""
    W, H = field.W, field.H
    x = vj * (2.0 / (W - 1)) - 1.0
    y = vi * (2.0 / (H - 1)) - 1.0
    z = field.max_height * h[vi, vj]
    return [np.stack([x[j], y[j], z[j]]) for j in range(3)]


def vdirect_sums(field, S, o, d, M, h):
    """(sum_k w_k V_direct_k [3,n], sum_k <dw_k, V_direct_k> [n]) with samples, weights and triangles held fixed"""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    M = np.asarray(M, np.float64).reshape(3, 4); h = np.asarray(h, np.float64)
    fs, ft = coordinate_system(d)
    gV = np.zeros_like(o); gdiv = np.zeros(o.shape[1])
    for om, hit, w, dw, vi, vj, bw in S:
        q = _local(field, h, vi, vj)
        p = sum(bw[j] * (M[:, :3] @ q[j] + M[:, 3:4]) for j in range(3))
        da = fs * om[0] + ft * om[1] + d * om[2]
        po = p - o
        t = np.sqrt((po * po).sum(0) / (da * da).sum(0))
        V = np.where(hit, po / np.where(hit, t, 1.0), d)
        gV += w * V; gdiv += (dw * V).sum(0)
    return gV, gdiv


def reparam_tangent(field, S, act, o, d, M, h, dh=None, do=None, dd=None, dM=None):
    """(V_theta [3,n], div [n]) of hf_reparam_tangent, float64, and the two numerators (sum w dV, sum <dw, dV>)"""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    M = np.asarray(M, np.float64).reshape(3, 4); h = np.asarray(h, np.float64)
    n = o.shape[1]
    z = np.zeros((3, n))
    dh = np.zeros_like(h) if dh is None else np.asarray(dh, np.float64)
    do = z if do is None else np.asarray(do, np.float64)
    dd = z if dd is None else np.asarray(dd, np.float64)
    dM = np.zeros((3, 4)) if dM is None else np.asarray(dM, np.float64).reshape(3, 4)
    fs, ft = coordinate_system(d)
    dfs, dft = coordinate_system_jvp(d, dd)
    ez = M[:, 2:3] * field.max_height
    Z = np.zeros(n); dZ = np.zeros((3, n)); gV = np.zeros((3, n)); gdiv = np.zeros(n)
    for om, hit, w, dw, vi, vj, bw in S:
        q = _local(field, h, vi, vj)
        p = sum(bw[j] * (M[:, :3] @ q[j] + M[:, 3:4]) for j in range(3))
        dp = sum(bw[j] * (ez * dh[vi[j], vj[j]] + dM[:, :3] @ q[j] + dM[:, 3:4]) for j in range(3))
        da = fs * om[0] + ft * om[1] + d * om[2]
        dda = dfs * om[0] + dft * om[1] + dd * om[2]
        po = p - o
        n2 = (da * da).sum(0)
        t = np.where(hit, np.sqrt((po * po).sum(0) / n2), 1.0)
        dt = (po * (dp - do)).sum(0) / (t * n2) - t * (da * dda).sum(0) / n2
        dV = np.where(hit, (dp - do) / t - po * dt / (t * t), dd)
        Z += w; dZ += dw
        gV += w * dV; gdiv += (dw * dV).sum(0)
    iZ = 1.0 / np.maximum(Z, 1e-8)
    Vt = gV * iZ
    div = (gdiv - (Vt * dZ).sum(0)) * iZ
    return np.where(act, Vt, 0.0), np.where(act, div, 0.0), gV, gdiv

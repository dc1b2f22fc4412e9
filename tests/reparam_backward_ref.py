"""Float64 restatement of hf_reparam_backward_full (reparam.py:224-333 for a scene that is one heightfield): the
transpose of reparam_tangent_ref.reparam_tangent, from the same sample records (reparam_tangent_ref.samples).  For
upstream gradients (g_dir, g_div) of (direction, det) it returns the gradients of the heights, ray.o, ray.d and
to_world, with the weights detached.  The direction's gradient goes through normalize(d + V_theta) at V_theta = 0
(reparam.py:262-281), i.e. through P = (I - d d^T / |d|^2) / |d|."""
import numpy as np

import reparam_tangent_ref as R


def coordinate_system_vjp(n, gs, gt):
    """the transpose of reparam_tangent_ref.coordinate_system_jvp: dL/dn for gs = dL/ds, gt = dL/dt (sign held)"""
    sign = np.where(n[2] >= 0, 1.0, -1.0)
    a = -1.0 / (sign + n[2])
    gb = sign * gs[1] + gt[0]
    ga = sign * n[0] * n[0] * gs[0] + n[1] * n[1] * gt[1] + n[0] * n[1] * gb
    return np.stack([2 * sign * n[0] * a * gs[0] + n[1] * a * gb - sign * gs[2],
                     n[0] * a * gb + 2 * n[1] * a * gt[1] - gt[2],
                     a * a * ga])


def project(d, V):
    """P V: the tangent of normalize(d + V) at V = 0"""
    d = np.asarray(d, np.float64)
    n2 = (d * d).sum(0)
    return (V - d * ((d * V).sum(0) / n2)) / np.sqrt(n2)


def reparam_backward(field, S, act, o, d, M, h, g_dir, g_div):
    """(grad_h [H, W], grad_o [3, n], grad_d [3, n], grad_M [3, 4]), float64"""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    M = np.asarray(M, np.float64).reshape(3, 4); h = np.asarray(h, np.float64)
    g_dir = np.asarray(g_dir, np.float64); g_div = np.asarray(g_div, np.float64)
    n = o.shape[1]
    fs, ft = R.coordinate_system(d)
    Z = sum(s[2] for s in S); dZ = sum(s[3] for s in S)
    iZ = 1.0 / np.maximum(Z, 1e-8)
    gV = project(d, g_dir) * iZ - g_div * iZ * iZ * dZ          # dL/d(sum_k w_k V_direct_k)
    gdivV = g_div * iZ                                           # dL/d(sum_k <dw_k, V_direct_k>)
    ez = M[:, 2:3] * field.max_height
    grad_h = np.zeros_like(h); grad_o = np.zeros((3, n)); grad_d = np.zeros((3, n)); grad_M = np.zeros((3, 4))
    gfs = np.zeros((3, n)); gft = np.zeros((3, n))
    for om, hit, w, dw, vi, vj, bw in S:
        gVd = np.where(act, w * gV + gdivV * dw, 0.0)
        q = R._local(field, h, vi, vj)
        p = sum(bw[j] * (M[:, :3] @ q[j] + M[:, 3:4]) for j in range(3))
        da = fs * om[0] + ft * om[1] + d * om[2]
        po = p - o
        n2 = (da * da).sum(0)
        t = np.where(hit, np.sqrt((po * po).sum(0) / n2), 1.0)
        gt = -(gVd * po).sum(0) / (t * t)
        gpo = np.where(hit, gVd / t + gt * po / (t * n2), 0.0)   # gradient of p - o, t's dependence on it included
        gda = np.where(hit, -gt * t * da / n2, 0.0)              # gradient of d_aux
        grad_o -= gpo
        gfs += gda * om[0]; gft += gda * om[1]
        grad_d += gda * om[2] + np.where(~hit & act, gVd, 0.0)   # miss: V_direct = ray.d
        for j in range(3):
            gP = np.where(hit, bw[j] * gpo, 0.0)
            np.add.at(grad_h, (vi[j], vj[j]), (ez * gP).sum(0))
            grad_M[:, :3] += gP @ q[j].T
            grad_M[:, 3] += gP.sum(1)
    grad_d += coordinate_system_vjp(d, gfs, gft)
    return grad_h, grad_o, grad_d, grad_M

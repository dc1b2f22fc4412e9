"""Float64 restatement of the bounce-lighting row of include/hf.h (hf_bounce_rays, hf_bounce_lighting, _adjoint,
_tangent): the sample stream, the cosine-weighted directions and their frame, the masks, the spawned origins, the
value, its adjoint and its tangent, and the face normal of a grid triangle (rectangular grids, any constant affine
to_world) with its VJP and JVP.  The record (which
bounce rays hit, which lights reach the hit) and the normals n_q of the hits are inputs: nothing here traces.  Uses the
oracle's sample_tea_32 (through tests/sky_ref.py, which restates the shared stream) and nothing of the product.

Shapes: n samples, K directions, L lights.  hit [K, n] bool, lit [K, L, n] bool, n_q [K, 3, n], lights [L, 4] (unit
direction towards the light, irradiance)."""
import numpy as np

from reparam_tangent_ref import coordinate_system  # noqa: F401  ((s, t) of vector.h:116-136 for [3, n] float64 normals)
from sky_ref import RAY_EPSILON, eligible, samples, spawn_origin, tea32  # noqa: F401  (the stream and the masks are the sky row's)

MISS = 0xFFFFFFFF


def local_directions(ids, K, seed):
    """[K, 3, n]: square_to_cosine_hemisphere (warp.h:54-90, 320-328) of every sample's K draws, local frame"""
    out = np.empty((K, 3, len(ids)))
    for k in range(K):
        sx, sy = samples(ids, k, seed)
        x, y = 2.0 * sx - 1.0, 2.0 * sy - 1.0
        q13 = np.abs(x) < np.abs(y)
        r, rp = np.where(q13, y, x), np.where(q13, x, y)
        with np.errstate(invalid="ignore", divide="ignore"):
            phi = 0.25 * np.pi * rp / r
        phi = np.where(q13, 0.5 * np.pi - phi, phi)
        phi = np.where((x == 0) & (y == 0), 0.0, phi)
        px, py = r * np.cos(phi), r * np.sin(phi)
        out[k] = np.stack([px, py, np.sqrt(np.maximum(0.0, 1.0 - px * px - py * py))])
    return out


def directions(sh_n, ids, K, seed):
    """(w [K, 3, n] world directions s wo.x + t wo.y + sh_n wo.z, z [K, n] = wo.z)"""
    wo = local_directions(ids, K, seed)
    sh_n = np.asarray(sh_n, np.float64)
    s, t = coordinate_system(sh_n)
    w = s[None] * wo[:, 0:1] + t[None] * wo[:, 1:2] + sh_n[None] * wo[:, 2:3]
    return w, wo[:, 2]


def traced(sh_n, d, t, z):
    """[K, n]: direction k of an eligible sample is traced when wo.z > 0"""
    el, _ = eligible(sh_n, d, t)
    return el[None] & (z > 0)


def shadow_traced(front, n_q, lights):
    """[K, L, n]: the shadow ray towards light l is traced when the hit is seen from the front and <n_q, l_l> > 0; and
    the margins |<n_q, l_l>|"""
    co = np.einsum("kcn,lc->kln", np.asarray(n_q, np.float64), np.asarray(lights, np.float64)[:, :3])
    return np.asarray(front, bool)[:, None, :] & (co > 0), np.abs(co)


def unpack(hit_prim, lit_bits, L):
    """(hit [K, n], lit [K, L, n]) from the [K, n] record arrays"""
    prim = np.asarray(hit_prim).view(np.uint32)
    bits = np.asarray(lit_bits).view(np.uint8)
    lit = ((bits[:, None, :] >> np.arange(L, dtype=np.uint8)[None, :, None]) & 1).astype(bool)
    return prim != MISS, lit


# ---- the face normal of a grid triangle: P = A (j sx - 1, i sy - 1, h max_height) + T for to_world = [A | T] ----------
def prim_vertices(prim, W):
    """rows vi [3, m] and columns vj [3, m] of the three vertices: tri 0 = (v00, v10, v01), tri 1 = (v11, v01, v10)"""
    prim = np.asarray(prim, np.int64)
    cell, odd = prim >> 1, (prim & 1).astype(bool)
    cy, cx = cell // (W - 1), cell % (W - 1)
    vi = np.stack([np.where(odd, cy + 1, cy), np.where(odd, cy + 1, cy), np.where(odd, cy, cy + 1)])
    vj = np.stack([np.where(odd, cx + 1, cx), np.where(odd, cx, cx + 1), np.where(odd, cx + 1, cx)])
    return vi, vj


def _affine(to_world):
    """(A [3, 3], T [3]) of a row-major 3x4 to_world (None: the identity)"""
    M = np.eye(4)[:3] if to_world is None else np.asarray(to_world, np.float64).reshape(3, 4)
    return M[:, :3], M[:, 3]


def _edges(heights, prim, max_height, to_world=None):
    """the WORLD edges P1 - P0, P2 - P0 [3, m], the vertex ids and dP/dh = max_height A[:, 2] (the same for every vertex)"""
    H, W = heights.shape
    A, T = _affine(to_world)
    vi, vj = prim_vertices(prim, W)
    Q = np.stack([vj * (2.0 / (W - 1)) - 1.0, vi * (2.0 / (H - 1)) - 1.0, np.asarray(heights, np.float64)[vi, vj] * max_height], 1)
    P = np.einsum("cd,kdm->kcm", A, Q) + T[None, :, None]                 # [3 vertices, 3, m]
    return P[1] - P[0], P[2] - P[0], vi, vj, max_height * A[:, 2]


def face_normal(heights, prim, max_height, flip=False, to_world=None):
    """[3, m]: normalize(cross(P1 - P0, P2 - P0)) of the world vertices (not a transformed object normal: a mirror turns
    it over), negated with flip_normals"""
    e1, e2, _, _, _ = _edges(heights, prim, max_height, to_world)
    N = np.cross(e1, e2, axis=0)
    n = N / np.linalg.norm(N, axis=0)
    return -n if flip else n


def face_normal_jvp(heights, prim, max_height, dheights, flip=False, to_world=None):
    """[3, m]: the tangent of face_normal for the height tangent dheights [H, W]"""
    e1, e2, vi, vj, ez = _edges(heights, prim, max_height, to_world)
    dz = np.asarray(dheights, np.float64)[vi, vj]
    de1, de2 = ez[:, None] * (dz[1] - dz[0])[None], ez[:, None] * (dz[2] - dz[0])[None]
    N = np.cross(e1, e2, axis=0)
    r = 1.0 / np.linalg.norm(N, axis=0)
    n = N * r
    dN = np.cross(de1, e2, axis=0) + np.cross(e1, de2, axis=0)
    dn = (dN - n * (n * dN).sum(0)) * r
    return -dn if flip else dn


def face_normal_vjp(heights, prim, max_height, gn, flip=False, to_world=None):
    """[H, W]: the gradients gn [3, m] of the normals of `prim`, carried to the heights and added up"""
    e1, e2, vi, vj, ez = _edges(heights, prim, max_height, to_world)
    gn = -np.asarray(gn, np.float64) if flip else np.asarray(gn, np.float64)
    N = np.cross(e1, e2, axis=0)
    r = 1.0 / np.linalg.norm(N, axis=0)
    n = N * r
    gN = (gn - n * (n * gn).sum(0)) * r
    g1 = (np.cross(e2, gN, axis=0) * ez[:, None]).sum(0)                 # <dP/dh, dL/de1>
    g2 = (np.cross(gN, e1, axis=0) * ez[:, None]).sum(0)
    out = np.zeros(heights.shape)
    np.add.at(out, (vi[0], vj[0]), -(g1 + g2))
    np.add.at(out, (vi[1], vj[1]), g1)
    np.add.at(out, (vi[2], vj[2]), g2)
    return out


# ---- value, adjoint, tangent ---------------------------------------------------------------------------------------
def _R(sh_n, d, t, hit, lit, n_q, lights, albedo):
    """R [K, L, n] = albedo/pi E_l lit <n_q, l_l> (records of samples that are not eligible ignored) and the part
    without the cosine, A [K, L, n] = albedo/pi E_l lit"""
    lights = np.asarray(lights, np.float64)
    el, _ = eligible(sh_n, d, t)
    on = np.asarray(lit, bool) & np.asarray(hit, bool)[:, None, :] & el[None, None, :]
    A = on * (albedo / np.pi) * lights[None, :, 3, None]
    co = np.einsum("kcn,lc->kln", np.asarray(n_q, np.float64), lights[:, :3])
    return A * co, A


def _weight(weight, n):
    return np.ones(n) if weight is None else np.asarray(weight, np.float64)


def forward(sh_n, d, t, weight, hit, lit, n_q, lights, albedo, spp, attached=None, wz=None):
    """(image [L, n / spp], values [L, n], abs [L, n / spp]: the sum of the absolute values of an image element's
    addends).  attached (with wz = (w, z)): the value as a function of the ATTACHED shading normal, every term times
    <attached, w_k> / z_k with the directions frozen (prb.py:213-223) -- 1 at attached = sh_n, and what the adjoint's
    grad_sh_n differentiates."""
    K, n = np.asarray(hit).shape
    R, _ = _R(sh_n, d, t, hit, lit, n_q, lights, albedo)
    if attached is not None:
        w, z = wz
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(z > 0, np.einsum("cn,kcn->kn", np.asarray(attached, np.float64), w) / z, 0.0)
        R = R * ratio[:, None, :]
    terms = (_weight(weight, n) * (albedo / K))[None, None] * R           # [K, L, n]
    value = terms.sum(0)
    L = value.shape[0]
    return (value.reshape(L, -1, spp).mean(2), value,
            np.abs(terms).sum(0).reshape(L, -1, spp).sum(2) / spp)


def adjoint(sh_n, d, t, weight, hit, lit, n_q, lights, albedo, spp, w, z, grad_image):
    """dict: grad_sh_n [3, n], grad_weight [n], grad_nq [K, 3, n] (the gradient gN of every record's n_q), and the sums
    of the absolute values of the addends of grad_sh_n / grad_weight (abs_sh_n, abs_weight)"""
    K, n = np.asarray(hit).shape
    lights = np.asarray(lights, np.float64)
    R, A = _R(sh_n, d, t, hit, lit, n_q, lights, albedo)
    g = np.repeat(np.asarray(grad_image, np.float64), spp, axis=1) / spp   # [L, n]
    c = albedo / K
    wgt = _weight(weight, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        wz = np.where(z[:, None, :] > 0, w / z[:, None, :], 0.0)        # [K, 3, n]
    gR = g[None] * R                                                      # [K, L, n]
    G = gR.sum(1)                                                         # [K, n]
    return {"grad_sh_n": (wgt * c)[None] * (G[:, None, :] * wz).sum(0),
            "grad_weight": c * G.sum(0),
            "grad_nq": (wgt * c)[None, None] * np.einsum("kln,lc->kcn", g[None] * A, lights[:, :3]),
            "abs_sh_n": (np.abs(wgt) * c)[None] * (np.abs(gR).sum(1)[:, None, :] * np.abs(wz)).sum(0),
            "abs_weight": c * np.abs(gR).sum((0, 1))}


def tangent(sh_n, d, t, weight, hit, lit, n_q, lights, albedo, spp, w, z, dsh_n=None, dweight=None, dn_q=None):
    """(dimage [L, n / spp], abs [L, n / spp]) for tangents dsh_n [3, n], dweight [n] and dn_q [K, 3, n] (None: zero)"""
    K, n = np.asarray(hit).shape
    lights = np.asarray(lights, np.float64)
    R, A = _R(sh_n, d, t, hit, lit, n_q, lights, albedo)
    wgt = _weight(weight, n)
    terms = []
    if dsh_n is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            wz = np.where(z[:, None, :] > 0, w / z[:, None, :], 0.0)
        for c in range(3):
            terms.append(wgt[None, None] * R * (np.asarray(dsh_n, np.float64)[c][None] * wz[:, c])[:, None, :])
    if dweight is not None:
        terms.append(np.asarray(dweight, np.float64)[None, None] * R)
    if dn_q is not None:
        for c in range(3):
            terms.append(wgt[None, None] * A * (np.asarray(dn_q, np.float64)[:, c][:, None, :] * lights[None, :, c, None]))
    L = len(lights)
    if not terms:
        return np.zeros((L, n // spp)), np.zeros((L, n // spp))
    terms = (albedo / K) * np.stack(terms)                                # [parts, K, L, n]
    return (terms.sum((0, 1)).reshape(L, -1, spp).mean(2),
            np.abs(terms).sum((0, 1)).reshape(L, -1, spp).sum(2) / spp)

"""The thin lens (include/hf.h hf_thinlens_rays, hf_thinlens_project and their derivatives) restated in numpy the way
the reference computes it (src/sensors/thinlens.cpp:216-254, 305-350), NOT from the closed forms of the header:
camera_to_sample is sensor_ref's product of the five matrices, sample_to_camera numpy.linalg.inv of it, the aperture
point is warp::square_to_uniform_disk_concentric (warp.h) of a second TEA draw, and sample_ray / sample_direction follow
the reference line by line.  The tangents are the chain rule through exactly those steps, in the 15 variables to_world
(12), x_fov, aperture_radius and focus_distance; the adjoints are reverse sweeps through the same steps, written on their
own.  closed_rays / closed_project are the header's closed forms, for tests/test_thinlens_ref.py to hold against the
steps.  float64 by default; dt=np.float32 evaluates the same text in float32 (scripts/thinlens_f32_error.py).  A helper
module."""
import types

import numpy as np

import sensor_ref as R
from sensor_ref import camera_to_sample, film_positions, tea32

PAIR = 0x4C454E53   # HF_THINLENS_PAIR


def lens(to_world, fov, radius, focus, film=(13, 7), crop=None, near=1e-2, far=1e4):
    s = R.sensor(R.PERSPECTIVE, to_world, fov, film, crop, near, far)
    s.radius, s.focus = radius, focus
    return s


def pinhole(s):
    """the perspective sensor of the same pose, film and clip range"""
    return R.sensor(R.PERSPECTIVE, s.to_world, s.fov, s.film, s.crop, s.near, s.far)


def aperture_samples(ids, seed):
    """the aperture sample [2, n] of the wavefront indices ids: key = tea32(seed, PAIR).v0, (a0, a1) = tea32(key, id),
    (a >> 9) 2^-23 (exact in float32)"""
    ids = np.asarray(ids, np.uint64)
    key, _ = tea32(np.uint64(seed), np.uint64(PAIR))
    a0, a1 = tea32(np.full_like(ids, key), ids)
    return np.stack([(a >> np.uint64(9)).astype(np.float64) * 2.0 ** -23 for a in (a0, a1)])


def disk(sample, dt=np.float64):
    """warp::square_to_uniform_disk_concentric as (x, y, 0) rows [3, n]"""
    smp = np.asarray(sample, dt)
    x, y = dt(2) * smp[0] - dt(1), dt(2) * smp[1] - dt(1)
    is_zero = (x == 0) & (y == 0)
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    phi = dt(0.25 * np.pi) * rp / np.where(is_zero, dt(1), r)
    phi = np.where(q13, dt(0.5 * np.pi) - phi, phi)
    phi = np.where(is_zero, dt(0), phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros_like(r)]).astype(dt)


def _near_plane(s, pos, dt, d_fov=None):
    """sample_to_camera * (position_sample, 0): (C, S, smp4, h, near_p, dnear_p)"""
    C, dC = camera_to_sample(s, dt, d_fov)
    S = np.linalg.inv(C)
    dS = -S @ dC @ S
    smp4 = np.stack([(pos[0] - dt(s.crop[0])) / dt(s.crop[2]), (pos[1] - dt(s.crop[1])) / dt(s.crop[3]), np.zeros_like(pos[0]),
                     np.ones_like(pos[0])])
    h, dh = S @ smp4, dS @ smp4
    return C, S, smp4, h, h[:3] / h[3], dh[:3] / h[3] - h[:3] * dh[3] / h[3] ** 2


def rays(s, pos, D, dt=np.float64, d_to_world=None, d_fov=None, d_radius=0.0, d_focus=0.0):
    """(o [3, n], d [3, n], maxt [n], do, dd): thinlens.cpp:216-254 at the film positions pos with the disk points D, and
    its tangent"""
    pos, D = np.asarray(pos, dt), np.asarray(D, dt)
    A, c = s.to_world[:, :3].astype(dt), s.to_world[:, 3].astype(dt)
    dA, dc = R._split(d_to_world, dt)
    rad, foc, dr, df = dt(s.radius), dt(s.focus), dt(d_radius), dt(d_focus)
    _, _, _, _, near_p, dnear_p = _near_plane(s, pos, dt, d_fov)
    ap, dap = rad * D, dr * D                              # :235-236
    fd = foc / near_p[2]                                   # :239
    dfd = df / near_p[2] - foc * dnear_p[2] / near_p[2] ** 2
    focus_p, dfocus_p = near_p * fd, dnear_p * fd + near_p * dfd
    e, de = focus_p - ap, dfocus_p - dap                   # :242
    ln = np.linalg.norm(e, axis=0)
    dl = e / ln
    ddl = de / ln - e * (e * de).sum(0) / ln ** 3
    o0 = A @ ap + c[:, None]                               # :244
    do0 = dA @ ap + A @ dap + dc[:, None]
    d, dd = A @ dl, dA @ dl + A @ ddl                      # :245
    inv_z = dt(1) / dl[2]                                  # :247-251
    dinv_z = -ddl[2] * inv_z ** 2
    near_t, far_t = dt(s.near) * inv_z, dt(s.far) * inv_z
    o = o0 + d * near_t
    do = do0 + dd * near_t + d * dt(s.near) * dinv_z
    return o, d, far_t - near_t, do, dd


def rays_adjoint(s, pos, D, grad_o, grad_d, dt=np.float64):
    """(grad_to_world [12], grad_fov, grad_radius, grad_focus): the reverse sweep through the steps of rays()"""
    pos, D, go, gd = (np.asarray(v, dt) for v in (pos, D, grad_o, grad_d))
    A = s.to_world[:, :3].astype(dt)
    rad, foc = dt(s.radius), dt(s.focus)
    C, S, smp4, h, near_p, _ = _near_plane(s, pos, dt)
    ap = rad * D
    fd = foc / near_p[2]
    e = near_p * fd - ap
    ln = np.linalg.norm(e, axis=0)
    dl = e / ln
    d = A @ dl
    inv_z = dt(1) / dl[2]
    near_t = dt(s.near) * inv_z
    g_d = gd + go * near_t                                 # o = o0 + d near_t
    g_inv_z = dt(s.near) * (go * d).sum(0)
    gA = g_d @ dl.T + go @ ap.T                            # d = A dl, o0 = A ap + c
    g_dl = A.T @ g_d
    g_dl[2] += -g_inv_z * inv_z ** 2                       # inv_z = 1 / dl.z
    g_e = (g_dl - dl * (dl * g_dl).sum(0)) / ln            # dl = e / |e|
    g_ap = A.T @ go - g_e                                  # e = focus_p - ap
    g_fd = (g_e * near_p).sum(0)                           # focus_p = near_p fd
    g_near_p = g_e * fd
    g_near_p[2] += -g_fd * foc / near_p[2] ** 2            # fd = focus / near_p.z
    g_focus = (g_fd / near_p[2]).sum()
    g_radius = (g_ap * D).sum()                            # ap = radius D
    gS = R._unhom_back(h, g_near_p) @ smp4.T
    gC = -S.T @ gS @ S.T
    return (np.concatenate([gA, go.sum(1)[:, None]], axis=1).reshape(-1), R._fov_back(s, gC, R._pre(s, dt), dt), g_radius,
            g_focus)


def project(s, p, D, active=None, dt=np.float64, dp=None, d_to_world=None, d_fov=None, d_radius=0.0, d_focus=0.0):
    """sample_direction (thinlens.cpp:305-350) for the points p [3, n] with the disk points D: a namespace with ref,
    inside, valid, uv (pixels of the whole film), weight (unmasked), s_crop, and the tangents duv, dweight"""
    p, D = np.asarray(p, dt), np.asarray(D, dt)
    n = p.shape[1]
    rad, foc, dr, df = dt(s.radius), dt(s.focus), dt(d_radius), dt(d_focus)
    T = np.eye(4, dtype=dt)
    T[:3] = s.to_world.astype(dt)
    dT = np.zeros((4, 4), dt)
    dT[:3, :3], dT[:3, 3] = R._split(d_to_world, dt)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    dp4 = np.concatenate([np.zeros((3, n), dt) if dp is None else np.asarray(dp, dt), np.zeros((1, n), dt)])
    ref4 = Ti @ p4                                         # :309-310
    dref4 = Ti @ dp4 - Ti @ dT @ ref4
    ref, dref = ref4[:3], dref4[:3]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    inside = act & (ref[2] >= dt(s.near)) & (ref[2] <= dt(s.far))      # :315
    ap, dap = rad * D, dr * D                              # :320-321
    lr, dlr = ref - ap, dref - dap                         # :324-327
    dist = np.linalg.norm(lr, axis=0)
    ddist = (lr * dlr).sum(0) / dist
    local, dlocal = lr / dist, dlr / dist - lr * ddist / dist ** 2
    ct = local[2]                                          # :330-331
    inv_ct, dinv_ct = 1 / ct, -dlocal[2] / ct ** 2
    k, dk = foc * inv_ct, df * inv_ct + foc * dinv_ct
    Fp, dFp = ap + local * k, dap + dlocal * k + local * dk            # :333
    Fp4 = np.concatenate([Fp, np.ones((1, n), dt)])
    dFp4 = np.concatenate([dFp, np.zeros((1, n), dt)])
    C, dC = camera_to_sample(s, dt, d_fov)
    h = C @ Fp4
    dh = dC @ Fp4 + C @ dFp4
    sc = h[:2] / h[3]
    dsc = dh[:2] / h[3] - h[:2] * dh[3] / h[3] ** 2
    valid = inside & (sc[0] >= 0) & (sc[0] <= 1) & (sc[1] >= 0) & (sc[1] <= 1)   # :334 (x and y; the header's deviation)
    size, off = np.array(s.crop[2:], dt)[:, None], np.array(s.crop[:2], dt)[:, None]
    uv, duv = sc * size + off, dsc * size                  # :340
    S = np.linalg.inv(C)
    norm, dnorm = R._image_rect(S, -S @ dC @ S)
    value, dvalue = norm * inv_ct ** 3, dnorm * inv_ct ** 3 + 3 * norm * inv_ct ** 2 * dinv_ct    # :335
    weight = value / dist ** 2                             # :349
    dweight = dvalue / dist ** 2 - 2 * value * ddist / dist ** 3
    return types.SimpleNamespace(ref=ref, inside=inside, valid=valid, uv=uv, weight=weight, s_crop=sc, duv=duv, dweight=dweight)


def project_adjoint(s, p, D, active, grad_uv, grad_weight, dt=np.float64):
    """(grad_p [3, n], grad_to_world [12], grad_fov, grad_radius, grad_focus): the reverse sweep through the steps of
    project(); uv counts where inside, weight where valid"""
    r = project(s, p, D, active, dt)
    p, D = np.asarray(p, dt), np.asarray(D, dt)
    n = p.shape[1]
    rad, foc = dt(s.radius), dt(s.focus)
    guv, gw = (np.asarray(grad_uv, dt) * r.inside), (np.asarray(grad_weight, dt) * r.valid)
    T = np.eye(4, dtype=dt)
    T[:3] = s.to_world.astype(dt)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    ref4 = Ti @ p4
    ap = rad * D
    lr = ref4[:3] - ap
    dist = np.linalg.norm(lr, axis=0)
    local = lr / dist
    ct = local[2]
    inv_ct = 1 / ct
    Fp4 = np.concatenate([ap + local * (foc * inv_ct), np.ones((1, n), dt)])
    C, _ = camera_to_sample(s, dt)
    S = np.linalg.inv(C)
    h = C @ Fp4
    norm, _ = R._image_rect(S, np.zeros_like(S))
    value = norm * inv_ct ** 3
    # weight = value / dist^2, value = norm inv_ct^3
    g_value = gw / dist ** 2
    g_dist = -2 * gw * value / dist ** 3
    g_norm = (g_value * inv_ct ** 3).sum()
    g_inv_ct = 3 * norm * inv_ct ** 2 * g_value
    # uv = sc size + off, sc = h[:2] / h[3], h = C Fp4
    size = np.array(s.crop[2:], dt)[:, None]
    g_h = R._unhom_back(h, guv * size)
    gC = g_h @ Fp4.T
    g_Fp = (C.T @ g_h)[:3]
    # Fp = ap + local k, k = focus inv_ct
    g_ap = g_Fp.copy()
    g_local = g_Fp * (foc * inv_ct)
    g_k = (g_Fp * local).sum(0)
    g_focus = (g_k * inv_ct).sum()
    g_inv_ct = g_inv_ct + g_k * foc
    g_local[2] += -g_inv_ct / ct ** 2                      # inv_ct = 1 / local.z
    g_lr = g_local / dist                                  # local = lr / dist
    g_dist = g_dist - (g_local * lr).sum(0) / dist ** 2
    g_lr += g_dist * lr / dist                             # dist = |lr|
    g_ap -= g_lr                                           # lr = ref - ap
    g_radius = (g_ap * D).sum()                            # ap = radius D
    g_ref4 = np.concatenate([g_lr, np.zeros((1, n), dt)])
    # norm = 1 / |vol| of the image rectangle, from S = C^-1 (thinlens.cpp:204-210)
    e = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]], dt)
    h2 = S @ e
    q = h2[:3] / h2[3]
    rc = q[:2] / q[2]
    ext = rc[:, 1] - rc[:, 0]
    vol = ext[0] * ext[1]
    g_vol = -np.sign(vol) * g_norm / vol ** 2
    g_ext = np.array([g_vol * ext[1], g_vol * ext[0]])
    g_rc = np.stack([-g_ext, g_ext], axis=1)
    g_q = np.zeros_like(q)
    g_q[:2] = g_rc / q[2]
    g_q[2] = -(g_rc * q[:2]).sum(0) / q[2] ** 2
    gS = R._unhom_back(h2, g_q) @ e.T
    gC = gC - S.T @ gS @ S.T
    gT = -Ti.T @ (g_ref4 @ p4.T) @ Ti.T                    # ref4 = T^-1 p4
    return (Ti.T @ g_ref4)[:3], gT[:3].reshape(-1), R._fov_back(s, gC, R._pre(s, dt), dt), g_radius, g_focus


# ---- the header's closed forms, for the CPU test to hold against the steps ----
def closed_rays(s, pos, D):
    A, c = s.to_world[:, :3], s.to_world[:, 3]
    wx, wy = R.closed_w(s, pos)
    tau = np.tan(s.fov * np.pi / 360.0)
    v = np.stack([wx * tau, wy * tau, np.ones_like(wx)])
    e = s.focus * v - s.radius * D
    ln = np.linalg.norm(e, axis=0)
    o = c[:, None] + A @ (s.radius * (1.0 - s.near / s.focus) * D + s.near * v)
    return o, A @ (e / ln), (s.far - s.near) * ln / s.focus


def closed_project(s, p, D):
    """(uv, weight) of the header: F = r D + q f / q.z, uv = g film_size, weight = |q| / (A' q.z^3)"""
    A, c = s.to_world[:, :3], s.to_world[:, 3]
    ref = np.linalg.solve(A, p - c[:, None])
    q = ref - s.radius * D
    F = s.radius * D + q * s.focus / q[2]
    tau, a = np.tan(s.fov * np.pi / 360.0), s.film[0] / s.film[1]
    uv = np.stack([0.5 * (1 - F[0] / (s.focus * tau)) * s.film[0], 0.5 * (1 - a * F[1] / (s.focus * tau)) * s.film[1]])
    area = (2 * tau) ** 2 / a * (s.crop[2] * s.crop[3]) / (s.film[0] * s.film[1])
    return uv, np.linalg.norm(q, axis=0) / (area * q[2] ** 3)


# ---- the scenes of tests/test_gpu_thinlens.py and scripts/thinlens_f32_error.py ----
FILM, CROP, FOV, POSE, SPPS, SEED = R.FILM, R.CROP, R.FOV, R.POSE, R.SPPS, R.SEED
LENSES = tuple((r, f) for r in (0.0, 0.05, 0.3) for f in (0.5, 2.0))
NEAR = 1e-2
PROJECT_FAR = 50.0              # the far plane of the projection scenes: points on both sides of both planes
PROJECT_SEED = 5


def scene(crop, radius, focus, **kw):
    kw.setdefault("near", NEAR)
    return lens(POSE, FOV, radius, focus, FILM, crop, **kw)


def wavefront(s, spp, seed=SEED):
    """(ids, pos, D) of the whole wavefront of the crop window"""
    ids = np.arange(s.crop[2] * s.crop[3] * spp, dtype=np.uint64)
    return ids, film_positions(s, ids, spp, seed), disk(aperture_samples(ids, seed))


def directions(seed=11):
    """a tangent (d_to_world [12], d_fov, d_radius, d_focus), float32 values"""
    dtw, dfov = R.directions(seed)
    return dtw, dfov, np.float32(0.4), np.float32(-0.6)


cotangents = R.cotangents


def project_points(s, n=360, seed=13):
    """(p [3, n] float32, active [n] bool, D [3, n]): world points built so that no mask is decided by rounding -- lane i
    lies on a ray through ITS aperture point (wavefront index i, PROJECT_SEED) whose s_crop is drawn in [0.02, 0.98]^2 or at
    least 0.02 outside on one axis, at a depth in [1.05 near, 0.95 far] or outside by the same factor -- with every
    combination present"""
    rng = np.random.default_rng(seed)
    sc = rng.uniform(0.02, 0.98, (2, n))
    out = rng.random(n) < 0.25
    axis, side = rng.integers(0, 2, n), rng.integers(0, 2, n)
    off = np.where(side == 1, rng.uniform(1.02, 1.4, n), rng.uniform(-0.4, -0.02, n))
    sc[0] = np.where(out & (axis == 0), off, sc[0])
    sc[1] = np.where(out & (axis == 1), off, sc[1])
    z = np.exp(rng.uniform(np.log(1.05 * s.near), np.log(0.95 * s.far), n))
    cut = rng.random(n)
    z = np.where(cut < 0.1, rng.uniform(0.3 * s.near, s.near / 1.05, n), np.where(cut > 0.9, rng.uniform(1.05 * s.far, 1.5 * s.far, n), z))
    pos = np.stack([s.crop[0] + sc[0] * s.crop[2], s.crop[1] + sc[1] * s.crop[3]])
    wx, wy = R.closed_w(s, pos)
    tau = np.tan(s.fov * np.pi / 360.0)
    D = disk(aperture_samples(np.arange(n, dtype=np.uint64), PROJECT_SEED))
    ref = s.radius * D * (1.0 - z / s.focus) + np.stack([wx * tau, wy * tau, np.ones(n)]) * z
    p = (s.to_world[:, :3] @ ref + s.to_world[:, 3:4]).astype(np.float32)
    return p, rng.random(n) < 0.9, D


def mask_margins(s, p, D):
    """how far the points keep from the masks, on the float64 restatement: (the least distance of s_crop from the
    window's edges, the least |ref.z / plane - 1| over both clip planes)"""
    r = project(s, p, D)
    edge = np.minimum(np.abs(r.s_crop), np.abs(r.s_crop - 1.0)).min()
    depth = min(np.abs(r.ref[2] / s.near - 1.0).min(), np.abs(r.ref[2] / s.far - 1.0).min())
    return float(edge), float(depth)


project_cotangents = R.project_cotangents
err_abs, err_l2 = R.err_abs, R.err_l2


def ray_derivative_errors(s, spp, rays_t, rays_a):
    """the errors of a tangent (do, dd) = rays_t and an adjoint (grad_to_world, grad_fov, grad_radius, grad_focus) = rays_a
    of the scene (s, spp) under directions() and cotangents(), against the float64 restatement"""
    ids, pos, D = wavefront(s, spp)
    go, gd = cotangents(len(ids))
    _, _, _, do, dd = rays(s, pos, D, np.float64, *directions())
    ref = rays_adjoint(s, pos, D, go, gd)
    return {"tangent_do": err_abs(rays_t[0], do), "tangent_dd": err_abs(rays_t[1], dd),
            "adjoint": err_l2(np.concatenate([np.ravel(v) for v in rays_a]), np.concatenate([np.ravel(v) for v in ref]))}


project_errors = R.project_errors       # (grad13 holds the 15 numbers here)


def project_case(s, dt=np.float64):
    """the projection scene of s evaluated by the restatement in dt: (p, active, D, namespace as project_errors takes it)"""
    p, active, D = project_points(s)
    dp = np.random.default_rng(15).standard_normal(p.shape).astype(np.float32) * np.float32(0.2)
    r = project(s, p, D, active, dt, dp, *directions())
    guv, gw = project_cotangents(project(s, p, D, active).weight)
    gp, *g = project_adjoint(s, p, D, active, guv, gw, dt)
    r.grad_p, r.grad13, r.dp, r.guv, r.gw = gp, np.concatenate([np.ravel(v) for v in g]), dp, guv, gw
    return p, active, D, r

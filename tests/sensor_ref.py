"""The sensor (include/hf.h hf_sensor_rays, hf_sensor_project and their derivatives) restated in numpy the way the
reference computes it, NOT from the closed forms of the header: camera_to_sample is the product of the five matrices of
perspective_projection / orthographic_projection (sensor.h:228-301, transform.h:216-233), sample_to_camera is
numpy.linalg.inv of it, sample_ray and sample_direction follow perspective.cpp:198-234, 279-318, 334-383 and
orthographic.cpp:119-142 line by line, and the tangents are the chain rule through exactly those steps (d inv(C) =
-inv(C) dC inv(C), the quotient rule of the homogeneous division, ...).  The adjoints are reverse sweeps through the same
steps, written on their own: they share no line with the tangents.  closed_rays / closed_project are the header's closed forms, for tests/test_sensor_ref.py to hold against
the matrices; ortho_closed is workload.ortho_rays' expression in its operation order.  float64 by default; dt=np.float32
evaluates the same text in float32 (scripts/sensor_f32_error.py).  A helper module."""
import types

import numpy as np

PERSPECTIVE, ORTHOGRAPHIC = 0, 1


def sensor(type_, to_world, fov=None, film=(13, 7), crop=None, near=1e-2, far=1e4):
    m = np.asarray(to_world, np.float64).reshape(-1, 4)[:3]
    return types.SimpleNamespace(type=type_, to_world=m, fov=fov, film=tuple(film), crop=tuple(crop or (0, 0) + tuple(film)),
                                 near=near, far=far)


def look_at(origin, target, up):
    """transform.h:254-282 (workload.look_at's text)"""
    o, t, u = (np.asarray(a, np.float64) for a in (origin, target, up))
    d = (t - o) / np.linalg.norm(t - o)
    left = np.cross(u, d)
    left /= np.linalg.norm(left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(d, left), d, o
    return m


def tea32(v0, v1, rounds=4):
    """sample_tea_32 (random.h:76-91) on uint64 arrays that hold uint32 values"""
    M = np.uint64(0xFFFFFFFF)
    v0, v1 = np.asarray(v0, np.uint64) & M, np.asarray(v1, np.uint64) & M
    s = np.uint64(0)
    for _ in range(rounds):
        s = (s + np.uint64(0x9E3779B9)) & M
        v0 = (v0 + ((((v1 << np.uint64(4)) & M) + np.uint64(0xA341316C)) ^ (v1 + s) ^ ((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)))) & M
        v1 = (v1 + ((((v0 << np.uint64(4)) & M) + np.uint64(0xAD90777D)) ^ (v0 + s) ^ ((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)))) & M
    return v0, v1


def film_positions(s, ids, spp, seed):
    """pos [2, n] in pixels of the whole film, float64 (exact: an integer below 2^32 plus a multiple of 2^-23):
    integrator.cpp:251-268 over the crop window, common.py:331-337"""
    ids = np.asarray(ids, np.uint64)
    v0, v1 = tea32(np.full_like(ids, seed), ids)
    pix = ids // np.uint64(spp)
    py = pix // np.uint64(s.crop[2])
    px = pix - py * np.uint64(s.crop[2])
    j = [(v >> np.uint64(9)).astype(np.float64) * 2.0 ** -23 for v in (v0, v1)]
    return np.stack([px.astype(np.float64) + s.crop[0] + j[0], py.astype(np.float64) + s.crop[1] + j[1]])


def _scale(x, y, z, dt):
    return np.diag(np.array([x, y, z, 1], dt))


def _translate(x, y, z, dt):
    m = np.eye(4, dtype=dt)
    m[:3, 3] = (x, y, z)
    return m


def _pre(s, dt):
    """the four matrices in front of the projection (sensor.h:256-261, 294-299)"""
    film, cs, co = (np.array(v, dt) for v in (s.film, s.crop[2:], s.crop[:2]))
    rel_size, rel_offset, aspect = cs / film, co / film, film[0] / film[1]
    return _scale(dt(1) / rel_size[0], dt(1) / rel_size[1], 1, dt) @ _translate(-rel_offset[0], -rel_offset[1], 0, dt) \
        @ _scale(-0.5, dt(-0.5) * aspect, 1, dt) @ _translate(-1, dt(-1) / aspect, 0, dt)


def camera_to_sample(s, dt=np.float64, d_fov=None):
    """the five matrices; with d_fov also the tangent of the product (perspective: d cot(x) = -dx / sin(x)^2)"""
    pre = _pre(s, dt)
    near, far = dt(s.near), dt(s.far)
    recip = dt(1) / (far - near)
    if s.type == ORTHOGRAPHIC:   # transform.h: scale(1, 1, 1 / (far - near)) translate(0, 0, -near)
        return pre @ _scale(1, 1, recip, dt) @ _translate(0, 0, -near, dt), np.zeros((4, 4), dt)
    half = np.deg2rad(dt(s.fov) * dt(0.5))
    cot = dt(1) / np.tan(half)
    P = np.zeros((4, 4), dt)
    P[0, 0] = P[1, 1] = cot
    P[2, 2], P[2, 3], P[3, 2] = far * recip, -near * far * recip, 1
    dP = np.zeros((4, 4), dt)
    if d_fov is not None:
        dP[0, 0] = dP[1, 1] = -dt(d_fov) * dt(np.pi / 360) / np.sin(half) ** 2
    return pre @ P, pre @ dP


def _hom(M, q):
    """Transform * Point: q [3, n] -> the homogeneous [4, n] image"""
    return M @ np.concatenate([q, np.ones((1, q.shape[1]), q.dtype)])


def _split(d_to_world, dt):
    """(dA [3, 3], dc [3]) of a 12-vector tangent of to_world; None: zeros"""
    m = np.zeros((3, 4), dt) if d_to_world is None else np.asarray(d_to_world, dt).reshape(3, 4)
    return m[:, :3], m[:, 3]


def rays(s, pos, dt=np.float64, d_to_world=None, d_fov=None):
    """(o [3, n], d [3, n], maxt [n], do, dd): sample_ray at the film positions pos and its tangent (zeros without one)"""
    pos = np.asarray(pos, dt)
    A, c = s.to_world[:, :3].astype(dt), s.to_world[:, 3].astype(dt)
    dA, dc = _split(d_to_world, dt)
    C, dC = camera_to_sample(s, dt, d_fov)
    S = np.linalg.inv(C)
    dS = -S @ dC @ S
    smp = np.stack([(pos[0] - dt(s.crop[0])) / dt(s.crop[2]), (pos[1] - dt(s.crop[1])) / dt(s.crop[3]), np.zeros_like(pos[0])])
    h, dh = _hom(S, smp), dS @ np.concatenate([smp, np.ones((1, smp.shape[1]), dt)])
    near_p = h[:3] / h[3]
    dnear_p = dh[:3] / h[3] - h[:3] * dh[3] / h[3] ** 2
    if s.type == ORTHOGRAPHIC:
        o = A @ near_p + c[:, None]
        z = A[:, 2]
        d = z / np.linalg.norm(z)
        dz = dA[:, 2]
        dd = (dz - d * (d @ dz)) / np.linalg.norm(z)
        n = pos.shape[1]
        return (o, np.repeat(d[:, None], n, 1), np.full(n, dt(s.far) - dt(s.near)), dA @ near_p + A @ dnear_p + dc[:, None],
                np.repeat(dd[:, None], n, 1))
    ln = np.linalg.norm(near_p, axis=0)
    dl = near_p / ln                                      # perspective.cpp:222
    ddl = dnear_p / ln - near_p * (near_p * dnear_p).sum(0) / ln ** 3
    d = A @ dl                                            # :225
    dd = dA @ dl + A @ ddl
    inv_z = dt(1) / dl[2]                                 # :227-231
    dinv_z = -ddl[2] * inv_z ** 2
    near_t, far_t = dt(s.near) * inv_z, dt(s.far) * inv_z
    o = c[:, None] + d * near_t
    do = dc[:, None] + dd * near_t + d * dt(s.near) * dinv_z
    return o, d, far_t - near_t, do, dd


def _image_rect(S, dS):
    """(normalization = 1 / volume of m_image_rect, its tangent): perspective.cpp:185-191"""
    e = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]], S.dtype)
    h, dh = S @ e, dS @ e
    p, dp = h[:3] / h[3], dh[:3] / h[3] - h[:3] * dh[3] / h[3] ** 2
    r, dr = p[:2] / p[2], dp[:2] / p[2] - p[:2] * dp[2] / p[2] ** 2
    ext, dext = r[:, 1] - r[:, 0], dr[:, 1] - dr[:, 0]
    vol = ext[0] * ext[1]
    dvol = dext[0] * ext[1] + ext[0] * dext[1]
    sign = np.sign(vol)                                    # (the box orders its corners: the volume is the absolute value)
    return 1 / (sign * vol), -sign * dvol / vol ** 2


def project(s, p, active=None, dt=np.float64, dp=None, d_to_world=None, d_fov=None):
    """sample_direction of the perspective sensor for the points p [3, n]: a namespace with ref, inside, valid, uv
    (pixels of the whole film; every lane), weight (every lane, unmasked), s_crop, and the tangents duv, dweight"""
    p = np.asarray(p, dt)
    n = p.shape[1]
    T = np.eye(4, dtype=dt)
    T[:3] = s.to_world.astype(dt)
    dT = np.zeros((4, 4), dt)
    dT[:3, :3], dT[:3, 3] = _split(d_to_world, dt)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    dp4 = np.concatenate([np.zeros((3, n), dt) if dp is None else np.asarray(dp, dt), np.zeros((1, n), dt)])
    ref4 = Ti @ p4                                         # perspective.cpp:283-284
    dref4 = Ti @ dp4 - Ti @ dT @ ref4
    ref, dref = ref4[:3], dref4[:3]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    inside = act & (ref[2] >= dt(s.near)) & (ref[2] <= dt(s.far))
    C, dC = camera_to_sample(s, dt, d_fov)
    h = C @ ref4
    dh = dC @ ref4 + C @ dref4
    sc = h[:2] / h[3]                                      # :296-298
    dsc = dh[:2] / h[3] - h[:2] * dh[3] / h[3] ** 2
    valid = inside & (sc[0] >= 0) & (sc[0] <= 1) & (sc[1] >= 0) & (sc[1] <= 1)
    size, off = np.array(s.crop[2:], dt)[:, None], np.array(s.crop[:2], dt)[:, None]
    uv, duv = sc * size + off, dsc * size                  # :304, common.py:383-400
    dist = np.linalg.norm(ref, axis=0)                     # :306-309
    ddist = (ref * dref).sum(0) / dist
    local, dlocal = ref / dist, dref / dist - ref * ddist / dist ** 2
    S = np.linalg.inv(C)
    norm, dnorm = _image_rect(S, -S @ dC @ S)
    inv_ct, dinv_ct = 1 / local[2], -dlocal[2] / local[2] ** 2     # :372-382
    imp, dimp = norm * inv_ct ** 3, dnorm * inv_ct ** 3 + 3 * norm * inv_ct ** 2 * dinv_ct
    weight = imp / dist ** 2                               # :317
    dweight = dimp / dist ** 2 - 2 * imp * ddist / dist ** 3
    return types.SimpleNamespace(ref=ref, inside=inside, valid=valid, uv=uv, weight=weight, s_crop=sc, duv=duv, dweight=dweight)


def _unhom_back(h, g):
    """reverse of q = h[:k] / h[3] (k rows of g): the cotangent of the homogeneous [4, n] vector"""
    out = np.zeros_like(h)
    k = g.shape[0]
    out[:k] = g / h[3]
    out[3] = -(g * h[:k]).sum(0) / h[3] ** 2
    return out


def _fov_back(s, gC, pre, dt):
    """reverse of C = pre P(fov): dL/dfov from dL/dC (cot(x)' = -1 / sin(x)^2, x = fov pi / 360)"""
    gP = pre.T @ gC
    half = np.deg2rad(dt(s.fov) * dt(0.5))
    return (gP[0, 0] + gP[1, 1]) * (-dt(np.pi / 360) / np.sin(half) ** 2)


def rays_adjoint(s, pos, grad_o, grad_d, dt=np.float64):
    """(grad_to_world [12], grad_fov): the reverse sweep through the steps of rays(), written on its own (it shares the
    forward quantities with rays() and nothing of its tangent)"""
    pos, go, gd = np.asarray(pos, dt), np.asarray(grad_o, dt), np.asarray(grad_d, dt)
    A = s.to_world[:, :3].astype(dt)
    C, _ = camera_to_sample(s, dt)
    S = np.linalg.inv(C)
    smp = np.stack([(pos[0] - dt(s.crop[0])) / dt(s.crop[2]), (pos[1] - dt(s.crop[1])) / dt(s.crop[3]), np.zeros_like(pos[0])])
    smp4 = np.concatenate([smp, np.ones((1, smp.shape[1]), dt)])
    h = S @ smp4
    near_p = h[:3] / h[3]
    if s.type == ORTHOGRAPHIC:       # o = A near_p + c, d = z / |z| with z = A e_z
        gA = go @ near_p.T
        z = A[:, 2]
        d, gs = z / np.linalg.norm(z), gd.sum(1)
        gA[:, 2] += (gs - d * (d @ gs)) / np.linalg.norm(z)
        return np.concatenate([gA, go.sum(1)[:, None]], axis=1).reshape(-1), dt(0)
    ln = np.linalg.norm(near_p, axis=0)
    dl = near_p / ln
    d = A @ dl
    inv_z = dt(1) / dl[2]
    near_t = dt(s.near) * inv_z
    g_d = gd + go * near_t                                  # o = c + d near_t
    g_inv_z = dt(s.near) * (go * d).sum(0)
    gA = g_d @ dl.T                                         # d = A dl
    g_dl = A.T @ g_d
    g_dl[2] += -g_inv_z * inv_z ** 2                        # inv_z = 1 / dl.z
    g_near_p = (g_dl - dl * (dl * g_dl).sum(0)) / ln        # dl = near_p / |near_p|
    gS = _unhom_back(h, g_near_p) @ smp4.T                  # h = S smp4
    gC = -S.T @ gS @ S.T                                    # S = C^-1
    return np.concatenate([gA, go.sum(1)[:, None]], axis=1).reshape(-1), _fov_back(s, gC, _pre(s, dt), dt)


def project_adjoint(s, p, active, grad_uv, grad_weight, dt=np.float64):
    """(grad_p [3, n], grad_to_world [12], grad_fov): the reverse sweep through the steps of project(), written on its own;
    uv counts where inside, weight where valid"""
    r = project(s, p, active, dt)
    p = np.asarray(p, dt)
    n = p.shape[1]
    guv, gw = (np.asarray(grad_uv, dt) * r.inside), (np.asarray(grad_weight, dt) * r.valid)
    T = np.eye(4, dtype=dt)
    T[:3] = s.to_world.astype(dt)
    Ti = np.linalg.inv(T)
    p4 = np.concatenate([p, np.ones((1, n), dt)])
    ref4 = Ti @ p4
    ref = ref4[:3]
    C, _ = camera_to_sample(s, dt)
    S = np.linalg.inv(C)
    h = C @ ref4
    dist = np.linalg.norm(ref, axis=0)
    local = ref / dist
    norm, _ = _image_rect(S, np.zeros_like(S))
    inv_ct = 1 / local[2]
    imp = norm * inv_ct ** 3
    # weight = imp / dist^2, imp = norm inv_ct^3, inv_ct = 1 / local.z, local = ref / dist, dist = |ref|
    g_imp = gw / dist ** 2
    g_dist = -2 * gw * imp / dist ** 3
    g_norm = (g_imp * inv_ct ** 3).sum()
    g_local_z = -(3 * norm * inv_ct ** 2 * g_imp) / local[2] ** 2
    g_ref = np.zeros_like(ref)
    g_ref[2] = g_local_z / dist
    g_dist = g_dist - g_local_z * ref[2] / dist ** 2
    g_ref += g_dist * ref / dist
    # uv = sc size + off, sc = h[:2] / h[3], h = C ref4
    size = np.array(s.crop[2:], dt)[:, None]
    g_h = _unhom_back(h, guv * size)
    gC = g_h @ ref4.T
    g_ref4 = C.T @ g_h
    g_ref4[:3] += g_ref
    # norm = 1 / |vol| of the image rectangle, from S = C^-1 (perspective.cpp:185-191)
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
    gS = _unhom_back(h2, g_q) @ e.T
    gC = gC - S.T @ gS @ S.T
    # ref4 = T^-1 p4
    gT = -Ti.T @ (g_ref4 @ p4.T) @ Ti.T
    return (Ti.T @ g_ref4)[:3], gT[:3].reshape(-1), _fov_back(s, gC, _pre(s, dt), dt)


# ---- the header's closed forms, for the CPU test to hold against the matrices ----
def closed_w(s, pos):
    a = s.film[0] / s.film[1]
    return 1.0 - 2.0 * (pos[0] / s.film[0]), (1.0 - 2.0 * (pos[1] / s.film[1])) / a


def closed_rays(s, pos):
    A, c = s.to_world[:, :3], s.to_world[:, 3]
    wx, wy = closed_w(s, pos)
    if s.type == ORTHOGRAPHIC:
        return ortho_closed(s, pos)
    tau = np.tan(s.fov * np.pi / 360.0)
    v = np.stack([wx * tau, wy * tau, np.ones_like(wx)])
    ln = np.linalg.norm(v, axis=0)
    return c[:, None] + s.near * (A @ v), A @ (v / ln), (s.far - s.near) * ln


def ortho_closed(s, pos):
    """workload.ortho_rays' expression in its operation order: tw[k, 0] cx + tw[k, 1] cy + tw[k, 2] near + tw[k, 3]"""
    tw = s.to_world
    cx, cy = closed_w(s, pos)
    o = np.stack([tw[k, 0] * cx + tw[k, 1] * cy + tw[k, 2] * s.near + tw[k, 3] for k in range(3)])
    d = tw[:, 2] / np.linalg.norm(tw[:, 2])
    n = pos.shape[1]
    return o, np.repeat(d[:, None], n, 1), np.full(n, s.far - s.near)


def closed_project(s, p):
    """(uv, weight) of the header: uv = g film_size, weight = |ref| / (A' ref.z^3)"""
    A, c = s.to_world[:, :3], s.to_world[:, 3]
    ref = np.linalg.solve(A, p - c[:, None])
    tau, a = np.tan(s.fov * np.pi / 360.0), s.film[0] / s.film[1]
    uv = np.stack([0.5 * (1 - ref[0] / (ref[2] * tau)) * s.film[0], 0.5 * (1 - a * ref[1] / (ref[2] * tau)) * s.film[1]])
    area = (2 * tau) ** 2 / a * (s.crop[2] * s.crop[3]) / (s.film[0] * s.film[1])
    return uv, np.linalg.norm(ref, axis=0) / (area * ref[2] ** 3)


# ---- the scenes of tests/test_gpu_sensor.py and scripts/sensor_f32_error.py ----
FILM, CROP, FOV = (13, 7), (3, 2, 5, 4), 38.0
POSE = look_at((1.2, -0.9, 1.4), (0.1, 0.05, 0.2), (0.0, 0.0, 1.0))
ORTHO_POSE = POSE @ np.diag([0.9, 0.7, 1.0, 1.0])
SPPS, SEED = (1, 3, 4), 3
PROJECT_CLIP = (0.05, 50.0)     # the clip range of the projection scenes: points on both sides of both planes


def scene(type_, crop, **kw):
    return sensor(type_, ORTHO_POSE if type_ == ORTHOGRAPHIC else POSE, None if type_ == ORTHOGRAPHIC else FOV, FILM, crop, **kw)


def wavefront(s, spp, seed=SEED):
    """(ids, pos) of the whole wavefront of the crop window"""
    ids = np.arange(s.crop[2] * s.crop[3] * spp, dtype=np.uint64)
    return ids, film_positions(s, ids, spp, seed)


def directions(seed=11):
    """a tangent (d_to_world [12], d_fov), float32 values"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(12) * 0.3).astype(np.float32), np.float32(0.7)


def cotangents(n, seed=12):
    """(grad_o, grad_d) [3, n], float32 values"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3, n)).astype(np.float32), rng.standard_normal((3, n)).astype(np.float32)


def project_points(s, n=360, seed=13):
    """(p [3, n] float32, active [n] bool): world points built so that no mask is decided by rounding -- s_crop drawn in
    [0.02, 0.98]^2 or at least 0.02 outside on one axis, the depth in [1.05 near, 0.95 far] or outside by the same factor --
    with every combination present.  (The rounding of p to float32 moves s_crop by 1e-6 at most.)"""
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
    wx, wy = closed_w(s, pos)
    tau = np.tan(s.fov * np.pi / 360.0)
    ref = np.stack([wx * tau, wy * tau, np.ones(n)]) * z
    p = (s.to_world[:, :3] @ ref + s.to_world[:, 3:4]).astype(np.float32)
    return p, rng.random(n) < 0.9


def project_cotangents(weight, seed=14):
    """(grad_uv [2, n], grad_weight [n]) float32; grad_weight is drawn relative to the weight (which spans nine decades
    over the clip range), so that every lane's term is of order one"""
    rng = np.random.default_rng(seed)
    n = weight.shape[0]
    return rng.standard_normal((2, n)).astype(np.float32), (rng.standard_normal(n) / weight).astype(np.float32)


# ---- the error measures the float32 table and the GPU test share ----
def err_abs(got, ref):
    """the largest difference over max(1, the largest |ref|)"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def err_l2(got, ref):
    """the L2 norm of the difference over the L2 norm of ref"""
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / np.linalg.norm(ref))


def ray_derivative_errors(s, spp, rays_t, rays_a):
    """the errors of a tangent (do, dd) = rays_t and an adjoint (grad_to_world, grad_fov) = rays_a of the scene (s, spp)
    under directions() and cotangents(), against the float64 restatement"""
    ids, pos = wavefront(s, spp)
    dtw, dfov = directions()
    go, gd = cotangents(len(ids))
    _, _, _, do, dd = rays(s, pos, np.float64, dtw, dfov)
    g12, gf = rays_adjoint(s, pos, go, gd)
    return {"tangent_do": err_abs(rays_t[0], do), "tangent_dd": err_abs(rays_t[1], dd),
            "adjoint": err_l2(np.append(rays_a[0], rays_a[1]), np.append(g12, gf))}


def project_errors(s, p, active, got, ref):
    """got, ref: namespaces with uv, weight, duv, dweight, grad_p, grad13 (ref also inside, valid)"""
    i, v = ref.inside, ref.valid
    return {"project_uv": float(np.abs(got.uv - ref.uv)[:, i].max()),
            "project_weight": float(np.abs(got.weight / ref.weight - 1)[v].max()),
            "project_duv": err_abs(got.duv[:, i], ref.duv[:, i]),
            "project_dweight": float((np.abs(got.dweight - ref.dweight) / ref.weight)[v].max()),
            "project_grad_p": err_l2(got.grad_p, ref.grad_p), "project_adjoint": err_l2(got.grad13, ref.grad13)}


def project_case(s, dt=np.float64):
    """the projection scene of s evaluated by the restatement in dt: (p, active, namespace as project_errors takes it)"""
    p, active = project_points(s)
    dtw, dfov = directions()
    dp = np.random.default_rng(15).standard_normal(p.shape).astype(np.float32) * np.float32(0.2)
    r = project(s, p, active, dt, dp, dtw, dfov)
    guv, gw = project_cotangents(project(s, p, active).weight)
    gp, g12, gf = project_adjoint(s, p, active, guv, gw, dt)
    r.grad_p, r.grad13, r.dp, r.guv, r.gw = gp, np.append(g12, gf), dp, guv, gw
    return p, active, r

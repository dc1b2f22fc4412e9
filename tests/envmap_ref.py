"""Float64 restatement of the environment-map row of include/hf.h (hf_envmap_*): the sampling table, the draw, eval, the
value, its adjoint and its tangent.  The draw is float32 where the header says so (it must reproduce the device's cell
and fractions bit for bit when it is fed the DEVICE's table); everything after the draw is float64.  Visibility is an
input (a [K, n] bit array): nothing here traces.  Uses sky_ref's sample stream and nothing of the product."""
import numpy as np

import sky_ref as S

F = np.float32
ONE_BELOW = F(1.0 - 2.0 ** -24)
DEFAULT_ROT = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # the map's +Y -> world +Z


def with_seam(data0):
    """[H, W0] -> [H, W0 + 1]: the seam column, a copy of column 0 (envmap.cpp:147, 249-258)"""
    data0 = np.asarray(data0)
    return np.concatenate([data0, data0[:, :1]], 1)


def row_sin(H):
    """float32 [H - 1]: sin(pi (cy + 1/2) / (H - 1)), evaluated in double and rounded once"""
    return np.sin(np.pi * ((np.arange(H - 1) + 0.5) / (H - 1))).astype(F)


def cell_mean(data):
    """float32 [H - 1, W - 1]: m_c = 0.25 ((p00 + p10) + (p01 + p11)), p = max(texel, 0), float32 in this association"""
    p = np.maximum(np.asarray(data, F), F(0))
    return F(0.25) * ((p[:-1, :-1] + p[:-1, 1:]) + (p[1:, :-1] + p[1:, 1:]))


def mbar_of(data):
    """float32: the fp64 sum in row order of the rows' float32-rounded fp64 sums of m_c, over the cell count"""
    mc = cell_mean(data)
    rows = np.cumsum(mc.astype(np.float64), axis=1)[:, -1].astype(F)
    return F(np.cumsum(rows.astype(np.float64))[-1] / (mc.shape[0] * mc.shape[1]))


def cell_weight(data, u, mbar):
    """float32 [H - 1, W - 1]: weight_c = s ((1 - u) m_c + u mbar), one rounding per operation"""
    u = F(u)
    return row_sin(np.asarray(data).shape[0])[:, None] * ((F(1) - u) * cell_mean(data) + u * F(mbar))


def build_table(data, u):
    """the table as the header of include/hf.h defines it: float32 [4 + (H - 1) + (H - 1)(W - 1)]"""
    data = np.asarray(data, F)
    mbar = mbar_of(data)
    w = cell_weight(data, u, mbar)
    C = np.cumsum(w.astype(np.float64), axis=1).astype(F)            # (numpy's cumsum adds in order)
    M = np.cumsum(C[:, -1].astype(np.float64)).astype(F)
    return np.concatenate([np.array([M[-1], mbar, F(u), 0], F), M, C.ravel()])


def split_table(table, W, H):
    """(Sigma, mbar, u, M [H - 1], C [H - 1, W - 1]) of a table"""
    t = np.asarray(table, F)
    assert t.shape == (4 + (H - 1) + (H - 1) * (W - 1),)
    return t[0], t[1], t[2], t[4:4 + H - 1], t[4 + H - 1:].reshape(H - 1, W - 1)


def draw(data, table, sx, sy):
    """the draw of include/hf.h in float32 from a given table: (cx, cy, fx, fy, weight_c, valid)"""
    data = np.asarray(data, F)
    H, W = data.shape
    sigma, mbar, u, M, C = split_table(table, W, H)
    sx = np.asarray(sx, F); sy = np.asarray(sy, F)
    with np.errstate(all="ignore"):
        y = sy * sigma
        cy = np.minimum(np.searchsorted(M, y, side="left"), H - 2)        # the first row with !(M[cy] < y)
        rowsum = C[cy, W - 2]
        ylo = np.where(cy > 0, M[np.maximum(cy, 1) - 1], F(0)).astype(F)
        fy = np.minimum(np.maximum((y - ylo) / rowsum, F(0)), ONE_BELOW)
        x = sx * rowsum
        cx = np.empty_like(cy)
        for r in np.unique(cy):
            at = cy == r
            cx[at] = np.minimum(np.searchsorted(C[r], x[at], side="left"), W - 2)
        xlo = np.where(cx > 0, C[cy, np.maximum(cx, 1) - 1], F(0)).astype(F)
        wc = cell_weight(data, u, mbar)[cy, cx]
        fx = np.minimum(np.maximum((x - xlo) / wc, F(0)), ONE_BELOW)
    valid = (sigma > 0) & (wc > 0)
    return cx, cy, fx.astype(F), fy.astype(F), wc, valid


def bilinear_weights(fx, fy):
    fx = np.asarray(fx, np.float64); fy = np.asarray(fy, np.float64)
    return np.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx])


def corners(W, cx, cy):
    """[4, n] flat texel indices (v00, v10, v01, v11) of the cells"""
    r0 = cy * W + cx
    return np.stack([r0, r0 + 1, r0 + W, r0 + W + 1])


def shade(data, table, cx, cy, fx, fy, wc, valid, rot=None):
    """float64, per draw: world direction [3, n], L, G = 1 / pdf_omega (0 for an invalid draw), sin theta"""
    data = np.asarray(data, np.float64)
    H, W = data.shape
    sigma = float(np.asarray(table, F)[0])
    ux = (cx + (fx.astype(np.float64) + 0.5)) / (W - 1); uy = (cy + fy.astype(np.float64)) / (H - 1)
    th, ph = np.pi * uy, 2.0 * np.pi * ux
    local = np.stack([np.sin(th) * np.sin(ph), np.cos(th), -np.sin(th) * np.cos(ph)])
    R = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    b = bilinear_weights(fx, fy)
    L = (b * data.ravel()[corners(W, cx, cy)]).sum(0)
    with np.errstate(all="ignore"):
        G = np.where(valid, 2.0 * np.pi ** 2 * np.sin(th) * sigma / (wc.astype(np.float64) * (W - 1) * (H - 1)), 0.0)
    return R @ local, L, G, np.sin(th)


def draws(data, table, ids, K, seed, rot=None):
    """the K draws of every sample: a dict of [K, ...] arrays (w [K, 3, n], L, G, valid, idx [K, 4, n], b [K, 4, n])"""
    data = np.asarray(data, F)
    out = {k: [] for k in ("w", "L", "G", "valid", "idx", "b")}
    for k in range(K):
        sx, sy = S.samples(ids, k, seed)
        cx, cy, fx, fy, wc, valid = draw(data, table, sx, sy)
        w, L, G, _ = shade(data, table, cx, cy, fx, fy, wc, valid, rot)
        for key, v in (("w", w), ("L", L), ("G", G), ("valid", valid), ("idx", corners(data.shape[1], cx, cy)),
                       ("b", bilinear_weights(fx, fy))):
            out[key].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def traced(sh_n, d, t, dr):
    """[K, n]: eligible, valid and <sh_n, w_k> > 0; and the margins |<sh_n, w_k>|"""
    el, _ = S.eligible(sh_n, d, t)
    co = np.einsum("cn,kcn->kn", np.asarray(sh_n, np.float64), dr["w"])
    return el[None] & dr["valid"] & (co > 0), np.abs(co)


def _terms(sh_n, d, t, bits, dr):
    """b [K, n] (bits of eligible samples), co = <sh_n, w_k> [K, n]"""
    el, _ = S.eligible(sh_n, d, t)
    b = np.asarray(bits, bool) & el[None] & dr["valid"]
    return b, np.einsum("cn,kcn->kn", np.asarray(sh_n, np.float64), dr["w"])


def forward(sh_n, d, t, weight, bits, dr, albedo, spp, data=None):
    """(image [n / spp], per-sample values [n], S = the largest sum_k |term| of any sample); data: texels that replace
    the draws' L (the distribution stays the table's)"""
    K = dr["w"].shape[0]
    b, co = _terms(sh_n, d, t, bits, dr)
    L = dr["L"] if data is None else (dr["b"] * np.asarray(data, np.float64).ravel()[dr["idx"]]).sum(1)
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    terms = b * co * L * dr["G"]
    c = albedo / (np.pi * K)
    value = wgt * c * terms.sum(0)
    return value.reshape(-1, spp).mean(1), value, float((np.abs(wgt * c) * np.abs(terms).sum(0)).max())


def adjoint(sh_n, d, t, weight, bits, dr, albedo, spp, grad_image, shape):
    """(grad_sh_n [3, n], grad_weight [n], grad_data [H, W], per texel: the number of contributions and sum |terms|)"""
    K = dr["w"].shape[0]
    b, co = _terms(sh_n, d, t, bits, dr)
    g = np.repeat(np.asarray(grad_image, np.float64), spp) / spp
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    c = albedo / (np.pi * K)
    E = dr["L"] * dr["G"]
    gn = (g * wgt * c)[None] * ((b * E)[:, None, :] * dr["w"]).sum(0)
    gw = g * c * (b * co * E).sum(0)
    q = (g * wgt * c)[None] * b * co * dr["G"]                              # [K, n]
    contrib = q[:, None, :] * dr["b"]                                       # [K, 4, n]
    on = np.broadcast_to(b[:, None, :], contrib.shape)
    gd = np.zeros(shape[0] * shape[1]); cnt = np.zeros(gd.shape, np.int64); ab = np.zeros(gd.shape)
    np.add.at(gd, dr["idx"][on], contrib[on])
    np.add.at(cnt, dr["idx"][on], 1)
    np.add.at(ab, dr["idx"][on], np.abs(contrib[on]))
    return gn, gw, gd.reshape(shape), cnt.reshape(shape), ab.reshape(shape)


def adjoint_scales(sh_n, d, t, weight, bits, dr, albedo, spp, grad_image):
    """the largest sum_k |term| of any sample's grad_sh_n (per component, |w_k| <= 1) and grad_weight"""
    K = dr["w"].shape[0]
    b, co = _terms(sh_n, d, t, bits, dr)
    g = np.abs(np.repeat(np.asarray(grad_image, np.float64), spp)) / spp
    wgt = 1.0 if weight is None else np.abs(np.asarray(weight, np.float64))
    c = albedo / (np.pi * K)
    E = np.abs(dr["L"] * dr["G"])
    return float((g * wgt * c * (b * E).sum(0)).max()), float((g * c * (b * np.abs(co) * E).sum(0)).max())


def tangent(sh_n, d, t, weight, bits, dr, albedo, spp, dsh_n=None, dweight=None, ddata=None, return_scale=False):
    """dimage [n / spp] for tangents dsh_n [3, n], dweight [n] and ddata [H, W] (None: zero); return_scale: also the
    largest sum |term| of any sample"""
    K = dr["w"].shape[0]
    b, co = _terms(sh_n, d, t, bits, dr)
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    E = dr["L"] * dr["G"]
    dv = np.zeros(co.shape[1]); ab = np.zeros(co.shape[1])
    if dsh_n is not None:
        x = wgt * (b * E * np.einsum("cn,kcn->kn", np.asarray(dsh_n, np.float64), dr["w"]))
        dv = dv + x.sum(0); ab = ab + np.abs(x).sum(0)
    if dweight is not None:
        x = np.asarray(dweight, np.float64) * (b * co * E)
        dv = dv + x.sum(0); ab = ab + np.abs(x).sum(0)
    if ddata is not None:
        dL = dr["b"] * np.asarray(ddata, np.float64).ravel()[dr["idx"]]              # [K, 4, n]
        x = (wgt * (b * co * dr["G"]))[:, None, :] * dL
        dv = dv + x.sum((0, 1)); ab = ab + np.abs(x).sum((0, 1))
    c = albedo / (np.pi * K)
    out = (c * dv).reshape(-1, spp).mean(1)
    return (out, float(c * ab.max())) if return_scale else out


def lookup(d, W, H, rot=None):
    """Emitter::eval's map coordinates of world directions d [3, n] (envmap.cpp:323-333, 498-509), float64:
    (cx, cy, fx, fy)"""
    R = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    v = R.T @ np.asarray(d, np.float64)
    ux = np.arctan2(v[0], -v[2]) / (2.0 * np.pi) - 0.5 / (W - 1)
    uy = np.arccos(np.clip(v[1], -1.0, 1.0)) / np.pi
    ux = (ux - np.floor(ux)) * (W - 1); uy = (uy - np.floor(uy)) * (H - 1)
    cx = np.minimum(ux.astype(np.int64), W - 2); cy = np.minimum(uy.astype(np.int64), H - 2)
    return cx, cy, ux - cx, uy - cy


def eval_map(data, d, rot=None, active=None):
    data = np.asarray(data, np.float64)
    H, W = data.shape
    cx, cy, fx, fy = lookup(d, W, H, rot)
    v = (bilinear_weights(fx, fy) * data.ravel()[corners(W, cx, cy)]).sum(0)
    return v if active is None else np.where(active, v, 0.0)


def eval_adjoint(d, shape, grad_out, rot=None, active=None):
    """(grad_data [H, W], per texel: the number of contributions and sum |terms|)"""
    H, W = shape
    cx, cy, fx, fy = lookup(d, W, H, rot)
    on = np.ones(len(cx), bool) if active is None else np.asarray(active, bool)
    contrib = (np.asarray(grad_out, np.float64)[None] * bilinear_weights(fx, fy))[:, on]
    idx = corners(W, cx, cy)[:, on]
    gd = np.zeros(H * W); cnt = np.zeros(H * W, np.int64); ab = np.zeros(H * W)
    np.add.at(gd, idx, contrib); np.add.at(cnt, idx, 1); np.add.at(ab, idx, np.abs(contrib))
    return gd.reshape(shape), cnt.reshape(shape), ab.reshape(shape)


def pdf_direction(data, table, d, rot=None):
    """pdf_omega of world directions: weight_c (W - 1)(H - 1) / Sigma / (2 pi^2 sin theta) of the cell they fall in"""
    data = np.asarray(data, F)
    H, W = data.shape
    sigma, mbar, u, _, _ = split_table(table, W, H)
    cx, cy, fx, fy = lookup(d, W, H, rot)
    wc = cell_weight(data, u, mbar)[cy, cx].astype(np.float64)
    st = np.sin(np.pi * (cy + fy) / (H - 1))
    with np.errstate(all="ignore"):
        return np.where((sigma > 0) & (wc > 0), wc * (W - 1) * (H - 1) / float(sigma) / (2.0 * np.pi ** 2 * st), 0.0)


# ---- the maps of the tests (seam column = column 0) ------------------------------------------------------------------
def _angles(W0, H):
    th = np.pi * np.arange(H) / (H - 1)
    ph = 2.0 * np.pi * (np.arange(W0) + 0.5) / W0
    return th[:, None], ph[None, :]


def map_sun(W=17, H=9):
    """0.2 + 0.8 cos theta down to the horizon row (theta = pi / 2: 0.2), exactly 0 below, one texel of 50: zero-weight
    cells and a 250 : 1 range"""
    th, ph = _angles(W - 1, H)
    m = np.where(np.cos(th) > -1e-9, 0.2 + 0.8 * np.maximum(np.cos(th), 0.0), 0.0) * np.ones_like(ph)
    m[H // 4, W // 3] = 50.0
    return with_seam(m).astype(F)


def map_gradient(W=9, H=5):
    """0.6 + 0.4 cos phi sin theta + 0.3 cos theta: positive everywhere"""
    th, ph = _angles(W - 1, H)
    return with_seam(0.6 + 0.4 * np.cos(ph) * np.sin(th) + 0.3 * np.cos(th)).astype(F)


def map_2x2():
    return with_seam(np.array([[0.7], [0.4]])).astype(F)


MAPS = {"sun": map_sun, "gradient": map_gradient, "2x2": map_2x2}

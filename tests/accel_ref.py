"""The contract of the traversal's acceleration data, stated as data: the min/max pyramid and the per-node records
(csrc/hf_device.h: hf_dev_field, "Sheared bounds"; csrc/hf_kernels.hip: hf_shear_kernel and the comment below it).
Plain numpy, float64, written from those comments -- nothing here calls the library.

  check_level    raises AccelError on the first violation of A-F below at one level, returns the largest margins seen
  emulate_build  a float32 transcription of the documented build (records to check where there is no GPU)

Layout.  top = max(ceil(log2(max(W-1, H-1))), 1).  Level L (1..top) is stored padded: side x side slots, side =
2^(top - L), row-major by (iy, ix); node (ix, iy) covers the cells [ix 2^L, (ix+1) 2^L) x [iy 2^L, (iy+1) 2^L), of which
only those with x <= W-2 and y <= H-2 exist.  A record is 12 floats (a, b, c, f, lo0, hi0, lo1, hi1, lo2, hi2, lo3, hi3),
child j = 2 jy + jx the quadrant of S = 2^(L-1) cells a side at (x0 + jx S, y0 + jy S).

  A  absence      a pyramid slot without an existing cell is exactly (+inf, -inf); child j is absent iff its first cell
                  lies beyond the grid, an absent child is exactly (+inf, -inf), an existing one finite with lo <= hi
  B  pyramid      an existing slot holds bitwise the min and max of z = fl32(h s) over the vertices of its existing cells
  C  min/max      levels above SHEAR_TOP: (a, b, c) are exact zeros and the child ranges are bitwise the four pyramid
                  slots of the level below
  D  containment  levels up to SHEAR_TOP: with w = z - (c + a (x - xc) + b (y - yc)) in float64 from the stored plane,
                  lo_j - slack <= w <= hi_j + slack for every vertex of every existing cell of child j
  E  tightness    hi_j <= w_max + 2 eps_ref + slack and lo_j >= w_min - 2 eps_ref - slack
  F  slope factor f is bitwise fl32((|a| + |b|) + 2 max(max_j(hi_j - lo_j), 0)), from the record's own entries
"""
import numpy as np

SHEAR_TOP = 5          # HF_SHEAR_TOP (hf_device.h): levels 1..5 carry a fitted plane, the levels above the zero plane
F32 = np.float32
INF = F32(np.inf)

# The tolerances of D and E.
#
# The kernels evaluate, in float32, w = z - fma(a, x - xc, fma(b, y - yc, c)) and widen the extremes by
#   eps = 1e-6 (|c| + (|a| + |b|) size),   size = 2^L.
# eps covers the rounding of the plane evaluation: two fmas, each rounded once relative to a value bounded by
# |c| + (|a| + |b|) size, together at most 2^-23 of that magnitude = 0.12 eps.  It does NOT scale with the rounding of
# the final subtraction where |z| is much larger than the plane value: that subtraction rounds relative to |w| <= |z| +
# |plane|, i.e. by at most 2^-24 |z| + 0.06 eps, and the addition of eps to the extreme rounds once more by at most
# 2^-24 (|z| + |plane| + eps).  Per vertex that leaves 2^-23 |z| = one float32 rounding of z (SLACK |z|) uncovered by
# eps; everything else sums to less than 0.3 eps.  Hence
#   containment:  hi >= w - slack    (eps added, less than 0.3 eps + slack lost),
#   tightness:    hi <= w_max + 2 eps_ref + slack   (one eps is added by the kernel, less than one is its rounding; the
#                 slack is that of the vertex attaining w_max: another vertex v' can only round above it by
#                 slack' - slack <= 2^-23 (|plane' - plane| + (w_max - w')) < 0.24 eps + (w_max - w')),
# and the same with the signs turned for lo.  eps_ref is the kernel's formula in float64 from the stored plane.
SLACK = 2.0 ** -23
EPS_REL = 1e-6


class AccelError(AssertionError):
    """a violation of the contract; .check is the letter A-F"""

    def __init__(self, check, msg):
        super().__init__(f"check {check}: {msg}")
        self.check = check


def num_levels(W, H):
    top = 0
    while (1 << top) < W - 1 or (1 << top) < H - 1:
        top += 1
    return max(top, 1)


def scaled_heights(h, s):
    """z = fl32(h) * fl32(s) in float32: the product every kernel forms"""
    return np.asarray(h, F32) * F32(s)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _first(mask):
    """index tuple of the first True of a mask"""
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(mask)), mask.shape))


def block_minmax(z, B, ny, nx):
    """(min, max) of z[H, W] over the vertex blocks [iy B, min((iy+1) B, H-1)] x [ix B, min((ix+1) B, W-1)] of the first
    ny x nx nodes of B cells a side (all of which must have an existing cell): segment reductions along each axis, plus
    the shared vertex at the far edge of each block"""
    H, W = z.shape
    xs, ys = np.arange(nx) * B, np.arange(ny) * B
    assert xs[-1] <= W - 2 and ys[-1] <= H - 2
    xe, ye = np.minimum(xs + B, W - 1), np.minimum(ys + B, H - 1)
    out = []
    for red in (np.minimum, np.maximum):
        r = red(red.reduceat(z, xs, axis=1), z[:, xe])
        out.append(red(red.reduceat(r, ys, axis=0), r[ye, :]))
    return out[0], out[1]


def _child_exists(W, H, level, ny, nx):
    """[ny, nx, 4]: child j of node (ix, iy) has at least one existing cell"""
    size, S = 1 << level, 1 << (level - 1)
    x0 = (np.arange(nx) * size)[None, :, None]
    y0 = (np.arange(ny) * size)[:, None, None]
    j = np.arange(4)[None, None, :]
    return (x0 + (j & 1) * S <= W - 2) & (y0 + (j >> 1) * S <= H - 2)


def child_bounds(z32, W, H, level, rec, ny, nx):
    """For the stored planes rec[ny, nx, 12] of the first ny x nx nodes of a fitted level, per (node, child), all float64:
    w_min, w_max (exact extremes of z - plane over the child's vertices), the slack at the vertex attaining each, the
    extremes of w + slack and w - slack over the vertices (what containment compares with lo and hi), eps_ref [ny, nx], the
    per-vertex arrays (w, slack, valid) [ny, nx, 4, S+1, S+1] and the existence mask."""
    size, S = 1 << level, 1 << (level - 1)
    z = z32.astype(np.float64)
    a, b, c = (rec[..., k].astype(np.float64) for k in range(3))
    eps = EPS_REL * (np.abs(c) + (np.abs(a) + np.abs(b)) * size)
    x0 = (np.arange(nx) * size)[None, :, None, None, None]
    y0 = (np.arange(ny) * size)[:, None, None, None, None]
    j = np.arange(4)[None, None, :, None, None]
    d = np.arange(S + 1)
    X = x0 + (j & 1) * S + d[None, None, None, None, :]
    Y = y0 + (j >> 1) * S + d[None, None, None, :, None]
    exists = _child_exists(W, H, level, ny, nx)
    valid = exists[..., None, None] & (X <= W - 1) & (Y <= H - 1)
    zc = z[np.minimum(Y, H - 1), np.minimum(X, W - 1)]
    e = (Ellipsis, None, None, None)
    w = zc - (c[e] + a[e] * (X - (x0 + S)) + b[e] * (Y - (y0 + S)))
    slack = SLACK * np.abs(zc)
    flat = (ny, nx, 4, (S + 1) * (S + 1))
    w_hi = np.where(valid, w, -np.inf).reshape(flat)
    w_lo = np.where(valid, w, np.inf).reshape(flat)
    k_hi, k_lo = w_hi.argmax(-1)[..., None], w_lo.argmin(-1)[..., None]
    sl = slack.reshape(flat)
    return dict(w_max=np.take_along_axis(w_hi, k_hi, -1)[..., 0], w_min=np.take_along_axis(w_lo, k_lo, -1)[..., 0],
                slack_max=np.take_along_axis(sl, k_hi, -1)[..., 0], slack_min=np.take_along_axis(sl, k_lo, -1)[..., 0],
                up=np.where(valid, w - slack, -np.inf).max(axis=(3, 4)), dn=np.where(valid, w + slack, np.inf).min(axis=(3, 4)),
                eps=eps, w=w, slack=slack, valid=valid, exists=exists)


def slope_factor(rec):
    """F: fl32((|a| + |b|) + 2 max(max_j(hi_j - lo_j), 0)) in float32 from the record's own entries; an absent child gives
    -inf.  2 r is exact, so a contraction of the last two operations into an fma cannot change the bits."""
    rec = np.asarray(rec, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.maximum((rec[..., 5::2] - rec[..., 4::2]).max(axis=-1), F32(0))
        return ((np.abs(rec[..., 0]) + np.abs(rec[..., 1])) + F32(2) * r).astype(F32)


def check_level(h, s, W, H, top, level, records, minmax, child_minmax=None):
    """Checks A-F at one level.  records [side, side, 12] and minmax [side, side, 2] are the padded level as stored
    (float32), child_minmax the pyramid of level - 1 (needed above SHEAR_TOP).  Raises AccelError with the node, the child
    and the amounts on the first violation.  Returns the largest observed margins:
      'contain'  max (w - hi) / slack and (lo - w) / slack over all vertices (<= 1 passes D; negative: eps to spare)
      'tight'    max (hi - w_max) / eps_ref and (w_min - lo) / eps_ref over all children (E allows 2 + slack / eps_ref)"""
    assert top == num_levels(W, H) and 1 <= level <= top
    rec, mm = np.asarray(records, F32), np.asarray(minmax, F32)
    side, size, S = 1 << (top - level), 1 << level, 1 << (level - 1)
    assert rec.shape == (side, side, 12) and mm.shape == (side, side, 2)
    z32 = scaled_heights(h, s)
    assert z32.shape == (H, W)
    where = f"level {level}"
    nx, ny = -(-(W - 1) // size), -(-(H - 1) // size)          # nodes with an existing cell
    lo, hi = rec[..., 4::2], rec[..., 5::2]

    # ---- A: absence, on every slot of the padded level
    node_exists = np.zeros((side, side), bool)
    node_exists[:ny, :nx] = True
    bad = ~node_exists & ~((mm[..., 0] == INF) & (mm[..., 1] == -INF))
    if bad.any():
        iy, ix = _first(bad)
        raise AccelError("A", f"{where} node ({ix}, {iy}) has no cell but its pyramid slot is {tuple(mm[iy, ix])}, not (+inf, -inf)")
    exists = _child_exists(W, H, level, side, side)
    bad = ~exists & ~((lo == INF) & (hi == -INF))
    if bad.any():
        iy, ix, j = _first(bad)
        raise AccelError("A", f"{where} node ({ix}, {iy}) child {j} is absent but holds ({lo[iy, ix, j]}, {hi[iy, ix, j]})")
    with np.errstate(invalid="ignore"):
        bad = exists & ~(np.isfinite(lo) & np.isfinite(hi) & (lo <= hi))
    if bad.any():
        iy, ix, j = _first(bad)
        raise AccelError("A", f"{where} node ({ix}, {iy}) child {j} exists but holds ({lo[iy, ix, j]}, {hi[iy, ix, j]})")

    # ---- B: the pyramid slot of every existing node, bitwise
    mn, mx = block_minmax(z32, size, ny, nx)
    for name, got, want in (("min", mm[:ny, :nx, 0], mn), ("max", mm[:ny, :nx, 1], mx)):
        bad = _bits(got) != _bits(want)
        if bad.any():
            iy, ix = _first(bad)
            raise AccelError("B", f"{where} node ({ix}, {iy}) pyramid {name} is {got[iy, ix]!r}, the vertices give {want[iy, ix]!r}")

    stats = dict(contain=-np.inf, tight=-np.inf)
    if level > SHEAR_TOP:
        # ---- C: zero plane, the children are the pyramid slots of the level below
        bad = _bits(rec[..., 0:3]) != 0
        if bad.any():
            iy, ix, k = _first(bad)
            raise AccelError("C", f"{where} node ({ix}, {iy}) is a min/max level but plane entry {'abc'[k]} is {rec[iy, ix, k]!r}, not +0")
        cm = np.asarray(child_minmax, F32)
        assert cm.shape == (2 * side, 2 * side, 2), "check C needs the pyramid of the level below"
        kids = cm.reshape(side, 2, side, 2, 2).transpose(0, 2, 1, 3, 4).reshape(side, side, 8)   # [iy, ix, (jy, jx, min/max)]
        bad = _bits(rec[..., 4:12]) != _bits(kids)
        if bad.any():
            iy, ix, k = _first(bad)
            raise AccelError("C", f"{where} node ({ix}, {iy}) child {k >> 1} {'lo' if k % 2 == 0 else 'hi'} is {rec[iy, ix, 4 + k]!r}, "
                                  f"the pyramid slot below holds {kids[iy, ix, k]!r}")
    else:
        bad = ~np.isfinite(rec[..., 0:3])
        if bad.any():
            iy, ix, k = _first(bad)
            raise AccelError("D", f"{where} node ({ix}, {iy}) plane entry {'abc'[k]} is {rec[iy, ix, k]!r}")
        cb = child_bounds(z32, W, H, level, rec[:ny, :nx], ny, nx)
        ex = cb["exists"]
        lo64, hi64 = lo[:ny, :nx].astype(np.float64), hi[:ny, :nx].astype(np.float64)
        # ---- D: containment, per vertex (up = max of w - slack, dn = min of w + slack over the child's vertices)
        bad = ex & (cb["up"] > hi64)
        if bad.any():
            iy, ix, j = _first(bad)
            over = np.where(cb["valid"][iy, ix, j], cb["w"][iy, ix, j] - cb["slack"][iy, ix, j], -np.inf)
            dy, dx = _first(over == over.max())
            raise AccelError("D", f"{where} node ({ix}, {iy}) child {j}: vertex ({ix * size + (j & 1) * S + dx}, {iy * size + (j >> 1) * S + dy}) "
                                  f"has w = {cb['w'][iy, ix, j, dy, dx]!r} above hi = {hi64[iy, ix, j]!r} by more than slack = {cb['slack'][iy, ix, j, dy, dx]:.3e}")
        bad = ex & (cb["dn"] < lo64)
        if bad.any():
            iy, ix, j = _first(bad)
            under = np.where(cb["valid"][iy, ix, j], cb["w"][iy, ix, j] + cb["slack"][iy, ix, j], np.inf)
            dy, dx = _first(under == under.min())
            raise AccelError("D", f"{where} node ({ix}, {iy}) child {j}: vertex ({ix * size + (j & 1) * S + dx}, {iy * size + (j >> 1) * S + dy}) "
                                  f"has w = {cb['w'][iy, ix, j, dy, dx]!r} below lo = {lo64[iy, ix, j]!r} by more than slack = {cb['slack'][iy, ix, j, dy, dx]:.3e}")
        # ---- E: tightness
        eps = cb["eps"][..., None]
        bad = ex & (hi64 > cb["w_max"] + 2 * eps + cb["slack_max"])
        if bad.any():
            iy, ix, j = _first(bad)
            raise AccelError("E", f"{where} node ({ix}, {iy}) child {j}: hi = {hi64[iy, ix, j]!r} is loose, w_max = {cb['w_max'][iy, ix, j]!r}, "
                                  f"eps_ref = {eps[iy, ix, 0]:.3e}, slack = {cb['slack_max'][iy, ix, j]:.3e}")
        bad = ex & (lo64 < cb["w_min"] - 2 * eps - cb["slack_min"])
        if bad.any():
            iy, ix, j = _first(bad)
            raise AccelError("E", f"{where} node ({ix}, {iy}) child {j}: lo = {lo64[iy, ix, j]!r} is loose, w_min = {cb['w_min'][iy, ix, j]!r}, "
                                  f"eps_ref = {eps[iy, ix, 0]:.3e}, slack = {cb['slack_min'][iy, ix, j]:.3e}")
        # the margins that were observed (for the record; nothing is asserted on them)
        v = cb["valid"] & (cb["slack"] > 0)
        if v.any():
            e5 = (Ellipsis, None, None)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.maximum((cb["w"] - hi64[e5]) / cb["slack"], (lo64[e5] - cb["w"]) / cb["slack"])
            stats["contain"] = float(r[v].max())
        v = ex & (eps > 0)
        if v.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.maximum((hi64 - cb["w_max"]) / eps, (cb["w_min"] - lo64) / eps)
            stats["tight"] = float(r[v].max())

    # ---- F: the slope factor, bitwise, on every slot
    want = slope_factor(rec)
    bad = _bits(rec[..., 3]) != _bits(want)
    if bad.any():
        iy, ix = _first(bad)
        raise AccelError("F", f"{where} node ({ix}, {iy}) slope factor is {rec[iy, ix, 3]!r}, its own entries give {want[iy, ix]!r}")
    return stats


# -----------------------------------------------------------------------------------------------------------------
# emulate_build: the documented build in float32 numpy
# -----------------------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 and
    then to float32, which differs from the single rounding of a hardware fma only in rare double-rounding cases -- far
    inside eps, and the emulation claims the contract, not the device's bits"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emulate_build(h, s, W, H):
    """{level: (records [side, side, 12], minmax [side, side, 2])} for levels 1..top, padded as stored.

    Pyramid: level 1 from the vertices of each node's existing cells, then 2x2 reductions; slots without a cell hold
    (+inf, -inf).  Levels 1..SHEAR_TOP: the plane through the node's corner heights, the corners clamped to the grid,
      a = ((z10 - z00) + (z11 - z01)) / (2 size), b = ((z01 - z00) + (z11 - z10)) / (2 size), c = ((z00 + z10) + (z01 + z11)) / 4,
    per existing child the extremes of w = z - fma(a, x - xc, fma(b, y - yc, c)) widened by eps = 1e-6 (|c| + (|a| + |b|) size),
    absent children (+inf, -inf), and the slope factor of check F.  Levels above: the zero plane, the four pyramid slots
    of the level below as child ranges, the same slope factor."""
    z = scaled_heights(h, s)
    assert z.shape == (H, W)
    top = num_levels(W, H)
    out = {}
    # pyramid
    mms = {}
    for level in range(1, top + 1):
        side = 1 << (top - level)
        mm = np.empty((side, side, 2), F32)
        mm[..., 0], mm[..., 1] = INF, -INF
        if level == 1:
            nx, ny = -(-(W - 1) // 2), -(-(H - 1) // 2)
            mm[:ny, :nx, 0], mm[:ny, :nx, 1] = block_minmax(z, 2, ny, nx)
        else:
            c = mms[level - 1].reshape(side, 2, side, 2, 2)
            mm[..., 0], mm[..., 1] = c[..., 0].min(axis=(1, 3)), c[..., 1].max(axis=(1, 3))
        mms[level] = mm
    for level in range(1, top + 1):
        side, size, S = 1 << (top - level), 1 << level, 1 << (level - 1)
        rec = np.zeros((side, side, 12), F32)
        if level > SHEAR_TOP:
            c = mms[level - 1].reshape(side, 2, side, 2, 2).transpose(0, 2, 1, 3, 4)
            rec[..., 4:12] = c.reshape(side, side, 8)
        else:
            x0, y0 = (np.arange(side) * size)[None, :], (np.arange(side) * size)[:, None]
            xa, xb = np.minimum(x0, W - 1), np.minimum(x0 + size, W - 1)
            ya, yb = np.minimum(y0, H - 1), np.minimum(y0 + size, H - 1)
            z00, z10, z01, z11 = z[ya, xa], z[ya, xb], z[yb, xa], z[yb, xb]
            inv = F32(0.5) / F32(size)
            a = ((z10 - z00) + (z11 - z01)) * inv
            b = ((z01 - z00) + (z11 - z10)) * inv
            c = F32(0.25) * ((z00 + z10) + (z01 + z11))
            xc, yc = (x0 + S).astype(F32), (y0 + S).astype(F32)
            eps = F32(EPS_REL) * (np.abs(c) + (np.abs(a) + np.abs(b)) * F32(size))
            rec[..., 0], rec[..., 1], rec[..., 2] = a, b, c
            for j in range(4):
                cj0, ci0 = x0 + (j & 1) * S, y0 + (j >> 1) * S
                exists = (cj0 <= W - 2) & (ci0 <= H - 2)
                lo = np.full((side, side), INF, F32)
                hi = np.full((side, side), -INF, F32)
                for di in range(S + 1):
                    i = ci0 + di
                    row = _fma32(b, i.astype(F32) - yc, c)
                    for dj in range(S + 1):
                        jj = cj0 + dj
                        ok = exists & (i <= H - 1) & (jj <= W - 1)
                        w = z[np.minimum(i, H - 1), np.minimum(jj, W - 1)] - _fma32(a, jj.astype(F32) - xc, row)
                        lo = np.where(ok, np.minimum(lo, w), lo)
                        hi = np.where(ok, np.maximum(hi, w), hi)
                rec[..., 4 + 2 * j] = np.where(exists, lo - eps, INF)
                rec[..., 5 + 2 * j] = np.where(exists, hi + eps, -INF)
        rec[..., 3] = slope_factor(rec)
        out[level] = (rec, mms[level])
    return out


def check_all(h, s, W, H, levels_data, levels=None):
    """check_level on every level of {level: (records, minmax)} (or on `levels`); returns the largest margins"""
    top = num_levels(W, H)
    stats = dict(contain=-np.inf, tight=-np.inf)
    for level in (levels or range(1, top + 1)):
        rec, mm = levels_data[level]
        below = levels_data[level - 1][1] if level > SHEAR_TOP else None
        st = check_level(h, s, W, H, top, level, rec, mm, below)
        stats = {k: max(stats[k], st[k]) for k in stats}
    return stats


# -----------------------------------------------------------------------------------------------------------------
# the cases both test files run
# -----------------------------------------------------------------------------------------------------------------
# (2,2): top = 1, one cell.  (3,2), (2,3), (4,4): absent children inside existing nodes.  (33,33): top = 5 = SHEAR_TOP, every
# level fitted.  (34,33): top = 6, one min/max level.  (257,100): top = 8, the reduce, min/max-record and top kernels each
# build some depths.
SHAPES = [(2, 2), (3, 2), (2, 3), (4, 4), (5, 3), (17, 9), (33, 33), (34, 33), (65, 65), (100, 37), (257, 100)]


def terrain(kind, W, H, seed=0):
    """[H, W] float32 heights: 'rand' / 'sine' / 'stairs' of tests/common.py; 'ramp': an exact plane, heights multiples of
    2^-10 (with max_height a power of two every residual of an interior node is exactly zero); 'const'; 'wide': uniform
    in [-2, 3], heights outside [0, 1]"""
    import common
    rng = np.random.default_rng(seed + 1000 * W + H)
    if kind in ("rand", "sine", "stairs"):
        return common.heights(kind, W, H, rng)
    if kind == "ramp":
        return ((3.0 * np.arange(W)[None, :] + 5.0 * np.arange(H)[:, None]) * 2.0 ** -10).astype(F32)
    if kind == "const":
        return np.full((H, W), 0.375, F32)
    if kind == "wide":
        return rng.uniform(-2, 3, (H, W)).astype(F32)
    raise ValueError(kind)


# (W, H, terrain, max_height).  (257,100) takes 'rand' only among the three terrains of tests/common.py.  max_height: the
# contract z = fl32(h s) does not depend on the sign or the size of either factor.
CASES = ([(W, H, kind, 0.5) for (W, H) in SHAPES[:-1] for kind in ("rand", "sine", "stairs")]
         + [(257, 100, "rand", 0.5)]
         + [(W, H, kind, 0.5) for (W, H) in SHAPES for kind in ("ramp", "const")]
         + [(W, H, kind, s) for (W, H) in SHAPES for kind, s in (("rand", 1e-3), ("rand", 50.0), ("wide", -0.5))])

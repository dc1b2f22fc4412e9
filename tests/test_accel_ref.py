"""The checker of the acceleration data (tests/accel_ref.py) against records it can judge without a GPU: it accepts the
float32 emulation of the documented build on every small shape of tests/test_gpu_accel_records.py, and it rejects each
kind of broken record with the check that names the breakage.  This file is what shows that the GPU test can fail."""
import numpy as np
import pytest

import accel_ref as R

@pytest.mark.parametrize("W,H,kind,s", R.CASES)
def test_checker_accepts_the_emulated_build(W, H, kind, s):
    h = R.terrain(kind, W, H)
    R.check_all(h, s, W, H, R.emulate_build(h, s, W, H))


# ---- corruptions: one well-formed build, broken nine ways -------------------------------------------------------

W0, H0, S0 = 100, 37, 0.5          # top = 7: levels 1..5 fitted, 6 and 7 min/max; padded slots and absent children


@pytest.fixture(scope="module")
def good():
    h = R.terrain("rand", W0, H0)
    levels = R.emulate_build(h, S0, W0, H0)
    R.check_all(h, S0, W0, H0, levels)
    return h, levels


def _check(h, levels, level, rec=None, mm=None, below=None):
    r, m = levels[level]
    top = R.num_levels(W0, H0)
    if below is None and level > R.SHEAR_TOP:
        below = levels[level - 1][1]
    return R.check_level(h, S0, W0, H0, top, level, r if rec is None else rec, m if mm is None else mm, below)


def _widest_child(h, levels, level):
    """(iy, ix, j, eps_ref, slack) of the existing child with the widest range (so that a moved bound stays a range)"""
    rec = levels[level][0]
    size = 1 << level
    nx, ny = -(-(W0 - 1) // size), -(-(H0 - 1) // size)
    cb = R.child_bounds(R.scaled_heights(h, S0), W0, H0, level, rec[:ny, :nx], ny, nx)
    rng = np.where(cb["exists"], rec[:ny, :nx, 5::2] - rec[:ny, :nx, 4::2], -1.0)
    iy, ix, j = np.unravel_index(int(rng.argmax()), rng.shape)
    slack = max(cb["slack_max"][iy, ix, j], cb["slack_min"][iy, ix, j])
    return int(iy), int(ix), int(j), float(cb["eps"][iy, ix]), float(slack)


@pytest.mark.parametrize("level", [1, 3, 5])
@pytest.mark.parametrize("which", ["hi", "lo"])
def test_rejects_a_bound_that_is_too_narrow(good, level, which):
    h, levels = good
    iy, ix, j, eps, slack = _widest_child(h, levels, level)
    rec = levels[level][0].copy()
    d = np.float32(3 * eps + 2 * slack)
    if which == "hi":
        rec[iy, ix, 5 + 2 * j] -= d
    else:
        rec[iy, ix, 4 + 2 * j] += d
    with pytest.raises(R.AccelError, match=rf"check D: level {level} node \({ix}, {iy}\) child {j}") as e:
        _check(h, levels, level, rec=rec)
    assert e.value.check == "D"


@pytest.mark.parametrize("level", [1, 3, 5])
def test_rejects_a_bound_that_is_too_loose(good, level):
    h, levels = good
    iy, ix, j, eps, _ = _widest_child(h, levels, level)
    rec = levels[level][0].copy()
    rec[iy, ix, 5 + 2 * j] += np.float32(10 * eps)
    with pytest.raises(R.AccelError, match=rf"check E: level {level} node \({ix}, {iy}\) child {j}: hi"):
        _check(h, levels, level, rec=rec)


@pytest.mark.parametrize("level", [1, 2, 4])
def test_rejects_swapped_children(good, level):
    h, levels = good
    rec = levels[level][0].copy()
    # a node whose children 1 and 2 both exist and do not overlap: neither range can stand in for the other
    lo1, hi1, lo2, hi2 = (rec[..., k] for k in (6, 7, 8, 9))
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(lo1) & np.isfinite(lo2) & ((hi1 < lo2) | (hi2 < lo1))
    if not cand.any():   # overlapping everywhere: the pair that differs most
        cand = np.isfinite(lo1) & np.isfinite(lo2)
        with np.errstate(invalid="ignore"):
            d = np.where(cand, np.abs(hi1 - hi2), -1.0)
        cand = d == d.max()
    iy, ix = R._first(cand)
    assert not np.array_equal(rec[iy, ix, 6:8], rec[iy, ix, 8:10])
    rec[iy, ix, 6:8], rec[iy, ix, 8:10] = rec[iy, ix, 8:10].copy(), rec[iy, ix, 6:8].copy()
    with pytest.raises(R.AccelError, match=rf"check D: level {level} node \({ix}, {iy}\) child [12]"):
        _check(h, levels, level, rec=rec)


def test_rejects_swapped_children_on_a_minmax_level(good):
    h, levels = good
    rec = levels[6][0].copy()
    assert not np.array_equal(rec[0, 0, 6:8], rec[0, 0, 8:10])
    rec[0, 0, 6:8], rec[0, 0, 8:10] = rec[0, 0, 8:10].copy(), rec[0, 0, 6:8].copy()
    with pytest.raises(R.AccelError, match=r"check C: level 6 node \(0, 0\) child 1"):
        _check(h, levels, 6, rec=rec)


@pytest.mark.parametrize("level", [1, 3, 7])
def test_rejects_an_absent_child_with_a_finite_range(good, level):
    h, levels = good
    rec = levels[level][0].copy()
    # an existing node (child 0 holds a range) of which some child lies beyond the grid
    absent = np.isfinite(rec[..., 4:5]) & (rec[..., 4::2] == np.inf)
    iy, ix, j = R._first(absent)
    assert absent[iy, ix, j] and j > 0
    rec[iy, ix, 4 + 2 * j:6 + 2 * j] = rec[iy, ix, 4:6]
    with pytest.raises(R.AccelError, match=rf"check A: level {level} node \({ix}, {iy}\) child {j} is absent"):
        _check(h, levels, level, rec=rec)


@pytest.mark.parametrize("level", [1, 4, 6])
def test_rejects_a_padded_pyramid_slot_that_is_not_empty(good, level):
    h, levels = good
    mm = levels[level][1].copy()
    side = mm.shape[0]
    assert mm[side - 1, side - 1, 0] == np.inf
    mm[side - 1, side - 1] = 0.0
    with pytest.raises(R.AccelError, match=rf"check A: level {level} node \({side - 1}, {side - 1}\) has no cell"):
        _check(h, levels, level, mm=mm)


def test_rejects_stale_records(good):
    """records of other heights: one interior vertex (odd indices: a corner of no node, so every plane is unchanged)
    was 0.25 higher when they were built"""
    h, levels = good
    h2 = h.copy()
    y, x = 1 + 2 * np.array(np.unravel_index(int(h[1:-1:2, 1:-1:2].argmax()), h[1:-1:2, 1:-1:2].shape))
    h2[y, x] += 0.25
    stale = R.emulate_build(h2, S0, W0, H0)
    R.check_all(h2, S0, W0, H0, stale)
    for level in range(1, R.SHEAR_TOP + 1):       # the vertex tops its cells: every fitted level holds a loose hi
        with pytest.raises(R.AccelError, match=rf"check E: level {level} node \({x >> level}, {y >> level}\) child \d: hi"):
            _check(h, levels, level, rec=stale[level][0])
    top = R.num_levels(W0, H0)
    assert stale[top][1][0, 0, 1] != levels[top][1][0, 0, 1]
    for level in range(1, top + 1):               # and the stale pyramid is not the heights'
        with pytest.raises(R.AccelError, match=rf"check B: level {level} node \({x >> level}, {y >> level}\) pyramid max"):
            _check(h, levels, level, mm=stale[level][1])
    # the other direction (a vertex that has risen since the build) breaks containment
    with pytest.raises(R.AccelError, match=r"check D: level 1"):
        R.check_level(h2, S0, W0, H0, top, 1, levels[1][0], stale[1][1])


@pytest.mark.parametrize("level", [1, 5, 6, 7])
def test_rejects_a_halved_slope_factor(good, level):
    h, levels = good
    rec = levels[level][0].copy()
    assert rec[0, 0, 3] > 0
    rec[0, 0, 3] *= np.float32(0.5)
    with pytest.raises(R.AccelError, match=rf"check F: level {level} node \(0, 0\)"):
        _check(h, levels, level, rec=rec)


@pytest.mark.parametrize("level,k", [(6, 4), (6, 11), (7, 5), (7, 6)])
def test_rejects_a_minmax_child_one_ulp_off_the_pyramid(good, level, k):
    h, levels = good
    rec = levels[level][0].copy()
    away = np.float32(-np.inf if k % 2 == 0 else np.inf)      # lo downwards, hi upwards: still conservative, no longer the slot
    assert np.isfinite(rec[0, 0, k])
    rec[0, 0, k] = np.nextafter(rec[0, 0, k], away)
    with pytest.raises(R.AccelError, match=rf"check C: level {level} node \(0, 0\) child {(k - 4) >> 1}"):
        _check(h, levels, level, rec=rec)


def test_rejects_a_nonzero_plane_on_a_minmax_level(good):
    h, levels = good
    rec = levels[6][0].copy()
    rec[0, 1, 1] = np.float32(-0.0)
    with pytest.raises(R.AccelError, match=r"check C: level 6 node \(1, 0\) .* plane entry b"):
        _check(h, levels, 6, rec=rec)

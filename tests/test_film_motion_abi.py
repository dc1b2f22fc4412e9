"""The film that is differentiable in the sample positions and takes a per-sample weight (hf_film_splat_weighted,
_adjoint, _tangent) on the CPU: the three entry points are declared, exported and bound; every bad argument is refused
before anything touches a device; the float64 restatement (tests/film_ref.py) agrees with the oracle's film where the
two overlap, its position / weight derivatives with central differences of its own forward, and its tangent is the
transpose of its adjoint."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols
import film_ref as F

FNS = ("hf_film_splat_weighted", "hf_film_splat_weighted_adjoint", "hf_film_splat_weighted_tangent")


def test_symbols_declared_exported_and_bound():
    assert_symbols(FNS)


# ---- argument checks: host addresses stand in for device pointers, every case fails before a launch ------------------

def _call(lib, fn, n=4, channels=3, stddev=0.5, width=8, height=8, null=(), null_row=None, outs=("v", "w", "x", "y")):
    from hf_amd import _capi
    keep = (C.c_float * 64)()
    a = C.addressof(keep)

    def rows(name):
        if name in null:
            return None
        r = (_capi._fp * 8)(*([a] * 8))
        if null_row == name:
            r[min(channels, 8) - 1 if channels else 0] = None
        return r
    arg = lambda name: None if name in null else a
    head = (n, channels, rows("values"), arg("sample_weight"), arg("pos_x"), arg("pos_y"), width, height, stddev)
    if fn == FNS[0]:
        return getattr(lib, fn)(*head, arg("image"), arg("weight"), None)
    if fn == FNS[1]:
        return getattr(lib, fn)(*head, arg("grad_image"), arg("grad_weight"), rows("grad_values") if "v" in outs else None,
                                a if "w" in outs else None, a if "x" in outs else None, a if "y" in outs else None, None)
    return getattr(lib, fn)(*head, rows("dvalues"), arg("dsample_weight"), arg("dpos_x"), arg("dpos_y"), arg("image"),
                            arg("weight"), None)


COMMON = [{"null": ("pos_x",)}, {"null": ("pos_y",)}, {"channels": 0}, {"channels": 9}, {"stddev": 0.0}, {"stddev": 1.5},
          {"stddev": float("nan")}, {"stddev": -0.5}, {"n": 1 << 32}, {"width": 0}, {"height": 0}]
CASES = {
    FNS[0]: COMMON + [{"null": ("values",)}, {"null": ("image",)}, {"null": ("weight",)}, {"null_row": "values"}],
    FNS[1]: COMMON + [{"null": ("grad_image",)}, {"null_row": "values"}, {"null_row": "grad_values"}, {"outs": ()},
                      {"null": ("values",), "outs": ("x",)}, {"null": ("values",), "outs": ("v", "y")}],
    FNS[2]: COMMON + [{"null": ("values",)}, {"null": ("image",)}, {"null": ("weight",)}, {"null_row": "values"},
                      {"null_row": "dvalues"}],
}


@pytest.mark.parametrize("fn", FNS)
def test_bad_arguments_are_refused(fn):
    assert_refused(_call, fn, CASES[fn])


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def _samples(rng, n, Wd, Hd, stddev, margin=1e-3):
    """n film positions in [-1.5, size + 1.5], none with an |x| or |y| within `margin` of the radius for any pixel: a
    position that is gets drawn again (none is left out)"""
    pos = np.stack([rng.uniform(-1.5, Wd + 1.5, n), rng.uniform(-1.5, Hd + 1.5, n)])
    for _ in range(100):
        bad = (F.edge_distance(pos[0], Wd, stddev) <= margin) | (F.edge_distance(pos[1], Hd, stddev) <= margin)
        if not bad.any():
            break
        pos[0, bad] = rng.uniform(-1.5, Wd + 1.5, int(bad.sum()))
        pos[1, bad] = rng.uniform(-1.5, Hd + 1.5, int(bad.sum()))
    return pos


def test_restatement_agrees_with_the_oracle(oracle):
    rng = np.random.default_rng(8)
    n, K, Wd, Hd = 200, 3, 9, 7
    for stddev in (0.3, 0.5, 1.0):
        pos = np.stack([rng.uniform(-1.5, Wd + 1.5, n), rng.uniform(-1.5, Hd + 1.5, n)])
        v = rng.normal(size=(K, n)); g = rng.normal(size=(K, Wd * Hd))
        img, w = oracle.film_splat(v, pos, Wd, Hd, stddev)
        image, weight = F.forward(v, None, pos, Wd, Hd, stddev)
        assert np.count_nonzero(w) > 0.9 * w.size
        assert np.allclose(image, img, rtol=1e-12, atol=1e-12), np.abs(image - img).max()
        assert np.allclose(weight, w, rtol=1e-12, atol=1e-12), np.abs(weight - w).max()
        gv, _, _ = F.adjoint(v, None, pos, Wd, Hd, stddev, g)
        ref = oracle.film_splat_adjoint(pos, Wd, Hd, g, stddev)
        assert np.allclose(gv, ref, rtol=1e-12, atol=1e-12), np.abs(gv - ref).max()


@pytest.mark.parametrize("stddev", [0.3, 0.5, 1.0])
def test_position_and_weight_derivatives_against_central_differences(stddev):
    """step 1e-5 in float64: truncation ~ step^2 |w'''| / 6 ~ 5e-9 of the gradient, rounding ~ 1e-16 / step = 1e-11"""
    rng = np.random.default_rng(int(stddev * 10) + 40)
    n, K, Wd, Hd, step = 48, 3, 9, 7, 1e-5
    pos = _samples(rng, n, Wd, Hd, stddev)
    assert min(F.edge_distance(pos[0], Wd, stddev).min(), F.edge_distance(pos[1], Hd, stddev).min()) > 1e-3
    v = rng.normal(size=(K, n)); sw = rng.uniform(0.5, 1.5, n)
    gi = rng.normal(size=(K, Hd * Wd)); gw = rng.normal(size=Hd * Wd)

    def loss(v_, sw_, pos_):
        image, weight = F.forward(v_, sw_, pos_, Wd, Hd, stddev)
        return (image * gi).sum() + (weight * gw).sum()
    _, gsw, gpos = F.adjoint(v, sw, pos, Wd, Hd, stddev, gi, gw)
    fd_pos, fd_sw = np.zeros((2, n)), np.zeros(n)
    for i in range(n):
        for c in range(2):
            e = np.zeros((2, n)); e[c, i] = step
            fd_pos[c, i] = (loss(v, sw, pos + e) - loss(v, sw, pos - e)) / (2 * step)
        e = np.zeros(n); e[i] = step
        fd_sw[i] = (loss(v, sw + e, pos) - loss(v, sw - e, pos)) / (2 * step)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    print(f"stddev {stddev}: grad_pos_x {rel(gpos[0], fd_pos[0]):.3g} grad_pos_y {rel(gpos[1], fd_pos[1]):.3g} "
          f"grad_sample_weight {rel(gsw, fd_sw):.3g}")
    assert np.linalg.norm(fd_pos[0]) > 0 and np.linalg.norm(fd_pos[1]) > 0 and np.linalg.norm(fd_sw) > 0
    assert rel(gpos[0], fd_pos[0]) <= 1e-6
    assert rel(gpos[1], fd_pos[1]) <= 1e-6
    assert rel(gsw, fd_sw) <= 1e-6


@pytest.mark.parametrize("which", ["values", "sample_weight", "pos", "all"])
@pytest.mark.parametrize("stddev", [0.3, 0.5, 1.0])
def test_restatement_tangent_is_the_transpose_of_the_adjoint(stddev, which):
    rng = np.random.default_rng(23)
    n, K, Wd, Hd = 300, 3, 23, 17
    pos = np.stack([rng.uniform(-1.5, Wd + 1.5, n), rng.uniform(-1.5, Hd + 1.5, n)])
    v = rng.normal(size=(K, n)); sw = rng.uniform(0.5, 1.5, n)
    gi = rng.normal(size=(K, Hd * Wd)); gw = rng.normal(size=Hd * Wd)
    tan = {"values": rng.normal(size=(K, n)), "sample_weight": rng.normal(size=n), "pos": rng.normal(size=(2, n))}
    use = tan if which == "all" else {which: tan[which]}
    dimage, dweight = F.tangent(v, sw, pos, Wd, Hd, stddev, use.get("values"), use.get("sample_weight"), use.get("pos"))
    gv, gsw, gpos = F.adjoint(v, sw, pos, Wd, Hd, stddev, gi, gw)
    grads = {"values": gv, "sample_weight": gsw, "pos": gpos}
    lhs = (dimage * gi).sum() + (dweight * gw).sum()
    rhs = sum((grads[k] * use[k]).sum() for k in use)
    assert abs(lhs) > 1e-6
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs, abs(lhs - rhs) / abs(lhs))

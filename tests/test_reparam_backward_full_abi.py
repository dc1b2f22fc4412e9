"""Reverse-mode reparameterisation with respect to the heights, the ray and to_world (hf_reparam_backward_full) on the
CPU: the entry point is declared, exported and bound; every bad argument is refused before anything touches a device;
the float64 restatement (tests/reparam_backward_ref.py) is the transpose of tests/reparam_tangent_ref.py for every kind
of tangent, and its heights / ray.o / ray.d parts agree with oracle.reparam_backward."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols
import common
import reparam_backward_ref as B
import reparam_tangent_ref as R
from test_reparam_tangent_abi import _setup

FN = "hf_reparam_backward_full"


def test_symbol_declared_exported_and_bound():
    assert_symbols((FN,), ("reparameterize_ray_adjoint",))


def _call(lib, hf, n=4, num_rays=4, kappa=1e5, stride=None, null=(), outs=("h", "o", "d", "M")):
    from hf_amd import _capi
    keep = (C.c_float * 64)()
    a = C.addressof(keep)
    rows = (_capi._fp * 3)(a, a, a)
    p = _capi.hf_pi_t()
    p.t = p.prim_uv[0] = p.prim_uv[1] = p.prim_index = a
    arg = lambda name, v: None if name in null else v
    return getattr(lib, FN)(hf, n, arg("o", C.byref(rows)), arg("d", C.byref(rows)), None, num_rays, kappa, 3.0, 0, 0, None,
                            arg("pi", C.byref(p)), arg("bt", a), 4 * n if stride is None else stride,
                            arg("g_dir", C.byref(rows)), arg("g_div", a),
                            a if "h" in outs else None, C.byref(rows) if "o" in outs else None,
                            C.byref(rows) if "d" in outs else None, a if "M" in outs else None, None)


def test_bad_arguments_are_refused():
    fake = C.create_string_buffer(4096)   # never dereferenced: every case fails before the handle's device is read
    h = C.cast(fake, C.c_void_p)
    cases = [{"hf": None}]                                                 # (every case but this one has the handle h)
    cases += [{"null": (name,)} for name in ("o", "d", "pi", "bt", "g_dir", "g_div")]
    cases += [{"outs": ()}, {"kappa": 0.0}, {"kappa": -1.0}, {"kappa": float("nan")}, {"num_rays": 0}, {"num_rays": 33},
              {"stride": 3}, {"n": 1 << 32}]
    assert_refused(lambda lib, fn, hf=h, **kw: _call(lib, hf, **kw), FN, cases)


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def _grads(n):
    rng = np.random.default_rng(17)
    return rng.normal(size=(3, n)), rng.normal(size=n)


@pytest.mark.parametrize("which", ["h", "o", "d", "M", "all"])
def test_restatement_is_the_transpose_of_the_tangent(oracle, which):
    h, M, f, o, d, S, act = _setup(oracle, tw=common.affine(2))
    hits = sum(s[1].sum() for s in S)
    misses = sum((~s[1] & act).sum() for s in S)
    assert hits > 50 and misses > 10, (hits, misses)     # both branches of V_direct are exercised
    n = o.shape[1]
    rng = np.random.default_rng(5)
    tan = {"h": rng.normal(size=h.shape), "o": rng.normal(size=(3, n)), "d": rng.normal(size=(3, n)),
           "M": rng.normal(size=(3, 4))}
    use = tan if which == "all" else {which: tan[which]}
    g_dir, g_div = _grads(n)
    o64, d64, h64 = o.astype(np.float64), d.astype(np.float64), h.astype(np.float64)
    Vt, div, _, _ = R.reparam_tangent(f, S, act, o64, d64, M, h64, use.get("h"), use.get("o"), use.get("d"), use.get("M"))
    gh, go, gd, gM = B.reparam_backward(f, S, act, o64, d64, M, h64, g_dir, g_div)
    grads = {"h": gh, "o": go, "d": gd, "M": gM}
    lhs = (g_dir * B.project(d64, Vt)).sum() + (g_div * div).sum()
    rhs = sum((grads[k] * use[k]).sum() for k in use)
    assert abs(lhs) > 1e-6
    assert abs(lhs - rhs) <= 1e-9 * abs(lhs), (lhs, rhs, abs(lhs - rhs) / abs(lhs))
    assert np.all(go[:, ~act] == 0) and np.all(gd[:, ~act] == 0)


def test_restatement_agrees_with_the_oracle(oracle):
    h, M, f, o, d, S, act = _setup(oracle)
    hits = sum(s[1].sum() for s in S)
    misses = sum((~s[1] & act).sum() for s in S)
    assert hits > 50 and misses > 10, (hits, misses)
    n = o.shape[1]
    g_dir, g_div = _grads(n)
    rh, ro, rd = oracle.reparam_backward(f, o, d, g_dir.astype(np.float32), g_div.astype(np.float32), num_rays=6,
                                         kappa=300.0, exponent=3.0, antithetic=True, seed=4, active=act, ray_grads=True)
    g32 = g_dir.astype(np.float32).astype(np.float64), g_div.astype(np.float32).astype(np.float64)
    gh, go, gd, _ = B.reparam_backward(f, S, act, o, d, M, h, *g32)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert np.linalg.norm(rh) > 0 and np.linalg.norm(ro) > 0 and np.linalg.norm(rd) > 0
    assert rel(gh, rh) <= 3e-5, rel(gh, rh)
    assert rel(go, ro) <= 2e-4, rel(go, ro)
    assert rel(gd, rd) <= 2e-4, rel(gd, rd)

"""Forward-mode reparameterisation (hf_reparam_tangent) on the CPU: the entry point is declared, exported and bound;
NULL handles, bad num_rays and bad kappa are refused before anything touches a device; the float64 restatement
(tests/reparam_tangent_ref.py) is the directional derivative of sum_k w_k V_direct_k and sum_k <d_w_omega_k,
V_direct_k> for tangents of the heights, the ray and to_world, reduces to oracle.reparam_forward for heights, and
reproduces the known answers of the reference's test01 (src/render/tests/test_reparameterization.py:29-98)."""
import ctypes as C

import numpy as np
import pytest

from abi_helpers import assert_refused, assert_symbols
import common
import reparam_tangent_ref as R


def test_symbol_declared_exported_and_bound():
    assert_symbols(("hf_reparam_tangent",), ("reparameterize_ray_tangent",))
    from hf_amd import shape as sh
    import torch
    assert sh._ReparameterizeOp.jvp is not torch.autograd.Function.jvp


def _call(lib, hf, n=4, num_rays=4, kappa=1e5, pi=True, out=True):
    from hf_amd import _capi
    keep = (C.c_float * 64)()
    a = C.addressof(keep)
    rows = (_capi._fp * 3)(a, a, a)
    p = _capi.hf_pi_t()
    p.t = p.prim_uv[0] = p.prim_uv[1] = p.prim_index = a
    return lib.hf_reparam_tangent(hf, n, C.byref(rows), C.byref(rows), None, num_rays, kappa, 3.0, 0, 0, None,
                                  C.byref(p) if pi else None, a, 4 * n, None, None, None, None,
                                  C.byref(rows) if out else None, a if out else None, None)


def test_bad_arguments_are_refused():
    fake = C.create_string_buffer(4096)   # never dereferenced: every case fails before the handle's device is read
    h = C.cast(fake, C.c_void_p)
    cases = [{"hf": None}, {"num_rays": 0}, {"num_rays": 33}, {"kappa": 0.0}, {"kappa": float("nan")}, {"kappa": -1.0},
             {"pi": False}, {"out": False}, {"n": 1 << 32}]                # (every case but the first has the handle h)
    assert_refused(lambda lib, fn, hf=h, **kw: _call(lib, hf, **kw), "hf_reparam_tangent", cases)


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def _scene(oracle, W=33, H=29, seed=0, tw=None):
    rng = np.random.default_rng(seed)
    u = np.arange(W) / (W - 1.0); v = np.arange(H)[:, None] / (H - 1.0)
    h = (0.5 + 0.3 * np.sin(2 * np.pi * 1.5 * u) * np.cos(2 * np.pi * 1.2 * v)
         + 0.03 * rng.uniform(-1, 1, (H, W))).astype(np.float32)
    M = np.eye(4)[:3] if tw is None else np.asarray(tw, np.float64)
    return h, M, oracle.OracleField(h, max_height=0.5, to_world=M)


def _setup(oracle, tw=None, n=60, kappa=300.0, antithetic=True, seed=4):
    h, M, f = _scene(oracle, tw=tw)
    rng = np.random.default_rng(11)
    tgt = np.stack([rng.uniform(-1.1, 1.1, n), rng.uniform(-1.1, 1.1, n), np.full(n, 0.25)])
    o = tgt + np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.0, 2.0, n)])
    A = np.asarray(M, np.float64)
    o, tgt = A[:, :3] @ o + A[:, 3:4], A[:, :3] @ tgt + A[:, 3:4]
    d = tgt - o; d /= np.linalg.norm(d, axis=0)
    o, d = o.astype(np.float32), d.astype(np.float32)
    active = (np.arange(n) % 7 != 3).astype(np.uint8)
    S, act = R.samples(oracle, f, o, d, 6, kappa, 3.0, antithetic, seed, active)
    return h, M, f, o, d, S, act


@pytest.mark.parametrize("which", ["h", "o", "d", "M", "all"])
def test_restatement_is_the_derivative_of_the_vdirect_sums(oracle, which):
    h, M, f, o, d, S, act = _setup(oracle, tw=common.affine(2))
    rng = np.random.default_rng(5)
    n = o.shape[1]
    tan = {"h": rng.normal(size=h.shape), "o": rng.normal(size=(3, n)), "d": rng.normal(size=(3, n)),
           "M": rng.normal(size=(3, 4))}
    use = tan if which == "all" else {which: tan[which]}
    hits = sum(s[1].sum() for s in S)
    misses = sum((~s[1] & act).sum() for s in S)
    assert hits > 50 and misses > 10, (hits, misses)     # both branches of V_direct are exercised
    o64, d64, h64 = o.astype(np.float64), d.astype(np.float64), h.astype(np.float64)
    _, _, gV, gdiv = R.reparam_tangent(f, S, act, o64, d64, M, h64, use.get("h"), use.get("o"), use.get("d"), use.get("M"))
    eps = 1e-6

    def at(s):
        z = lambda k, shp: s * use[k] if k in use else np.zeros(shp)
        return R.vdirect_sums(f, S, o64 + z("o", (3, n)), d64 + z("d", (3, n)), M + z("M", (3, 4)), h64 + z("h", h.shape))
    (vp, dp), (vm, dm) = at(eps), at(-eps)
    fdV, fdD = (vp - vm) / (2 * eps), (dp - dm) / (2 * eps)
    assert np.linalg.norm(gV - fdV) <= 1e-6 * np.linalg.norm(fdV), np.linalg.norm(gV - fdV) / np.linalg.norm(fdV)
    assert np.linalg.norm(gdiv - fdD) <= 1e-6 * np.linalg.norm(fdD), np.linalg.norm(gdiv - fdD) / np.linalg.norm(fdD)
    assert np.linalg.norm(fdV) > 1e-3


def test_restatement_reduces_to_the_oracle_for_heights(oracle):
    h, M, f, o, d, S, act = _setup(oracle)
    dh = np.random.default_rng(8).normal(size=h.shape)
    Vt, div, _, _ = R.reparam_tangent(f, S, act, o, d, M, h, dh=dh)
    ref_V, ref_div = oracle.reparam_forward(f, o, d, dh, num_rays=6, kappa=300.0, antithetic=True, seed=4, active=act)
    assert np.allclose(Vt, ref_V, rtol=1e-4, atol=1e-5 * np.abs(ref_V).max())
    assert np.allclose(div, ref_div, rtol=1e-4, atol=1e-5 * np.abs(ref_div).max())
    assert np.all(Vt[:, ~act] == 0) and np.all(div[~act] == 0)


# the reference's test01: a rectangle [-1, 1]^2 at z = 0 (here: a flat heightfield) translated along x by theta; rays
# from z = -5 along +z at one side, the centre and one corner; 32 auxiliary rays, kappa 1e6, exponent 3
TEST01 = {"side": [0.0, 1.0, -5.0], "centre": [0.0, 0.0, -5.0], "corner": [0.99, -0.99, -5.0]}
TRANSLATE_X = np.array([[0, 0, 0, 1.0], [0, 0, 0, 0], [0, 0, 0, 0]])


@pytest.mark.parametrize("name", list(TEST01))
def test_restatement_reproduces_the_reference_test01(oracle, name):
    h = np.zeros((9, 9), np.float32)
    M = np.eye(4)[:3]
    f = oracle.OracleField(h, max_height=1.0, to_world=M)
    o = np.array(TEST01[name], np.float32)[:, None]; d = np.array([[0.0], [0.0], [1.0]], np.float32)
    S, act = R.samples(oracle, f, o, d, 32, 1e6, 3.0)
    Vt, div, _, _ = R.reparam_tangent(f, S, act, o, d, M, h, dM=TRANSLATE_X)
    r = np.concatenate([o, d, [[np.inf]]]).astype(np.float32)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    p = f.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)["p"].astype(np.float64)
    new_d = p + np.array([[1.0], [0.0], [0.0]]) - o
    new_d /= np.linalg.norm(new_d)
    assert abs(float(new_d[0, 0] - d[0, 0]) - float(Vt[0, 0])) <= 1e-2, (new_d.ravel(), Vt.ravel())
    assert abs(Vt[1, 0]) < 1e-4 and abs(Vt[2, 0]) < 1e-4, Vt.ravel()

"""Environment-map lighting (hf_envmap_*) on the scenes `affine`, `mirror_flip` and `rand8` of tests/lighting_scenes.py
(2300 samples: a partial last wave and workgroup; K = 4, seed 5) under the maps of tests/envmap_ref.py: `sun` (17 x 9, u = 0
and 0.25: zero-weight cells, a 250 : 1 range), `gradient` (9 x 5, positive everywhere) and `2x2` (one cell).  Every
comparison has a judge that is not the product: the oracle for what is traced, the float64 restatement
(tests/envmap_ref.py, held against quadrature and central differences by tests/test_envmap_ref.py) for what is computed.
The restatement reads the DEVICE's table for the draws, so that it draws the same cells; the table itself is compared
with the restatement's own.

cpu_model() runs a (scene, map) pair with the oracle and the restatement alone and returns the shares that make the pair
a test; test_scene_conditions_on_the_cpu asserts them without a GPU."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import common
import envmap_ref as E
import lighting_scenes as LS
import sky_ref as S
from lighting_scenes import K, MARGIN, SEED, SPLIT, _np, _rows7
from row_helpers import GUARD, _cu, _fold, guarded, intact, sub

gpu = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
SCENES = ("affine", "mirror_flip", "rand8")
MAPS = (("sun", 0.0), ("sun", 0.25), ("gradient", 0.0), ("2x2", 0.0))
PAIRS = [(s, m, u) for s in SCENES for m, u in MAPS]
ROT = E.DEFAULT_ROT
ALBEDO = 0.7


def _id(p):
    return "-".join(str(x) for x in p)


def cpu_model(sc, data, table, oracle, ids=None):
    """the (scene, map) pair through the oracle and the restatement only: records, draws, visibility and the shares"""
    f = LS.oracle_field(sc, oracle)
    r = sc.rays
    t, u, v, prim = f.ray_intersect_preliminary(r)
    rec = f.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)
    p, gn, sh_n, d = (x.astype(np.float64) for x in (rec["p"], rec["n"], rec["sh_n"], r[3:6]))
    m = types.SimpleNamespace(field=f, t=t, p=p, n=gn, sh_n=sh_n, d=d)
    m.dr = E.draws(data, table, np.arange(sc.n) if ids is None else ids, K, SEED, ROT)
    m.eligible, _ = S.eligible(sh_n, d, t)
    m.traced, m.margin = E.traced(sh_n, d, t, m.dr)
    m.vis = np.zeros((K, sc.n), bool)
    for k in range(K):
        tr = np.flatnonzero(m.traced[k])
        rk = LS._rays7(S.spawn_origin(p, gn, m.dr["w"][k])[:, tr], m.dr["w"][k][:, tr])
        m.vis[k, tr] = ~f.ray_test(rk).astype(bool)
    valid = m.dr["valid"] & m.eligible[None]
    on = np.broadcast_to(m.vis[:, None, :], m.dr["idx"].shape)
    touched = np.bincount(m.dr["idx"][on], minlength=data.size)
    m.shares = {"eligible": float(m.eligible.mean()), "valid": valid.sum() / max(m.eligible.sum() * K, 1),
                "traced": m.traced.sum() / max(valid.sum(), 1), "unoccluded": m.vis.sum() / max(m.traced.sum(), 1),
                "undecided": float((m.eligible[None] & m.dr["valid"] & (m.margin <= MARGIN)).mean()),
                "texels_touched": int((touched > 0).sum()), "max_per_texel": int(touched.max())}
    return m


def check_shares(name, s):
    print(name, s)
    assert s["eligible"] > 0.5 and s["valid"] == 1.0 and 0.3 <= s["traced"] <= 0.95
    assert 0.3 <= s["unoccluded"] <= 0.95 and s["undecided"] <= 1e-3 and s["max_per_texel"] <= 4435


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_scene_conditions_on_the_cpu(oracle, pair):
    scene, name, u = pair
    data = E.MAPS[name]()
    m = cpu_model(LS.scene(scene), data, E.build_table(data, u), oracle)
    check_shares(pair, m.shares)
    assert m.shares["texels_touched"] >= {"sun": 96, "gradient": 38, "2x2": 4}[name]


# ---- the GPU side ------------------------------------------------------------------------------------------------------
_BUILT = {}


def _env(hf, name, u, to_world=None):
    data = E.MAPS[name]()
    return data, hf.Envmap(_cu(data[:, :-1]), to_world=to_world, defensive=u)


def _scene(hf, oracle, name):
    if name not in _BUILT:
        sc = LS.scene(name)
        sc.shape = hf.Heightfield(heightfield=_cu(sc.h), max_height=sc.max_height, to_world=np.asarray(sc.to_world, np.float64),
                                  flip_normals=sc.flip)
        rt = _cu(sc.rays)
        sc.ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
        sc.si = si = sc.shape.ray_intersect(sc.ray, hf.RayFlags.All)
        sc.np = {k: _np(v) for k, v in (("p", si.p), ("n", si.n), ("sh_n", si.sh_frame.n), ("d", sc.ray.d), ("t", si.t))}
        sc.arrs = [sc.np[k] for k in ("sh_n", "d", "t")]
        sc.eligible, _ = S.eligible(*sc.arrs)
        sc.field = LS.oracle_field(sc, oracle)
        _BUILT[name] = sc
    return _BUILT[name]


@pytest.fixture(scope="module", params=PAIRS, ids=_id)
def cfg(request, hf, oracle):
    scene, name, u = request.param
    sc = _scene(hf, oracle, scene)
    c = types.SimpleNamespace(sc=sc, name=name, u=u, pair=request.param)
    c.data, c.env = _env(hf, name, u)
    c.table = _np(c.env.table())
    c.dr = E.draws(c.data, c.table, np.arange(sc.n), 32, SEED, ROT)          # every num_rays is a prefix
    c.traced, c.margin = E.traced(*sc.arrs, c.dr)
    c.rays = [hf.envmap_rays(sc.si, sc.ray, c.env, k, seed=SEED, return_weight=True) for k in range(K)]
    _, vis = hf.envmap_lighting(sc.shape, sc.si, sc.ray, c.env, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    c.vis_t, c.words = vis, _np(vis).view(np.uint32)
    return c


def _prefix(dr, k):
    return {key: v[:k] for key, v in dr.items()}


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the table ---------------------------------------------------------------------------------------------------------
def _big_map():
    rng = np.random.default_rng(3)
    m = rng.uniform(0.0, 2.0, (40, 599)) * (rng.uniform(size=(40, 599)) > 0.2)       # 599 cells per row: three chunks of 256
    return E.with_seam(m).astype(np.float32)


@gpu
@pytest.mark.parametrize("which", list(MAPS) + [("big", 0.1), ("big", 1.0)], ids=_id)
def test_table_against_the_restatement(hf, which):
    name, u = which
    data = _big_map() if name == "big" else E.MAPS[name]()
    env = hf.Envmap(_cu(data[:, :-1]), defensive=u)
    got = _np(env.table()).copy()
    ref = E.build_table(data, u)
    H, W = data.shape
    assert got.shape == ref.shape == (hf._capi.lib().hf_envmap_table_floats(W, H),)
    print(which, "max ulps", _ulps(got, ref).max(), "Sigma", got[0])
    assert _ulps(got[4:], ref[4:]).max() <= 1
    assert got[0] == got[4 + H - 2] and got[1] == ref[1] and got[2] == np.float32(u) and got[3] == 0     # the header: exact
    first = env.table()
    env.parameters_changed()
    assert env.table() is not first and torch.equal(env.table(), first)                 # bitwise the same from build to build
    with torch.no_grad():
        env.data.mul_(2.0)                                                              # a write to the texels: rebuilt
    assert np.allclose(_np(env.table())[0], 2.0 * got[0], rtol=1e-6)


# ---- sample_direction at forced samples, eval, pdf ------------------------------------------------------------------------
def _forced(data, table):
    """(sx, sy): 0, 1 - 2^-23, every marginal and conditional boundary divided by its total, and its float32 neighbours.
    On `sun` the zero-weight cell rows come last, so their boundaries are M / Sigma = 1: no sample of [0, 1) reaches them, and
    the clip folds them onto 1 - 2^-23.  The boundary of a zero-weight cell that a sample CAN land on is that of the `hole`
    map below (a zero-weight FIRST row: sy = 0 draws it and is invalid), with the all-zero map for Sigma = 0."""
    H, W = data.shape
    sigma, _, _, M, Cc = E.split_table(table, W, H)
    F = np.float32
    near = lambda v: np.concatenate([np.nextafter(v, F(-1)), v, np.nextafter(v, F(2))])
    top = F(1 - 2.0 ** -23)
    with np.errstate(all="ignore"):
        ys = np.clip(np.nan_to_num(np.concatenate([[F(0), top], near((M / sigma).astype(F))])), 0, top).astype(F)
        sx, sy = [], []
        for r in range(H - 1):
            lo = M[r - 1] if r else F(0)
            mid = F((float(lo) + float(M[r])) / 2 / float(sigma)) if sigma > 0 else F(0.5)
            xs = np.clip(np.nan_to_num(np.concatenate([[F(0), top], near((Cc[r] / Cc[r, -1]).astype(F))])), 0, top).astype(F)
            sx += [xs, np.full(len(ys), F(0.37)) if r == 0 else xs[:0]]
            sy += [np.full(len(xs), np.clip(mid, 0, top)), ys if r == 0 else ys[:0]]
    return np.concatenate(sx).astype(F), np.concatenate(sy).astype(F)


def _hole_map():
    m = E.map_gradient()
    m[:2] = 0.0                                                              # cell row 0 has no weight: M[0] = 0
    return m


# (rounded to float32, as the entries receive it: near a pole the lookup amplifies a 6e-8 error of the rotation a thousandfold)
GENERIC_ROT = (common.rot(0, 0.4) @ common.rot(2, -1.1) @ common.rot(1, 0.7)).astype(np.float32).astype(np.float64)
FLT_MIN = 2.0 ** -126      # below it a float32 is denormal and cannot hold a relative 1e-5


@gpu
@pytest.mark.parametrize("which", list(MAPS) + [("hole", 0.0), ("zero", 0.0)], ids=_id)
@pytest.mark.parametrize("rot", ["default", "generic"])
def test_sample_direction_eval_and_pdf(hf, which, rot):
    name, u = which
    data = {"hole": _hole_map, "zero": lambda: np.zeros((5, 9), np.float32)}.get(name, E.MAPS.get(name))()
    R = ROT if rot == "default" else GENERIC_ROT
    env = hf.Envmap(_cu(data[:, :-1]), to_world=None if rot == "default" else R, defensive=u)
    table = _np(env.table())
    H, W = data.shape
    rng = np.random.default_rng(11)
    fsx, fsy = _forced(data, table)
    sx = np.concatenate([fsx, (rng.integers(0, 1 << 23, 3000) * 2.0 ** -23).astype(np.float32)])
    sy = np.concatenate([fsy, (rng.integers(0, 1 << 23, 3000) * 2.0 ** -23).astype(np.float32)])
    ds, weight = env.sample_direction(_cu(np.stack([sx, sy])))
    cx, cy, fx, fy, wc, valid = E.draw(data, table, sx, sy)
    w, L, G, st = E.shade(data, table, cx, cy, fx, fy, wc, valid, R)
    assert np.array_equal(_np(ds.cell), cy * (W - 1) + cx)                    # the cell: bit for bit
    got_w, got_pdf, got_d = _np(weight), _np(ds.pdf), _np(ds.d)
    assert not got_w[~valid].any() and not got_pdf[~valid].any()              # an invalid draw: weight 0, pdf 0
    if name == "zero":
        assert not valid.any()
        return
    if name == "hole":
        assert (~valid).any() and valid.any()
    else:
        assert valid.all()
    frac = _np(ds.frac)
    assert np.array_equal(frac[0][valid].view(np.uint32), fx[valid].view(np.uint32))      # (fx, fy): bit for bit
    assert np.array_equal(frac[1][valid].view(np.uint32), fy[valid].view(np.uint32))
    print(which, rot, "direction err", np.abs(got_d - w)[:, valid].max())
    assert np.abs(got_d - w)[:, valid].max() <= 2e-6
    with np.errstate(divide="ignore"):                                          # (theta = 0 exactly: G = 0, pdf = inf on both sides)
        ref_pdf = 1.0 / np.where(valid, G, 1.0)
    bad = valid & ~(np.isclose(got_w, L * G, rtol=1e-5, atol=FLT_MIN) & np.isclose(got_pdf, ref_pdf, rtol=1e-5, atol=FLT_MIN))
    print("E / pdf mismatches", [(sx[i], sy[i], got_w[i], (L * G)[i], got_pdf[i], ref_pdf[i]) for i in np.flatnonzero(bad)[:5]])
    assert not bad.any()
    inner = valid & (np.minimum(fx, 1 - fx) > 1e-3) & (np.minimum(fy, 1 - fy) > 1e-3)
    assert inner.sum() > 1000
    # rtol 1e-4 and nothing else.  Measured on an MI355X: at most 4.5e-5 over the ten (map, rotation) pairs.  The float32
    # rounding of the direction alone accounts for it (the restatement's float64 lookup of its own direction rounded to
    # float32 is off by up to 6.6e-5 on these draws): near a pole the azimuth of a rounded direction is off by
    # 6e-8 / sin(theta), and where L falls to zero inside a cell (cell row 4 of `sun`) 1.5e-7 of a cell is 1.5e-4 of an L
    # that is 1e-3 of a cell from zero.  Where all four texels are zero both sides are exactly zero.
    ev = _np(env.eval(ds.d)).astype(np.float64)
    rel = np.abs(ev - L)[inner & (L != 0)] / np.abs(L)[inner & (L != 0)]
    print(which, rot, "eval(sample_direction) max rel err", rel.max(), "smallest |L|", np.abs(L)[inner & (L != 0)].min())
    assert np.allclose(ev[inner], L[inner], rtol=1e-4, atol=0)
    assert np.allclose(_np(env.pdf_direction(ds.d))[inner], got_pdf[inner], rtol=1e-4)


@gpu
@pytest.mark.parametrize("which", MAPS[1:], ids=_id)
def test_eval_grid_and_eval_adjoint(hf, which):
    name, u = which
    data, env = _env(hf, name, u, to_world=GENERIC_ROT)
    H, W = data.shape
    th = np.pi * np.arange(32) / 31.0                                          # both poles
    ph = 2.0 * np.pi * np.arange(64) / 64.0 + np.pi / (W - 1)                  # the seam, at phi = pi / (W - 1)
    T, P = np.meshgrid(th, ph, indexing="ij")
    local = np.stack([np.sin(T) * np.sin(P), np.cos(T), -np.sin(T) * np.cos(P)]).reshape(3, -1)
    local[:, :64] = np.array([[0.0], [1.0], [0.0]]); local[:, -64:] = np.array([[0.0], [-1.0], [0.0]])
    d = (GENERIC_ROT @ local).astype(np.float32)
    rng = np.random.default_rng(2)
    act = rng.uniform(size=d.shape[1]) < 0.9
    got = _np(env.eval(_cu(d), active=_cu(act)))
    ref = E.eval_map(data, d.astype(np.float64), GENERIC_ROT, act)
    print(which, "eval err", np.abs(got - ref).max())
    assert not got[~act].any() and np.allclose(got, ref, rtol=1e-5, atol=1e-7 * np.abs(data).max())
    go = rng.normal(size=d.shape[1]).astype(np.float32)
    acc = rng.uniform(1e-3, 2e-3, data.shape).astype(np.float32)               # a non-zero accumulator: accumulation is proven
    gd, dd, act_t, go_t = _cu(acc), _cu(d), _cu(act.astype(np.uint8)), _cu(go)
    lib = hf._capi.lib()
    hf._capi.check(lib.hf_envmap_eval_adjoint(d.shape[1], C.byref(hf.shape._p3(dd)), act_t.data_ptr(), W, H, C.byref(env._rot),
                                              go_t.data_ptr(), gd.data_ptr(), torch.cuda.current_stream().cuda_stream))
    rgd, cnt, ab = E.eval_adjoint(d.astype(np.float64), data.shape, go, GENERIC_ROT, act)
    err = np.abs((_np(gd).astype(np.float64) - acc) - rgd)
    bound = (cnt + 4) * 2.0 ** -24 * (ab + acc)                                # (the prior value is one more term of the sum)
    print(which, "eval_adjoint max err / bound", (err / bound).max())
    assert np.all(err <= bound) and np.array_equal(_np(gd)[cnt == 0], acc[cnt == 0])
    # through autograd: the seam column's gradient lands on column 0
    env.data.requires_grad_(True)
    (env.eval(dd, active=_cu(act)) * _cu(go)).sum().backward()
    assert np.all(np.abs(_np(env.data.grad).astype(np.float64) - _fold(rgd)) <= (_fold(cnt) + 5) * 2.0 ** -24 * _fold(ab))


# ---- rays, visibility ---------------------------------------------------------------------------------------------------
@gpu
def test_materialised_rays_against_the_restatement(hf, cfg):
    sc = cfg.sc
    assert np.abs(sc.np["p"]).max() < 4                                        # (what the 1e-6 on origins rests on)
    for k in range(K):
        r, wgt = cfg.rays[k]
        d, o, maxt = _np(r.d), _np(r.o), _np(r.maxt)
        w, valid = cfg.dr["w"][k], cfg.dr["valid"][k]
        assert valid.all() and np.abs(d - w).max() <= 2e-6, (k, np.abs(d - w).max())
        assert np.all((maxt == np.inf) | (maxt == -1.0))
        sure = (cfg.margin[k] > MARGIN) | ~sc.eligible
        assert sure.mean() > 0.999
        tr = maxt == np.inf
        assert np.array_equal(tr[sure], cfg.traced[k][sure]), k
        ref_o = S.spawn_origin(sc.np["p"], sc.np["n"], w)
        assert tr.any() and (~tr).any() and np.abs(o - ref_o)[:, tr].max() <= 1e-6
        assert np.allclose(_np(wgt), cfg.dr["L"][k] * cfg.dr["G"][k], rtol=1e-5, atol=0)
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(4)).to(device="cuda", dtype=torch.int32)
    r = hf.envmap_rays(sc.si, sc.ray, cfg.env, 2, seed=SEED, ray_index=ids)
    w = E.draws(cfg.data, cfg.table, _np(ids), 3, SEED, ROT)["w"][2]
    assert np.abs(_np(r.d) - w).max() <= 2e-6                                  # the samples follow the id
    same = hf.envmap_rays(sc.si, sc.ray, cfg.env, 2, seed=SEED, ray_index=torch.arange(sc.n, dtype=torch.int32, device="cuda"))
    assert torch.equal(same.d, cfg.rays[2][0].d) and torch.equal(same.o, cfg.rays[2][0].o) and torch.equal(same.maxt, cfg.rays[2][0].maxt)
    assert not torch.equal(hf.envmap_rays(sc.si, sc.ray, cfg.env, 2, seed=SEED + 1).d, cfg.rays[2][0].d)


@gpu
def test_visibility_three_ways_exactly(hf, cfg):
    """the fused word == hf_envmap_rays + ray_test in both coherence modes == the oracle's ray_test on those rays"""
    sc = cfg.sc
    vis = S.unpack(cfg.words, 32)
    assert not vis[K:].any()
    n_seen = n_traced = 0
    for k in range(K):
        r = cfg.rays[k][0]
        tr = _np(r.maxt >= 0)
        oracle_vis = np.zeros(sc.n, bool)
        oracle_vis[tr] = ~sc.field.ray_test(_rows7(r)[:, tr]).astype(bool)
        assert np.array_equal(vis[k], oracle_vis), ("fused != oracle", k, int((vis[k] != oracle_vis).sum()))
        n_seen += int(vis[k].sum()); n_traced += int(tr.sum())
        for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
            old = sc.shape.ray_coherence()
            sc.shape.set_ray_coherence(mode)
            try:
                two = _np((r.maxt >= 0) & ~sc.shape.ray_test(r))
            finally:
                sc.shape.set_ray_coherence(old)
            assert np.array_equal(two, vis[k]), ("two-call != fused", mode, k)
    valid = cfg.dr["valid"][:K] & sc.eligible[None]
    shares = {"eligible": float(sc.eligible.mean()), "valid": valid.sum() / (sc.eligible.sum() * K), "traced": n_traced / valid.sum(),
              "unoccluded": n_seen / n_traced, "undecided": float((valid & (cfg.margin[:K] <= MARGIN)).mean()),
              "max_per_texel": int(np.bincount(cfg.dr["idx"][:K][np.broadcast_to(vis[:K, None, :], cfg.dr["idx"][:K].shape)]).max())}
    check_shares(cfg.pair, shares)


# ---- image, adjoint, tangent -------------------------------------------------------------------------------------------
def _close(got, ref, S_):
    err = np.abs(got - ref)
    bound = 1e-5 * np.abs(ref) + 1e-7 * S_
    print("   max |ref|", np.abs(ref).max(), "S", S_, "max err", err.max(), "max err / bound", (err / bound).max())
    return bool(np.all(err <= bound))


def _texel_bound(got, prior, ref, cnt, ab):
    err = np.abs((got.astype(np.float64) - prior) - ref)
    bound = (cnt + 4) * 2.0 ** -24 * (ab + np.abs(prior))
    print("   grad_data max |ref|", np.abs(ref).max(), "max err / bound", (err / np.maximum(bound, 1e-300))[cnt > 0].max(initial=0))
    return bool(np.all(err <= bound))


def _adjoint_abi(hf, cfg, sn, dd, tt, ww, num_rays, spp, vis, gi, prior, ids=None):
    """hf_envmap_lighting_adjoint through the C ABI with a pre-filled grad_data: (grad_sh_n, grad_weight, grad_data)"""
    lib, p3 = hf._capi.lib(), hf.shape._p3
    n = sn.shape[1]
    W, H = cfg.env.resolution
    gn = torch.empty_like(sn); gw = torch.empty(n, device="cuda"); gd = _cu(prior)
    dat = cfg.env.full().detach().contiguous()
    hf._capi.check(lib.hf_envmap_lighting_adjoint(n, spp, C.byref(p3(sn)), C.byref(p3(dd)), tt.data_ptr(), hf.shape._ptr(ww),
                                                  num_rays, SEED, hf.shape._ptr(ids), W, H, dat.data_ptr(),
                                                  cfg.env.table().data_ptr(), C.byref(cfg.env._rot), ALBEDO, vis.data_ptr(),
                                                  gi.data_ptr(), C.byref(p3(gn)), gw.data_ptr(), gd.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    return gn, gw, gd


@gpu
@pytest.mark.parametrize("spp", [4, 3, 64, 128])
def test_image_adjoint_and_tangent_against_the_restatement(hf, cfg, spp):
    """rtol 1e-5, atol 1e-7 S with S the largest sum_k |term| of any sample: the sky row's atol of 1e-7 at its term scale
    of one, scaled to this estimator's terms; grad_data per texel within (m + 4) 2^-24 sum |terms|"""
    sc = cfg.sc
    m = sc.n - sc.n % spp
    arrs = [a[..., :m] for a in sc.arrs]
    el = sc.eligible[:m]
    for num_rays in (1, 4, 32):
        for with_weight in (False, True):
            rng = np.random.default_rng(100 * spp + num_rays)
            dr = {key: v[:num_rays, ..., :m] for key, v in cfg.dr.items()}
            si, ray = sub(hf, sc, 0, m, requires_grad=True)
            wgt = rng.uniform(0.5, 1.5, m).astype(np.float32) if with_weight else None
            wt = _cu(wgt).requires_grad_(True) if with_weight else None
            cfg.env.data.requires_grad_(True); cfg.env.data.grad = None
            img, vis = hf.envmap_lighting(sc.shape, si, ray, cfg.env, albedo=ALBEDO, spp=spp, num_rays=num_rays, seed=SEED,
                                          weight=wt, return_visibility=True)
            assert img.shape == (m // spp,) and vis.shape == (m,)
            if num_rays == K:
                assert np.array_equal(_np(vis).view(np.uint32), cfg.words[:m])
            bits = S.unpack(_np(vis), num_rays)
            ref, _, S_ = E.forward(*arrs, wgt, bits, dr, ALBEDO, spp)
            print(cfg.pair, "spp", spp, "num_rays", num_rays, "weight", with_weight, "image")
            assert ref.max() > 0 and _close(_np(img), ref, S_)
            gi = rng.normal(size=m // spp).astype(np.float32)
            (img * _cu(gi)).sum().backward()
            gn, gw, gd, cnt, ab = E.adjoint(*arrs, wgt, bits, dr, ALBEDO, spp, gi, cfg.data.shape)
            Sn, Sw = E.adjoint_scales(*arrs, wgt, bits, dr, ALBEDO, spp, gi)
            print("grad_sh_n"); got_n = _np(si.sh_frame.n.grad)
            assert np.abs(gn).max() > 0 and _close(got_n, gn, Sn) and not got_n[:, ~el].any()
            if with_weight:
                print("grad_weight"); got_w = _np(wt.grad)
                assert _close(got_w, gw, Sw) and not got_w[~el].any()
            # through autograd: zeros, the atomics, and the seam column folded onto column 0 (one more addition)
            assert np.all(np.abs(_np(cfg.env.data.grad).astype(np.float64) - _fold(gd)) <= (_fold(cnt) + 5) * 2.0 ** -24 * _fold(ab))
            # the accumulating entry itself, per texel
            prior = rng.uniform(0.5, 1.0, cfg.data.shape).astype(np.float32) * np.float32(1e-3 * np.abs(gd).max() + 1e-6)
            sn, dd, tt = (_cu(a) for a in arrs)
            an, aw, ad = _adjoint_abi(hf, cfg, sn, dd, tt, wt.detach() if with_weight else None, num_rays, spp, vis, _cu(gi), prior)
            assert torch.equal(an, si.sh_frame.n.grad)
            assert _texel_bound(_np(ad), prior, gd, cnt, ab) and np.array_equal(_np(ad)[cnt == 0], prior[cnt == 0])
            an2, aw2, _ = _adjoint_abi(hf, cfg, sn, dd, tt, wt.detach() if with_weight else None, num_rays, spp, vis, _cu(gi), prior)
            assert torch.equal(an, an2) and torch.equal(aw, aw2)                             # bitwise repeatable
            cfg.env.data.requires_grad_(False)
            dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
            dw = rng.uniform(-0.5, 0.5, m).astype(np.float32) if with_weight else None
            dda = rng.uniform(-0.5, 0.5, cfg.data[:, :-1].shape).astype(np.float32)
            tans = []
            for _ in range(2):
                with fwAD.dual_level():
                    si2, _r = sub(hf, sc, 0, m)
                    si2.sh_frame.n = fwAD.make_dual(si2.sh_frame.n, _cu(dn))
                    wd = fwAD.make_dual(wt.detach(), _cu(dw)) if with_weight else None
                    env2 = hf.Envmap(fwAD.make_dual(cfg.env.data.detach(), _cu(dda)), defensive=cfg.u)
                    out = hf.envmap_lighting(sc.shape, si2, ray, env2, albedo=ALBEDO, spp=spp, num_rays=num_rays, seed=SEED, weight=wd)
                    tans.append(fwAD.unpack_dual(out).tangent.clone())
            assert torch.equal(tans[0], tans[1])
            tref, St = E.tangent(*arrs, wgt, bits, dr, ALBEDO, spp, dn, dw, E.with_seam(dda), return_scale=True)
            print("tangent")
            assert np.abs(tref).max() > 0 and _close(_np(tans[0]), tref, St)
            # transposition on the device: <adjoint(g), (dn, dw, ddata)> = <g, tangent>, 1e-5 of the sum of absolute terms
            # (those of the adjoint side alone, as tests/test_envmap_ref.py takes them)
            parts = [_np(an).astype(np.float64) * dn, (_np(aw).astype(np.float64) * dw) if with_weight else np.zeros(1),
                     (_np(ad).astype(np.float64) - prior) * E.with_seam(dda)]
            lhs = sum(x.sum() for x in parts); rhs = (_np(tans[0]).astype(np.float64) * gi).sum()
            absum = sum(np.abs(x).sum() for x in parts)
            assert abs(lhs - rhs) <= 1e-5 * absum, (lhs, rhs, absum)


@gpu
def test_a_cut_wavefront_is_the_whole(hf, cfg):
    sc = cfg.sc
    gi = _cu(np.random.default_rng(5).normal(size=sc.n // 4).astype(np.float32))
    ids = torch.arange(sc.n, dtype=torch.int32, device="cuda")
    wt = _cu(np.random.default_rng(6).uniform(0.5, 1.5, sc.n).astype(np.float32))
    dn = _cu(np.random.default_rng(7).normal(size=(3, sc.n)).astype(np.float32))
    out = []
    for lo, hi in ((0, sc.n), (0, SPLIT), (SPLIT, sc.n)):
        si, ray = sub(hf, sc, lo, hi, requires_grad=True)
        w = wt[lo:hi].clone().requires_grad_(True)
        cfg.env.data.requires_grad_(True); cfg.env.data.grad = None
        img, vis = hf.envmap_lighting(sc.shape, si, ray, cfg.env, albedo=ALBEDO, spp=4, num_rays=K, seed=SEED, weight=w,
                                      ray_index=ids[lo:hi].contiguous(), return_visibility=True)
        (img * gi[lo // 4:hi // 4]).sum().backward()
        cfg.env.data.requires_grad_(False)
        with fwAD.dual_level():
            si2, _r = sub(hf, sc, lo, hi)
            si2.sh_frame.n = fwAD.make_dual(si2.sh_frame.n, dn[:, lo:hi].contiguous())
            tan = fwAD.unpack_dual(hf.envmap_lighting(sc.shape, si2, ray, cfg.env, albedo=ALBEDO, spp=4, num_rays=K, seed=SEED,
                                                      weight=w.detach(), ray_index=ids[lo:hi].contiguous())).tangent
        out.append((vis, img.detach(), si.sh_frame.n.grad, w.grad, tan, cfg.env.data.grad.clone()))
    whole, a, b = out
    assert np.array_equal(_np(whole[0]).view(np.uint32), cfg.words)
    for j in range(5):
        assert torch.equal(whole[j], torch.cat([a[j], b[j]], dim=-1)), j
    bits = S.unpack(cfg.words, K)
    _, _, gd, cnt, ab = E.adjoint(*sc.arrs, _np(wt), bits, _prefix(cfg.dr, K), ALBEDO, 4, _np(gi), cfg.data.shape)
    err = np.abs(_np(a[5] + b[5]).astype(np.float64) - _fold(gd))
    assert np.all(err <= (_fold(cnt) + 6) * 2.0 ** -24 * _fold(ab))              # (two sums and the fold: two more roundings)


# ---- edge cases, capture -------------------------------------------------------------------------------------------------
@gpu
def test_edge_cases_and_guards(hf, cfg):
    sc = cfg.sc
    lib, p3 = hf._capi.lib(), hf.shape._p3
    # an empty wavefront, and one that misses everything
    si0, ray0 = sub(hf, sc, 0, 0, requires_grad=True)
    img0, vis0 = hf.envmap_lighting(sc.shape, si0, ray0, cfg.env, spp=4, num_rays=K, return_visibility=True)
    assert img0.shape == (0,) and vis0.shape == (0,)
    img0.sum().backward()
    assert len(hf.envmap_rays(si0, ray0, cfg.env, 0)) == 0
    up = hf.Ray3f(sc.ray.o, -sc.ray.d)
    sim = sc.shape.ray_intersect(up, hf.RayFlags.All)
    assert not bool(sim.is_valid().any())
    imgm, vism = hf.envmap_lighting(sc.shape, sim, up, cfg.env, spp=4, num_rays=K, return_visibility=True)
    assert not bool(imgm.any()) and not bool(vism.any())
    # an all-zero map: nothing is traced, the image is exactly zero
    zero = hf.Envmap(torch.zeros_like(cfg.env.data))
    imgz, visz = hf.envmap_lighting(sc.shape, sc.si, sc.ray, zero, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    assert not bool(imgz.any()) and not bool(visz.any())
    assert bool((hf.envmap_rays(sc.si, sc.ray, zero, 1, seed=SEED).maxt == -1).all())
    with pytest.raises(hf.HfError):
        hf.envmap_lighting(sc.shape, sc.si, sc.ray, cfg.env, spp=3)
    with pytest.raises(hf.HfError):
        hf.envmap_lighting(sc.shape, sc.si, sc.ray, cfg.env, num_rays=33)
    # guard values around every output row at n = 197
    n, G = 197, 96
    start = int(torch.nonzero(sc.si.is_valid())[0]) // 64 * 64
    cut = lambda x: x.detach()[..., start:start + n].contiguous()
    p, nr, sn, d, t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.sh_frame.n), cut(sc.ray.d), cut(sc.si.t)
    W, H = cfg.env.resolution
    dat, tab, rot = cfg.env.full().detach().contiguous(), cfg.env.table(), C.byref(cfg.env._rot)
    envargs = (W, H, dat.data_ptr(), tab.data_ptr(), rot)
    stream = torch.cuda.current_stream().cuda_stream
    image, ip = guarded(n, G)
    vis = torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ids = torch.arange(start, start + n, dtype=torch.int32, device="cuda")
    hf._capi.check(lib.hf_envmap_lighting(sc.shape._h, n, 1, p3(p), p3(nr), p3(sn), p3(d), t.data_ptr(), None, K, SEED,
                                          ids.data_ptr(), *envargs, ALBEDO, ip[0], vis.data_ptr() + 4 * G, stream))
    assert intact(image, n, G) and bool((vis[:G] == 0x5A5A5A5A).all()) and bool((vis[G + n:] == 0x5A5A5A5A).all())
    assert np.array_equal(_np(vis[G:G + n]).view(np.uint32), cfg.words[start:start + n])      # the slice, with its ids
    words = vis[G:G + n].contiguous()
    gi = torch.ones(n, device="cuda")
    gn, gp = guarded(n, G, 3); gw, gwp = guarded(n, G)
    gd = torch.full((H + 2, W), GUARD, device="cuda")
    gd[1:H + 1] = 0.0
    head = (n, 1, p3(sn), p3(d), t.data_ptr(), None, K, SEED, ids.data_ptr(), *envargs, ALBEDO, words.data_ptr())
    hf._capi.check(lib.hf_envmap_lighting_adjoint(*head, gi.data_ptr(), gp, gwp[0], gd.data_ptr() + 4 * W, stream))
    assert intact(gn, n, G) and intact(gw, n, G) and bool((gd[0] == GUARD).all()) and bool((gd[H + 1] == GUARD).all())
    dimg, dp = guarded(n, G)
    hf._capi.check(lib.hf_envmap_lighting_tangent(*head, p3(sn), None, dat.data_ptr(), dp[0], stream))
    assert intact(dimg, n, G)
    ro, rop = guarded(n, G, 3); rd, rdp = guarded(n, G, 3); rm, rmp = guarded(n, G); rw, rwp = guarded(n, G)
    hf._capi.check(lib.hf_envmap_rays(n, p3(p), p3(nr), p3(sn), p3(d), t.data_ptr(), 0, SEED, ids.data_ptr(), *envargs, rop, rdp,
                                      rmp[0], rwp[0], stream))
    assert intact(ro, n, G) and intact(rd, n, G) and intact(rm, n, G) and intact(rw, n, G)
    sd, sdp = guarded(n, G, 3); sw, swp = guarded(n, G); sp, spp_ = guarded(n, G); sf, sfp = guarded(n, G, 2)
    cell = torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    smp = torch.rand((2, n), device="cuda")
    hf._capi.check(lib.hf_envmap_sample_direction(n, (hf._capi._fp * 2)(smp[0].data_ptr(), smp[1].data_ptr()), *envargs, sdp,
                                                  swp[0], spp_[0], cell.data_ptr() + 4 * G,
                                                  (hf._capi._fp * 2)(sfp[0], sfp[1]), stream))
    assert intact(sd, n, G) and intact(sw, n, G) and intact(sp, n, G) and intact(sf, n, G)
    assert bool((cell[:G] == 0x5A5A5A5A).all()) and bool((cell[G + n:] == 0x5A5A5A5A).all()) and bool((cell[G:G + n] < (W - 1) * (H - 1)).all())
    ev, evp = guarded(n, G)
    hf._capi.check(lib.hf_envmap_eval(n, p3(d), None, W, H, dat.data_ptr(), rot, evp[0], stream))
    assert intact(ev, n, G)
    gd.fill_(GUARD); gd[1:H + 1] = 0.0                          # grad_data is the one output of hf_envmap_eval_adjoint
    hf._capi.check(lib.hf_envmap_eval_adjoint(n, p3(d), None, W, H, rot, gi.data_ptr(), gd.data_ptr() + 4 * W, stream))
    assert bool((gd[0] == GUARD).all()) and bool((gd[H + 1] == GUARD).all()) and bool((gd[1:H + 1] != GUARD).all())
    assert abs(float(gd[1:H + 1].sum()) - n) <= 1e-4 * n       # (the four bilinear weights of a lane sum to one; gi = 1)
    torch.cuda.synchronize()


@gpu
def test_graph_capture_of_table_forward_and_adjoint(hf, cfg):
    sc = cfg.sc
    lib, p3 = hf._capi.lib(), hf.shape._p3
    n = sc.n
    W, H = cfg.env.resolution
    dat = cfg.env.full().detach().contiguous()
    p, nr, sn, d, t = (x.detach().contiguous() for x in (sc.si.p, sc.si.n, sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    table = torch.zeros_like(cfg.env.table())
    image = torch.zeros(n // 4, device="cuda"); vis = torch.zeros(n, dtype=torch.int32, device="cuda")
    gi = _cu(np.random.default_rng(3).normal(size=n // 4).astype(np.float32))
    gn = torch.zeros_like(sn); gw = torch.zeros(n, device="cuda"); gd = torch.zeros_like(dat)
    rot = C.byref(cfg.env._rot)

    def step(stream):
        hf._capi.check(lib.hf_envmap_build_table(W, H, dat.data_ptr(), cfg.u, table.data_ptr(), stream))
        hf._capi.check(lib.hf_envmap_lighting(sc.shape._h, n, 4, p3(p), p3(nr), p3(sn), p3(d), t.data_ptr(), None, K, SEED, None,
                                              W, H, dat.data_ptr(), table.data_ptr(), rot, ALBEDO, image.data_ptr(),
                                              vis.data_ptr(), stream))
        hf._capi.check(lib.hf_envmap_lighting_adjoint(n, 4, p3(sn), p3(d), t.data_ptr(), None, K, SEED, None, W, H, dat.data_ptr(),
                                                      table.data_ptr(), rot, ALBEDO, vis.data_ptr(), gi.data_ptr(), p3(gn),
                                                      gw.data_ptr(), gd.data_ptr(), stream))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in (table, image, vis, gn, gw)]
    assert torch.equal(table, cfg.env.table()) and np.array_equal(_np(vis).view(np.uint32), cfg.words)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        for x in (table, image, gn, gw):
            x.fill_(-1.0)
        vis.fill_(-1); gd.zero_()
        g.replay()
        torch.cuda.synchronize()
        runs.append([x.clone() for x in (table, image, vis, gn, gw)])
    for a, b, e in zip(runs[0], runs[1], eager):
        assert torch.equal(a, b) and torch.equal(a, e)
    assert bool(gd.any())


# ---- through Python ------------------------------------------------------------------------------------------------------
HEIGHTS_BOUND = 5e-7        # relative L2 of the chain to the heights (the sky row's measured figure)


@gpu
def test_gradients_through_python(hf, oracle, cfg):
    """torch.autograd.grad of a scalar loss through envmap_lighting with respect to the heights (via the surface
    interaction), envmap.data and weight against the restatement's chain (its grad_sh_n carried to the heights by the
    oracle's adjoint); forward_ad of the texels agrees with the restatement's tangent"""
    sc = cfg.sc
    shape = hf.Heightfield(heightfield=_cu(sc.h), max_height=sc.max_height, to_world=np.asarray(sc.to_world, np.float64),
                           flip_normals=sc.flip)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    rng = np.random.default_rng(11)
    wgt = rng.uniform(0.5, 1.5, sc.n).astype(np.float32)
    wt = _cu(wgt).requires_grad_(True)
    data = cfg.env.data.detach().clone().requires_grad_(True)
    env = hf.Envmap(data, defensive=cfg.u)
    img, vis = hf.envmap_lighting(shape, si, sc.ray, env, albedo=ALBEDO, spp=4, num_rays=K, seed=SEED, weight=wt,
                                  return_visibility=True)
    assert np.array_equal(_np(vis).view(np.uint32), cfg.words)
    gi = rng.normal(size=tuple(img.shape)).astype(np.float32)
    gh, gdat, gwt = torch.autograd.grad((img * _cu(gi)).sum(), (shape.heightfield, data, wt))
    bits = S.unpack(cfg.words, K)
    r = sc.rays
    t, u, v, prim = sc.field.ray_intersect_preliminary(r)
    rec = sc.field.compute_surface_interaction(r, t, u, v, prim, oracle.RAY_ALL)
    dr = _prefix(cfg.dr, K)
    gn, gw, gd, cnt, ab = E.adjoint(rec["sh_n"], r[3:6], rec["t"], wgt, bits, dr, ALBEDO, 4, gi, cfg.data.shape)
    ref_h = sc.field.adjoint(r, t, u, v, prim, {"sh_n": gn.astype(np.float32)}, oracle.RAY_ALL)
    err = np.linalg.norm(_np(gh) - ref_h) / np.linalg.norm(ref_h)
    print(cfg.pair, "dL/dheight relative L2 error", err, "norm", np.linalg.norm(ref_h))
    assert np.linalg.norm(ref_h) > 0 and err <= HEIGHTS_BOUND, err
    assert _close(_np(gwt), gw, E.adjoint_scales(rec["sh_n"], r[3:6], rec["t"], wgt, bits, dr, ALBEDO, 4, gi)[1])
    fcnt, fab = _fold(cnt), _fold(ab)                                                  # the seam column lands on column 0
    errd = np.abs(_np(gdat).astype(np.float64) - _fold(gd))
    assert gdat.shape == data.shape and np.abs(gd[:, -1]).max() > 0
    assert np.all(errd <= (fcnt + 5) * 2.0 ** -24 * fab) and not _np(gdat)[fcnt == 0].any()
    dda = rng.uniform(-0.5, 0.5, tuple(data.shape)).astype(np.float32)
    with fwAD.dual_level():
        env2 = hf.Envmap(fwAD.make_dual(data.detach(), _cu(dda)), defensive=cfg.u)
        out = hf.envmap_lighting(sc.shape, sc.si, sc.ray, env2, albedo=ALBEDO, spp=4, num_rays=K, seed=SEED)
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref, St = E.tangent(*sc.arrs, None, bits, dr, ALBEDO, 4, None, None, E.with_seam(dda), return_scale=True)
    assert np.abs(tref).max() > 0 and _close(tan, tref, St)


@gpu
def test_inverse_envmap_descends(hf):
    import inverse_envmap
    hist = inverse_envmap.run(grid=32, film=32, map_size=(17, 9), steps=30, verbose=False)
    print("inverse_envmap: loss", hist[0], "->", hist[-1], "ratio", hist[-1] / hist[0], "texel error", inverse_envmap.run.texel_error)
    assert np.isfinite(hist[-1]) and hist[-1] < hist[0]

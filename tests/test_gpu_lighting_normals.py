"""Sky, bounce and envmap lighting on the GPU (hf_sky_*, hf_bounce_*, hf_envmap_*) where the shading normal is NOT the
geometric normal: the scenes of tests/lighting_scenes.py (2300 samples, K = 4, seed 5), each with two kinds of sh_n:
  `smooth`  the shape built with face_normals = False, the records those of shape.ray_intersect; sh_n is first held to
            smooth_ref.surface to 1e-5 and n, p, t, prim_index to the flat shape's record bit for bit;
  `bent`    the flat shape's records with sh_n = normalize(n + 0.5 tau) (lighting_scenes.bent_normals: 26.6 degrees off n on
            every hit), handed over as a SurfaceInteraction3f assembled from tensors.  No smooth-shading code is involved,
            and the eligibility of 76 - 109 samples per scene differs from what n would decide.
The kernels use sh_n for eligibility, for the hemisphere test, for the bounce frame and for every cosine, and n for the
side and direction of the spawn offset alone; the bounce's second vertex is shaded with the face normal of the hit
triangle.  Where sh_n = n (every other lighting test) none of that can be told apart; here hundreds of lanes per scene
separate them (tests/test_lighting_normals.py counts them on the CPU; the floors are lighting_scenes.FLOOR_*).

Every comparison has a judge that is not the product: the oracle for what is traced, the float64 restatements
(sky_ref, bounce_ref, envmap_ref), fed with the float32 records the kernels read, for what is computed.
  (1) the materialised rays against the restatement, the origins on the far side of the facet where <n, w> < 0;
  (2) the record three ways, exactly: fused == the two-call sequence (both coherence modes) == the oracle;
  (3) image, grad_sh_n, grad_weight and tangent at spp 4 and 3 with a weight, under the rows' own bounds;
  (4) a permuted ray_index is followed (one scene, one kind).
The film stages at spp 64 and 128, graph capture, guard rows and the chain to the heights are covered by
test_gpu_lighting_scenes.py, test_gpu_sky_lighting.py, test_gpu_bounce_lighting.py and test_gpu_envmap_lighting.py.

Measured on an MI355X with the kernels' float32 records, the four directions together: exactly the counts of the table in
tests/test_lighting_normals.py, in every column and every configuration (sky traced with <n, w> < 0: 546 - 895, of those
unoccluded 34 - 268; sky not traced with <n, w> > 0: 543 - 918; bounce traced with <n, w> < 0: 402 - 1065, of those hit
243 - 1033, hits seen from behind 243 - 1033; envmap traced below 452 - 1889, of those unoccluded 21 - 222, not traced
above 224 - 837; `bent` eligibility differs on 76 - 109 samples); max |sh_n - smooth_ref| of `smooth` 4.0e-6 - 8.7e-6.

What the tests catch, each tried once on a build with that one change (none of the lighting tests from before notices
any of them):
  * `traced` from n in hf_sky_kernel: (2) fails in all eight configurations, 12 - 120 lanes of direction 0;
  * the bounce ray's origin offset along sh_n in hf_bounce_kernel: (2) fails in all eight, 101 - 262 lanes of direction 0;
  * n and sh_n exchanged in the forward call of envmap_lighting: (2) fails in all twelve envmap configurations (8 - 80
    lanes of direction 0) and (3) in all twenty-four;
  * either of the first two made in the rays kernel as well (so that fused and two-call agree): (1) and (2) fail in all eight;
  * the sky forward's cosine taken with n: (3) fails in all sixteen.
"""
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import bounce_ref as B
import envmap_ref as E
import lighting_scenes as LS
import sky_ref as S
from lighting_scenes import K, MARGIN, MISS, SEED, _close, _np, _records, _rows7
from row_helpers import _cu, sub
from test_gpu_envmap_lighting import _close as _close_env, _fold

pytestmark = pytest.mark.gpu

CONFIGS = [(s, k) for s in LS.NAMES for k in LS.KINDS]
ENV_CONFIGS = [(s, k, m, u) for s in LS.ENV_SCENES for k in LS.KINDS for m, u in LS.ENV_MAPS]
ROT = E.DEFAULT_ROT
ALBEDO = 0.7
_BUILT, _ENV = {}, {}


def _id(p):
    return "-".join(str(x) for x in p)


@pytest.fixture(scope="module", params=CONFIGS, ids=_id)
def cfg(request, hf, oracle):
    return _scene(hf, oracle, *request.param)


@pytest.fixture(scope="module", params=ENV_CONFIGS, ids=_id)
def ecfg(request, hf, oracle):
    return _env(hf, oracle, *request.param)


def _scene(hf, oracle, name, kind):
    """(scene, kind) on the GPU with its two-call sequences and fused records, built once per module"""
    if (name, kind) not in _BUILT:
        _BUILT[name, kind] = _build(hf, oracle, name, kind)
    return _BUILT[name, kind]


def _build(hf, oracle, name, kind):
    sc = LS.scene(name)
    sc.kind = kind
    sc.tw64 = np.asarray(sc.to_world, np.float64)
    mk = lambda fn: hf.Heightfield(heightfield=_cu(sc.h), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                                   face_normals=fn)
    rt = _cu(sc.rays)
    sc.ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
    flat = mk(True)
    fsi = flat.ray_intersect(sc.ray, hf.RayFlags.All)
    sc.hit = _np(fsi.is_valid())
    sc.field = LS.oracle_field(sc, oracle)
    t, _, _, prim = sc.field.ray_intersect_preliminary(sc.rays)
    fprim = _np(fsi.prim_index).view(np.uint32)
    assert np.array_equal(sc.hit, np.isfinite(t)) and np.array_equal(fprim[sc.hit], prim[sc.hit])
    if kind == "smooth":
        sc.shape = mk(False)
        si = sc.shape.ray_intersect(sc.ray, hf.RayFlags.All)
        # a failure names its side: the record but for the shading frame is the flat shape's, sh_n is the restatement's
        for key in ("n", "p", "t", "prim_index"):
            assert torch.equal(getattr(si, key), getattr(fsi, key)), ("not the flat record", key)
        ref = LS.smooth_normals(sc, sc.rays, fprim, sc.hit)
        err = np.abs(_np(si.sh_frame.n) - ref)[:, sc.hit].max()
        print(name, "smooth: max |sh_n - smooth_ref|", err)
        assert err <= 1e-5, err
    else:
        sc.shape = flat
        si = hf.SurfaceInteraction3f()
        si.p, si.n, si.t = fsi.p.detach(), fsi.n.detach(), fsi.t.detach()
        si.sh_frame = hf.Frame3f(None, None, _cu(LS.bent_normals(_np(fsi.n), sc.hit)))
    sc.si = si
    sc.lt = torch.from_numpy(sc.lights)
    sc.np = {k: _np(v) for k, v in (("p", si.p), ("n", si.n), ("sh_n", si.sh_frame.n), ("d", sc.ray.d), ("t", si.t))}
    sc.arrs = [sc.np[k] for k in ("sh_n", "d", "t")]
    ids = np.arange(sc.n)
    sc.w, sc.z = B.directions(sc.np["sh_n"], ids, K, SEED)                # [K, 3, n], [K, n]
    sc.ws = S.directions(ids, K, SEED)
    sc.eligible, elm = S.eligible(*sc.arrs)
    sc.eligible_n, _ = S.eligible(sc.np["n"], sc.np["d"], sc.np["t"])
    sc.el_sure = (elm > MARGIN) | ~sc.hit                                 # eligibility is not decided by a rounding
    sc.traced = B.traced(*sc.arrs, sc.z)
    sc.straced, sc.smargin = S.traced(*sc.arrs, sc.ws)
    # the two-call sequences, once for all tests
    sc.brays = [hf.bounce_rays(sc.shape, si, sc.ray, k, seed=SEED) for k in range(K)]
    sc.si2 = [sc.shape.ray_intersect(r, hf.RayFlags.All) for r in sc.brays]
    sc.srays = [[hf.bounce_rays(sc.shape, si, sc.ray, k, seed=SEED, to_light=sc.lights[l, :3]) for l in range(sc.L)] for k in range(K)]
    sc.sky_rays = [hf.sky_rays(si, sc.ray, k, seed=SEED) for k in range(K)]
    # the fused records
    _, prim, lit = hf.bounce_lighting(sc.shape, si, sc.ray, sc.lt, spp=4, num_rays=K, seed=SEED, return_records=True)
    sc.prim, sc.lit = _np(prim).view(np.uint32), _np(lit)
    _, vis = hf.sky_lighting(sc.shape, si, sc.ray, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    sc.words = _np(vis).view(np.uint32)
    return sc


def _env(hf, oracle, scene, kind, name, u):
    if (scene, kind, name, u) not in _ENV:
        sc = _scene(hf, oracle, scene, kind)
        c = types.SimpleNamespace(sc=sc, name=name, u=u, pair=(scene, kind, name, u))
        c.data = E.MAPS[name]()
        c.env = hf.Envmap(_cu(c.data[:, :-1]), defensive=u)
        c.table = _np(c.env.table())                                      # the DEVICE's table: the restatement draws the same cells
        c.dr = E.draws(c.data, c.table, np.arange(sc.n), K, SEED, ROT)
        c.traced, c.margin = E.traced(*sc.arrs, c.dr)
        c.rays = [hf.envmap_rays(sc.si, sc.ray, c.env, k, seed=SEED) for k in range(K)]
        _, vis = hf.envmap_lighting(sc.shape, sc.si, sc.ray, c.env, spp=4, num_rays=K, seed=SEED, return_visibility=True)
        c.words = _np(vis).view(np.uint32)
        _ENV[scene, kind, name, u] = c
    return _ENV[scene, kind, name, u]


# ---- (1) the materialised rays ---------------------------------------------------------------------------------------
def _check_ray(sc, r, w, want, sure, what):
    """one materialised ray of every sample against the restatement: direction w [3, n], traced mask `want` on the lanes
    `sure`, origins spawn_origin(p, n, w) with the GEOMETRIC normal.  Returns (traced, traced with <n, w> < -MARGIN,
    not traced with <n, w> > MARGIN among the eligible)"""
    d, o, maxt = _np(r.d), _np(r.o).astype(np.float64), _np(r.maxt)
    p, n = sc.np["p"].astype(np.float64), sc.np["n"].astype(np.float64)
    assert np.abs(d - w).max() <= 2e-6, (what, np.abs(d - w).max())
    assert np.all((maxt == np.inf) | (maxt == -1.0))
    assert sure.mean() > 0.999, (what, sure.mean())
    tr = maxt == np.inf
    assert np.array_equal(tr[sure], want[sure]), (what, int((tr != want)[sure].sum()))
    cg = (n * w).sum(0)
    ref = S.spawn_origin(p, n, w)
    err, err_other = np.abs(o - ref).max(0), np.abs(o - (2.0 * p - ref)).max(0)
    decided = np.abs(cg) > MARGIN                                          # the side of the offset is not decided by a rounding
    assert (tr & decided).mean() > 0.999 * tr.mean()
    assert tr.any() and (~tr).any() and err[tr & decided].max() <= 1e-6, (what, err[tr & decided].max())
    assert np.minimum(err, err_other)[tr & ~decided].max(initial=0.0) <= 1e-6
    below = tr & (cg < -MARGIN)
    assert np.all(((o - p) * n).sum(0)[below] < 0), what                   # the far side of the facet
    if sc.kind == "bent":                                                  # what n alone would shade is not traced
        flipped = sc.eligible_n & ~sc.eligible & sc.el_sure
        assert not tr[flipped].any(), what
    return tr, below, sc.eligible & sc.el_sure & ~tr & (cg > MARGIN)


def test_materialised_rays_against_the_restatement(hf, cfg):
    sc = cfg
    assert np.abs(sc.np["p"]).max() < 4                                    # (what the 1e-6 on origins rests on)
    n_below = {"bounce": 0, "sky": 0}
    n_above = 0
    for k in range(K):
        # bounce ray k: the frame is sh_n's
        sure = sc.el_sure & ((sc.z[k] > MARGIN) | ~sc.eligible)
        tr, below, _ = _check_ray(sc, sc.brays[k], sc.w[k], sc.traced[k], sure, ("bounce", k))
        n_below["bounce"] += int(below.sum())
        # the shadow rays from the two-call sequence's second vertex: the face normal of the hit triangle
        d = _np(sc.brays[k].d).astype(np.float64)
        valid = _np(sc.si2[k].is_valid())
        p2, n2 = _np(sc.si2[k].p).astype(np.float64), _np(sc.si2[k].n).astype(np.float64)
        nq = LS.normals_of(sc, _np(sc.si2[k].prim_index), valid)
        assert np.abs(p2).max() < 4 and np.abs(n2 - nq)[:, valid].max() <= 2e-6
        cw = (nq * d).sum(0)
        front = valid & (-cw > 0)
        want, margin = B.shadow_traced(front[None], nq[None], sc.lights)
        for l in range(sc.L):
            s = sc.srays[k][l]
            sd, so, smaxt = _np(s.d), _np(s.o), _np(s.maxt)
            assert np.abs(sd - sc.lights[l, :3, None]).max() == 0
            assert np.all((smaxt == np.inf) | (smaxt == -1.0))
            sure = ~valid | ((np.abs(cw) > MARGIN) & (margin[0, l] > MARGIN))
            assert sure.mean() > 0.999
            st = smaxt == np.inf
            assert np.array_equal(st[sure], want[0, l][sure]), (k, l)
            ref_o = B.spawn_origin(p2, nq, np.broadcast_to(sc.lights[l, :3, None].astype(np.float64), p2.shape))
            assert st.any() and np.abs(so - ref_o)[:, st].max() <= 1e-6, (k, l, np.abs(so - ref_o)[:, st].max())
        # sky ray k
        sure = sc.el_sure & ((sc.smargin[k] > MARGIN) | ~sc.eligible)
        tr, below, above = _check_ray(sc, sc.sky_rays[k], sc.ws[k], sc.straced[k], sure, ("sky", k))
        n_below["sky"] += int(below.sum()); n_above += int(above.sum())
    flips = int((sc.eligible != sc.eligible_n).sum())
    print(sc.name, sc.kind, "traced with <n, w> < 0:", n_below, "sky not traced with <n, w> > 0:", n_above, "eligibility differs:", flips)
    assert n_below["bounce"] >= LS.FLOOR_BELOW and n_below["sky"] >= LS.FLOOR_BELOW and n_above >= LS.FLOOR_ABOVE
    if sc.kind == "bent":
        assert flips >= LS.FLOOR_ELIGIBILITY and (sc.eligible_n & ~sc.eligible & sc.el_sure).sum() >= LS.FLOOR_ELIGIBILITY


def test_materialised_envmap_rays_against_the_restatement(hf, ecfg):
    c, sc = ecfg, ecfg.sc
    n_below = n_above = 0
    for k in range(K):
        valid = c.dr["valid"][k]
        sure = sc.el_sure & ((c.margin[k] > MARGIN) | ~sc.eligible | ~valid)
        tr, below, above = _check_ray(sc, c.rays[k], c.dr["w"][k], c.traced[k], sure, ("envmap", k))
        n_below += int(below.sum()); n_above += int((above & valid).sum())
    print(c.pair, "traced with <n, w> < 0:", n_below, "not traced with <n, w> > 0:", n_above)
    assert n_below >= LS.FLOOR_BELOW and n_above >= LS.FLOOR_ABOVE


# ---- (2) the record, three ways --------------------------------------------------------------------------------------
def _both_modes(hf, shape, fn):
    """fn() in both coherence modes"""
    out = []
    for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
        old = shape.ray_coherence()
        shape.set_ray_coherence(mode)
        try:
            out.append((mode, fn()))
        finally:
            shape.set_ray_coherence(old)
    return out


def _shadow_three_ways(hf, sc, rays, vis, what):
    """the fused visibility bits `vis` [K, n] == ray_test on the materialised rays in both coherence modes == the oracle's
    ray_test; returns (traced-below and unoccluded, traced-below and occluded)"""
    n64 = sc.np["n"].astype(np.float64)
    seen = hidden = 0
    for k in range(K):
        r = rays[k]
        tr = _np(r.maxt >= 0)
        oracle_vis = np.zeros(sc.n, bool)
        oracle_vis[tr] = ~sc.field.ray_test(_rows7(r)[:, tr]).astype(bool)
        assert np.array_equal(vis[k], oracle_vis), ("fused != oracle", what, k, int((vis[k] != oracle_vis).sum()))
        for mode, two in _both_modes(hf, sc.shape, lambda: _np((r.maxt >= 0) & ~sc.shape.ray_test(r))):
            assert np.array_equal(two, oracle_vis), ("two-call != oracle", what, mode, k, int((two != oracle_vis).sum()))
        below = tr & ((n64 * _np(r.d)).sum(0) < -MARGIN)
        seen += int((below & oracle_vis).sum()); hidden += int((below & ~oracle_vis).sum())
    print(sc.name, sc.kind, what, "traced with <n, w> < 0: unoccluded", seen, "occluded", hidden)
    assert seen >= LS.FLOOR_OUTCOME and hidden >= LS.FLOOR_OUTCOME       # both outcomes occur below the facet
    return seen, hidden


def test_record_three_ways_exactly(hf, cfg):
    """the fused kernels' hit_prim / lit_bits / vis_bits == the two-call sequence in both coherence modes == the oracle
    on the materialised rays.  The oracle is the judge: each side is compared with it, so a difference names its side."""
    sc = cfg
    hit, lit = B.unpack(sc.prim, sc.lit, 8)
    assert not lit[:, sc.L:].any()                                         # no bit at or above n_lights
    vis = S.unpack(sc.words, 32)
    assert not vis[K:].any()
    n64 = sc.np["n"].astype(np.float64)
    n_back = n_below = n_below_hit = 0
    for k in range(K):
        r = sc.brays[k]
        tr = _np(r.maxt >= 0)
        t, _, _, prim = sc.field.ray_intersect_preliminary(_rows7(r)[:, tr])
        oracle_prim = np.full(sc.n, MISS, np.uint32)
        oracle_prim[np.flatnonzero(tr)[np.isfinite(t)]] = prim[np.isfinite(t)]
        assert np.array_equal(sc.prim[k], oracle_prim), ("fused != oracle", k, int((sc.prim[k] != oracle_prim).sum()))
        d = _np(r.d).astype(np.float64)
        below = tr & ((n64 * d).sum(0) < -MARGIN)
        n_below += int(below.sum()); n_below_hit += int((below & hit[k]).sum())
        # n_q is the face normal of the RECORDED triangle (whatever face_normals says): a hit seen from behind -- now most
        # hits of the rays that leave below the facet -- is recorded and carries no light
        nq = LS.normals_of(sc, sc.prim[k], hit[k])
        assert np.abs(_np(sc.si2[k].n) - nq)[:, hit[k]].max() <= 2e-6
        cw = (nq * d).sum(0)
        n_back += int((hit[k] & (cw > MARGIN)).sum())
        assert not lit[k][:, hit[k] & (cw > MARGIN)].any()
        oracle_lit = np.zeros((sc.L, sc.n), bool)
        for l in range(sc.L):
            s = sc.srays[k][l]
            st = _np(s.maxt >= 0)
            oracle_lit[l, st] = ~sc.field.ray_test(_rows7(s)[:, st]).astype(bool)
            assert np.array_equal(lit[k, l], oracle_lit[l]), ("fused != oracle", k, l, int((lit[k, l] != oracle_lit[l]).sum()))
        # the two-call sequence, in both coherence modes
        def two_call():
            pi = sc.shape.ray_intersect_preliminary(r)
            return (np.where(_np(pi.is_valid()), _np(pi.prim_index).view(np.uint32), np.uint32(MISS)),
                    [_np((s.maxt >= 0) & ~sc.shape.ray_test(s)) for s in sc.srays[k]])
        for mode, (two, two_lit) in _both_modes(hf, sc.shape, two_call):
            assert np.array_equal(two, oracle_prim), ("two-call != oracle", mode, k, int((two != oracle_prim).sum()))
            for l in range(sc.L):
                assert np.array_equal(two_lit[l], oracle_lit[l]), ("two-call != oracle", mode, k, l)
    print(sc.name, sc.kind, "bounce traced with <n, w> < 0:", n_below, "of those hit:", n_below_hit, "hits seen from behind:", n_back,
          "lit records", lit.sum((0, 2))[:sc.L])
    assert n_below >= LS.FLOOR_BELOW and n_below_hit >= LS.FLOOR_BOUNCE_HIT and n_back >= LS.FLOOR_BEHIND
    assert np.all(lit.sum((0, 2))[:sc.L] > 0)
    _shadow_three_ways(hf, sc, sc.sky_rays, vis, "sky")


def test_envmap_visibility_three_ways_exactly(hf, ecfg):
    vis = S.unpack(ecfg.words, 32)
    assert not vis[K:].any()
    _shadow_three_ways(hf, ecfg.sc, ecfg.rays, vis, "envmap " + _id(ecfg.pair[2:]))


# ---- (3) image, adjoint, tangent -------------------------------------------------------------------------------------
SPPS = [4, 3]              # the tree film; one atomic per sample


def _shaded(sc, m):
    """(eligible [m], the samples whose gradients are exact zeros)"""
    el = sc.eligible[:m]
    assert (~el).any()
    if sc.kind == "bent":                                                  # ... the samples that n alone would shade among them
        assert (sc.eligible_n[:m] & ~el).sum() >= LS.FLOOR_ELIGIBILITY
    return el


@pytest.mark.parametrize("spp", SPPS)
def test_bounce_image_adjoint_and_tangent_against_the_restatement(hf, cfg, spp):
    """Values are at most 1 by the sizes of the inputs, not by a run: a sample's value under one light is at most
    weight_max albedo (albedo/pi) E <= 1.5 * 0.7 * 0.7 / pi = 0.23."""
    sc = cfg
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    rng = np.random.default_rng(100 * spp + 4)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32)
    wt = _cu(wgt).requires_grad_(True)
    img, prim, lit = hf.bounce_lighting(sc.shape, si, ray, sc.lt, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wt,
                                        return_records=True)
    assert img.shape == (sc.L, m // spp) and prim.shape == (K, m) and lit.shape == (K, m)
    # the record proven equal to the oracle by test_record_three_ways_exactly
    assert np.array_equal(_np(prim).view(np.uint32), sc.prim[:, :m]) and np.array_equal(_np(lit), sc.lit[:, :m])
    hit, lt = _records(prim, lit, sc.L)
    nq = np.stack([LS.normals_of(sc, sc.prim[k, :m], hit[k]) for k in range(K)])
    arrs = [a[..., :m] for a in sc.arrs]
    w, z = sc.w[:, :, :m], sc.z[:, :m]
    ref, _, absum = B.forward(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp)
    print(sc.name, sc.kind, "spp", spp, "image")
    assert np.all(ref.max(1) > 0) and 0.002 < ref.max() <= 1.0 and _close(_np(img), ref, absum, K)   # (every light's row is lit)
    gi = rng.normal(size=(sc.L, m // spp)).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    adj = B.adjoint(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp, w, z, gi)
    el = _shaded(sc, m)
    got_n, got_w = _np(si.sh_frame.n.grad), _np(wt.grad)
    print("grad_sh_n")
    assert np.abs(adj["grad_sh_n"]).max() > 0 and _close(got_n, adj["grad_sh_n"], adj["abs_sh_n"], K)
    print("grad_weight")
    assert _close(got_w, adj["grad_weight"], adj["abs_weight"], K)
    assert not got_n[:, ~el].any() and not got_w[~el].any()               # exact zeros
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32)
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), _cu(dn))
        out = hf.bounce_lighting(sc.shape, si, ray, sc.lt, albedo=albedo, spp=spp, num_rays=K, seed=SEED,
                                 weight=fwAD.make_dual(wt.detach(), _cu(dw)))
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref, tabs = B.tangent(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp, w, z, dn, dw)
    print("tangent")
    assert tan.shape == (sc.L, m // spp) and np.abs(tref).max() > 0 and _close(tan, tref, tabs, K)


@pytest.mark.parametrize("spp", SPPS)
def test_sky_image_adjoint_and_tangent_against_the_restatement(hf, cfg, spp):
    """rtol 1e-5, atol 1e-7, the inputs sized so that |value| <= 1 (tests/test_gpu_sky_lighting.py)"""
    sc = cfg
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    L = 1.0 / (4.0 * albedo * wmax)
    rng = np.random.default_rng(100 * spp + 8)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32)
    wt = _cu(wgt).requires_grad_(True)
    img, vis = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wt,
                               return_visibility=True)
    assert img.shape == (m // spp,) and vis.shape == (m,)
    assert np.array_equal(_np(vis).view(np.uint32), sc.words[:m])        # the word proven equal to the oracle
    bits = S.unpack(_np(vis), K)
    arrs = [a[..., :m] for a in sc.arrs]
    w = sc.ws[:, :, :m]
    ref, _ = S.forward(*arrs, wgt, bits, w, L, albedo, spp)
    got = _np(img)
    print(sc.name, sc.kind, "spp", spp, "image: max", ref.max(), "err", np.abs(got - ref).max())
    assert 0.02 < ref.max() <= 1.0 and np.allclose(got, ref, rtol=1e-5, atol=1e-7), np.abs(got - ref).max()
    gi = rng.normal(size=m // spp).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    gn, gw = S.adjoint(*arrs, wgt, bits, w, L, albedo, spp, gi)
    got_n, got_w = _np(si.sh_frame.n.grad), _np(wt.grad)
    print("grad_sh_n: max", np.abs(gn).max(), "err", np.abs(got_n - gn).max(), "grad_weight: err", np.abs(got_w - gw).max())
    assert np.abs(gn).max() > 0 and np.allclose(got_n, gn, rtol=1e-5, atol=1e-7), np.abs(got_n - gn).max()
    assert np.allclose(got_w, gw, rtol=1e-5, atol=1e-7), np.abs(got_w - gw).max()
    el = _shaded(sc, m)
    assert not got_n[:, ~el].any() and not got_w[~el].any()               # exact zeros
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32)
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), _cu(dn))
        out = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=K, seed=SEED,
                              weight=fwAD.make_dual(wt.detach(), _cu(dw)))
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref = S.tangent(*arrs, wgt, bits, w, L, albedo, spp, dn, dw)
    print("tangent: max", np.abs(tref).max(), "err", np.abs(tan - tref).max())
    assert np.abs(tref).max() > 0 and np.allclose(tan, tref, rtol=1e-5, atol=1e-7), np.abs(tan - tref).max()


@pytest.mark.parametrize("spp", SPPS)
def test_envmap_image_adjoint_and_tangent_against_the_restatement(hf, ecfg, spp):
    """the bounds of tests/test_gpu_envmap_lighting.py: rtol 1e-5, atol 1e-7 S with S the largest sum_k |term| of any
    sample; the texels' gradient through autograd (the seam column folded onto column 0) per texel within
    (m + 5) 2^-24 sum |terms|"""
    c, sc = ecfg, ecfg.sc
    m = sc.n - sc.n % spp
    arrs = [a[..., :m] for a in sc.arrs]
    dr = {key: v[..., :m] for key, v in c.dr.items()}
    rng = np.random.default_rng(100 * spp + K)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, 1.5, m).astype(np.float32)
    wt = _cu(wgt).requires_grad_(True)
    c.env.data.requires_grad_(True); c.env.data.grad = None
    try:
        img, vis = hf.envmap_lighting(sc.shape, si, ray, c.env, albedo=ALBEDO, spp=spp, num_rays=K, seed=SEED, weight=wt,
                                      return_visibility=True)
        assert img.shape == (m // spp,) and vis.shape == (m,)
        assert np.array_equal(_np(vis).view(np.uint32), c.words[:m])     # the word proven equal to the oracle
        bits = S.unpack(_np(vis), K)
        ref, _, S_ = E.forward(*arrs, wgt, bits, dr, ALBEDO, spp)
        print(c.pair, "spp", spp, "image")
        assert ref.max() > 0 and _close_env(_np(img), ref, S_)
        gi = rng.normal(size=m // spp).astype(np.float32)
        (img * _cu(gi)).sum().backward()
        got_d = _np(c.env.data.grad).astype(np.float64)
    finally:
        c.env.data.requires_grad_(False); c.env.data.grad = None
    gn, gw, gd, cnt, ab = E.adjoint(*arrs, wgt, bits, dr, ALBEDO, spp, gi, c.data.shape)
    Sn, Sw = E.adjoint_scales(*arrs, wgt, bits, dr, ALBEDO, spp, gi)
    el = _shaded(sc, m)
    got_n, got_w = _np(si.sh_frame.n.grad), _np(wt.grad)
    print("grad_sh_n")
    assert np.abs(gn).max() > 0 and _close_env(got_n, gn, Sn)
    print("grad_weight")
    assert _close_env(got_w, gw, Sw)
    assert not got_n[:, ~el].any() and not got_w[~el].any()               # exact zeros
    assert np.abs(gd).max() > 0 and np.all(np.abs(got_d - _fold(gd)) <= (_fold(cnt) + 5) * 2.0 ** -24 * _fold(ab))
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32)
    dda = rng.uniform(-0.5, 0.5, c.data[:, :-1].shape).astype(np.float32)
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), _cu(dn))
        env2 = hf.Envmap(fwAD.make_dual(c.env.data.detach(), _cu(dda)), defensive=c.u)
        out = hf.envmap_lighting(sc.shape, si, ray, env2, albedo=ALBEDO, spp=spp, num_rays=K, seed=SEED,
                                 weight=fwAD.make_dual(wt.detach(), _cu(dw)))
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref, St = E.tangent(*arrs, wgt, bits, dr, ALBEDO, spp, dn, dw, E.with_seam(dda), return_scale=True)
    print("tangent")
    assert np.abs(tref).max() > 0 and _close_env(tan, tref, St)


# ---- (4) ray_index ---------------------------------------------------------------------------------------------------
def test_a_permuted_ray_index_is_followed(hf, oracle):
    """the records of a launch with permuted ids are those of the two-call sequence with the same ids, and not the
    position-indexed records"""
    c = _env(hf, oracle, "affine", "bent", *LS.ENV_MAPS[0])
    sc = c.sc
    ids = torch.randperm(sc.n, generator=torch.Generator().manual_seed(4)).to(device="cuda", dtype=torch.int32)
    _, prim, lit = hf.bounce_lighting(sc.shape, sc.si, sc.ray, sc.lt, spp=4, num_rays=K, seed=SEED, ray_index=ids, return_records=True)
    _, sky = hf.sky_lighting(sc.shape, sc.si, sc.ray, spp=4, num_rays=K, seed=SEED, ray_index=ids, return_visibility=True)
    _, env = hf.envmap_lighting(sc.shape, sc.si, sc.ray, c.env, spp=4, num_rays=K, seed=SEED, ray_index=ids, return_visibility=True)
    prim = _np(prim).view(np.uint32)
    _, lit = B.unpack(prim, _np(lit), sc.L)
    sky, env = S.unpack(_np(sky), K), S.unpack(_np(env), K)
    for k in range(K):
        r = hf.bounce_rays(sc.shape, sc.si, sc.ray, k, seed=SEED, ray_index=ids)
        pi = sc.shape.ray_intersect_preliminary(r)
        two = np.where(_np(pi.is_valid()), _np(pi.prim_index).view(np.uint32), np.uint32(MISS))
        assert np.array_equal(prim[k], two), ("bounce", k, int((prim[k] != two).sum()))
        for l in range(sc.L):
            s = hf.bounce_rays(sc.shape, sc.si, sc.ray, k, seed=SEED, ray_index=ids, to_light=sc.lights[l, :3])
            two = _np((s.maxt >= 0) & ~sc.shape.ray_test(s))
            assert np.array_equal(lit[k, l], two), ("shadow", k, l, int((lit[k, l] != two).sum()))
        for what, got, r in (("sky", sky, hf.sky_rays(sc.si, sc.ray, k, seed=SEED, ray_index=ids)),
                             ("envmap", env, hf.envmap_rays(sc.si, sc.ray, c.env, k, seed=SEED, ray_index=ids))):
            two = _np((r.maxt >= 0) & ~sc.shape.ray_test(r))
            assert np.array_equal(got[k], two), (what, k, int((got[k] != two).sum()))
    assert (prim != sc.prim).mean() > 0.02 and (sky != S.unpack(sc.words, K)).mean() > 0.02
    assert (env != S.unpack(c.words, K)).mean() > 0.02

"""Sky and bounce lighting on the GPU (hf_sky_*, hf_bounce_*) on the four scenes of tests/lighting_scenes.py: a general
affine to_world, a mirror with flip_normals, flip_normals seen from below, and 8 lights over a small random field;
rectangular grids, 1 / 3 / 8 lights, 2300 samples (partial last wave and workgroup), K = 4, seed 5.  The methods and
bounds are those of tests/test_gpu_sky_lighting.py and tests/test_gpu_bounce_lighting.py; every comparison has a judge
that is not the product: the oracle built with the same to_world and flip_normals for what is traced, the float64
restatements (tests/sky_ref.py, tests/bounce_ref.py, held against the oracle and central differences on the CPU by
tests/test_lighting_scenes.py) for what is computed.
  (1) the materialised rays against the restatement;
  (2) the record three ways, exactly: fused == the two-call sequence (both coherence modes) == the oracle;
  (3) image, grad_sh_n, grad_weight and tangent at spp 4, 3, 64 and 128 (quad, atomic, cross-lane and several-waves film
      stages; the PIXEL tangent), with n_q from bounce_ref.face_normal of the recorded triangles;
  (4) grad_heights and the height tangent of the bounce, the chain of both rows to the heights;
  (5) global ids: a wavefront cut in two equals the whole bit for bit, and permuted ids are followed by every kernel;
  (6) repeatability."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import bounce_ref as B
import lighting_scenes as LS
import sky_ref as S
from lighting_scenes import K, MARGIN, MISS, SEED, SPLIT, _close, _np, _records, _rows7
from row_helpers import _cu, sub

pytestmark = pytest.mark.gpu


_BUILT = {}


@pytest.fixture(scope="module", params=LS.NAMES)
def scene(request, hf, oracle):
    return _scene(hf, oracle, request.param)


def _scene(hf, oracle, name):
    """the scene on the GPU with its two-call sequences and fused records, built once per module"""
    if name not in _BUILT:
        _BUILT[name] = _build(hf, oracle, name)
    return _BUILT[name]


def _build(hf, oracle, name):
    sc = LS.scene(name)
    sc.ht = torch.from_numpy(sc.h).cuda()
    sc.tw64 = np.asarray(sc.to_world, np.float64)
    sc.shape = hf.Heightfield(heightfield=sc.ht, max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip)
    rt = torch.from_numpy(sc.rays).cuda()
    sc.ray = hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())
    sc.si = si = sc.shape.ray_intersect(sc.ray, hf.RayFlags.All)
    sc.lt = torch.from_numpy(sc.lights)
    sc.np = {k: _np(v) for k, v in (("p", si.p), ("n", si.n), ("sh_n", si.sh_frame.n), ("d", sc.ray.d), ("t", si.t))}
    sc.arrs = [sc.np[k] for k in ("sh_n", "d", "t")]
    ids = np.arange(sc.n)
    sc.w, sc.z = B.directions(sc.np["sh_n"], ids, K, SEED)                # [K, 3, n], [K, n]
    sc.ws = S.directions(ids, K, SEED)
    sc.eligible, _ = B.eligible(*sc.arrs)
    sc.traced = B.traced(*sc.arrs, sc.z)
    sc.straced, sc.smargin = S.traced(*sc.arrs, sc.ws)
    sc.field = LS.oracle_field(sc, oracle)
    # the two-call sequences, once for all tests
    sc.brays = [hf.bounce_rays(sc.shape, si, sc.ray, k, seed=SEED) for k in range(K)]
    sc.si2 = [sc.shape.ray_intersect(r, hf.RayFlags.All) for r in sc.brays]
    sc.srays = [[hf.bounce_rays(sc.shape, si, sc.ray, k, seed=SEED, to_light=sc.lights[l, :3]) for l in range(sc.L)] for k in range(K)]
    sc.sky_rays = [hf.sky_rays(si, sc.ray, k, seed=SEED) for k in range(K)]
    # the fused records
    _, prim, lit = hf.bounce_lighting(sc.shape, si, sc.ray, sc.lt, spp=4, num_rays=K, seed=SEED, return_records=True)
    sc.prim_t, sc.lit_t = prim, lit
    sc.prim, sc.lit = _np(prim).view(np.uint32), _np(lit)
    _, vis = hf.sky_lighting(sc.shape, si, sc.ray, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    sc.vis_t, sc.words = vis, _np(vis).view(np.uint32)
    return sc


def _nq(sc, prim, hit):
    """[K, 3, m] float64: the restatement's face normals of the recorded triangles (never a second product call)"""
    return np.stack([LS.normals_of(sc, prim[k], hit[k]) for k in range(len(prim))])


# ---- (1) the materialised rays ---------------------------------------------------------------------------------------
def test_materialised_rays_against_the_restatement(hf, scene):
    sc = scene
    assert np.abs(sc.np["p"]).max() < 4                                    # (what the 1e-6 on origins rests on)
    for k in range(K):
        # bounce ray k
        r = sc.brays[k]
        d, o, maxt = _np(r.d), _np(r.o), _np(r.maxt)
        assert np.abs(d - sc.w[k]).max() <= 2e-6, (k, np.abs(d - sc.w[k]).max())
        assert np.all((maxt == np.inf) | (maxt == -1.0))
        sure = (sc.z[k] > MARGIN) | ~sc.eligible
        assert sure.mean() > 0.999
        tr = maxt == np.inf
        assert np.array_equal(tr[sure], sc.traced[k][sure]), k
        ref_o = B.spawn_origin(sc.np["p"], sc.np["n"], sc.w[k])
        assert tr.any() and (~tr).any() and np.abs(o - ref_o)[:, tr].max() <= 1e-6, (k, np.abs(o - ref_o)[:, tr].max())
        # the shadow rays from the two-call sequence's second vertex
        p2, n2 = _np(sc.si2[k].p).astype(np.float64), _np(sc.si2[k].n).astype(np.float64)
        assert np.abs(p2).max() < 4
        valid = _np(sc.si2[k].is_valid())
        cw = (n2 * d.astype(np.float64)).sum(0)
        front = valid & (-cw > 0)
        want, margin = B.shadow_traced(front[None], n2[None], sc.lights)
        for l in range(sc.L):
            s = sc.srays[k][l]
            sd, so, smaxt = _np(s.d), _np(s.o), _np(s.maxt)
            assert np.abs(sd - sc.lights[l, :3, None]).max() == 0
            assert np.all((smaxt == np.inf) | (smaxt == -1.0))
            sure = ~valid | ((np.abs(cw) > MARGIN) & (margin[0, l] > MARGIN))
            assert sure.mean() > 0.999
            st = smaxt == np.inf
            assert np.array_equal(st[sure], want[0, l][sure]), (k, l)
            ref_o = B.spawn_origin(p2, n2, np.broadcast_to(sc.lights[l, :3, None].astype(np.float64), p2.shape))
            assert st.any() and np.abs(so - ref_o)[:, st].max() <= 1e-6, (k, l, np.abs(so - ref_o)[:, st].max())
        # sky ray k
        r = sc.sky_rays[k]
        d, o, maxt = _np(r.d), _np(r.o), _np(r.maxt)
        assert np.abs(d - sc.ws[k]).max() <= 2e-6, (k, np.abs(d - sc.ws[k]).max())
        assert np.all((maxt == np.inf) | (maxt == -1.0))
        sure = (sc.smargin[k] > MARGIN) | ~sc.eligible
        assert sure.mean() > 0.999
        tr = maxt == np.inf
        assert np.array_equal(tr[sure], sc.straced[k][sure]), k
        ref_o = S.spawn_origin(sc.np["p"], sc.np["n"], sc.ws[k])
        assert tr.any() and (~tr).any() and np.abs(o - ref_o)[:, tr].max() <= 1e-6, (k, np.abs(o - ref_o)[:, tr].max())


# ---- (2) the record, three ways --------------------------------------------------------------------------------------
def test_record_three_ways_exactly(hf, scene):
    """the fused kernels' hit_prim / lit_bits / vis_bits == the two-call sequence in both coherence modes == the oracle
    on the materialised rays.  The oracle is the judge: each side is compared with it, so a difference names its side."""
    sc = scene
    hit, lit = B.unpack(sc.prim, sc.lit, 8)
    assert not lit[:, sc.L:].any()                                         # no bit at or above n_lights
    if sc.L == 8:
        assert lit[:, 7].any()                                             # bit 7 is used
    vis = S.unpack(sc.words, 32)
    assert not vis[K:].any()
    n_hit = n_traced = n_seen = n_sky = n_back = 0
    n_lit, n_shadow = np.zeros(sc.L), np.zeros(sc.L)
    for k in range(K):
        # the oracle on the materialised rays
        tr = _np(sc.brays[k].maxt >= 0)
        t, _, _, prim = sc.field.ray_intersect_preliminary(_rows7(sc.brays[k])[:, tr])
        oracle_prim = np.full(sc.n, MISS, np.uint32)
        oracle_prim[np.flatnonzero(tr)[np.isfinite(t)]] = prim[np.isfinite(t)]
        assert np.array_equal(sc.prim[k], oracle_prim), ("fused != oracle", k, int((sc.prim[k] != oracle_prim).sum()))
        n_hit += int(hit[k].sum()); n_traced += int(tr.sum())
        # a hit seen from behind (a spawned origin under the neighbouring facet of a crease that the shear made acute)
        # is recorded and carries no light
        cw = (LS.normals_of(sc, sc.prim[k], hit[k]) * _np(sc.brays[k].d)).sum(0)
        n_back += int((hit[k] & (cw > 0)).sum())
        assert not lit[k][:, hit[k] & (cw > MARGIN)].any()
        oracle_lit = np.zeros((sc.L, sc.n), bool)
        for l in range(sc.L):
            st = _np(sc.srays[k][l].maxt >= 0)
            oracle_lit[l, st] = ~sc.field.ray_test(_rows7(sc.srays[k][l])[:, st]).astype(bool)
            assert np.array_equal(lit[k, l], oracle_lit[l]), ("fused != oracle", k, l, int((lit[k, l] != oracle_lit[l]).sum()))
            n_lit[l] += int(lit[k, l].sum()); n_shadow[l] += int(st.sum())
        str_ = _np(sc.sky_rays[k].maxt >= 0)
        oracle_vis = np.zeros(sc.n, bool)
        oracle_vis[str_] = ~sc.field.ray_test(_rows7(sc.sky_rays[k])[:, str_]).astype(bool)
        assert np.array_equal(vis[k], oracle_vis), ("fused != oracle", k, int((vis[k] != oracle_vis).sum()))
        n_seen += int(vis[k].sum()); n_sky += int(str_.sum())
        # the two-call sequence, in both coherence modes
        for mode in (hf.Heightfield.COHERENCE_AUTO, hf.Heightfield.COHERENCE_INCOHERENT):
            old = sc.shape.ray_coherence()
            sc.shape.set_ray_coherence(mode)
            try:
                pi = sc.shape.ray_intersect_preliminary(sc.brays[k])
                two = np.where(_np(pi.is_valid()), _np(pi.prim_index).view(np.uint32), np.uint32(MISS))
                assert np.array_equal(two, oracle_prim), ("two-call != oracle", mode, k, int((two != oracle_prim).sum()))
                for l in range(sc.L):
                    two = _np((sc.srays[k][l].maxt >= 0) & ~sc.shape.ray_test(sc.srays[k][l]))
                    assert np.array_equal(two, oracle_lit[l]), ("two-call != oracle", mode, k, l, int((two != oracle_lit[l]).sum()))
                two = _np((sc.sky_rays[k].maxt >= 0) & ~sc.shape.ray_test(sc.sky_rays[k]))
                assert np.array_equal(two, oracle_vis), ("two-call != oracle", mode, k, int((two != oracle_vis).sum()))
            finally:
                sc.shape.set_ray_coherence(old)
    print(sc.name, "eligible share", sc.eligible.mean(), "bounce hit share", n_hit / n_traced, "sky unoccluded share", n_seen / n_sky,
          "lit share", n_lit / n_shadow, "lit records", n_lit, "hits seen from behind", n_back)
    assert 0.2 <= n_hit / n_traced <= 0.8 and 0.2 <= n_seen / n_sky <= 0.8
    assert np.all((0.03 <= n_lit / n_shadow) & (n_lit / n_shadow <= 0.97)) and np.all(n_lit >= 40)


# ---- (3) image, adjoint, tangent -------------------------------------------------------------------------------------
SPPS = [4, 3, 64, 128]     # quad stages; one atomic per sample; all cross-lane stages; two waves per pixel + the PIXEL tangent


@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("spp", SPPS)
def test_bounce_image_adjoint_and_tangent_against_the_restatement(hf, scene, spp, with_weight):
    """Values are at most 1 by the sizes of the inputs, not by a run: a sample's value under one light is at most
    weight_max albedo (albedo/pi) E <= 1.5 * 0.7 * 0.7 / pi = 0.23."""
    sc = scene
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    rng = np.random.default_rng(100 * spp + 4)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32) if with_weight else None
    wt = _cu(wgt).requires_grad_(True) if with_weight else None
    img, prim, lit = hf.bounce_lighting(sc.shape, si, ray, sc.lt, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wt,
                                        return_records=True)
    assert img.shape == (sc.L, m // spp) and prim.shape == (K, m) and lit.shape == (K, m)
    assert np.array_equal(_np(prim).view(np.uint32), sc.prim[:, :m]) and np.array_equal(_np(lit), sc.lit[:, :m])
    hit, lt = _records(prim, lit, sc.L)
    nq = _nq(sc, _np(prim), hit)
    arrs = [a[..., :m] for a in sc.arrs]
    w, z = sc.w[:, :, :m], sc.z[:, :m]
    ref, _, absum = B.forward(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp)
    print(sc.name, "spp", spp, "image")
    assert np.all(ref.max(1) > 0) and 0.002 < ref.max() <= 1.0 and _close(_np(img), ref, absum, K)   # (every light's row is lit)
    gi = rng.normal(size=(sc.L, m // spp)).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    adj = B.adjoint(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp, w, z, gi)
    el = sc.eligible[:m]
    got_n = _np(si.sh_frame.n.grad)
    print("grad_sh_n")
    assert np.abs(adj["grad_sh_n"]).max() > 0 and _close(got_n, adj["grad_sh_n"], adj["abs_sh_n"], K)
    assert (~el).any() and not got_n[:, ~el].any()                       # exact zeros
    if with_weight:
        got_w = _np(wt.grad)
        print("grad_weight")
        assert _close(got_w, adj["grad_weight"], adj["abs_weight"], K)
        assert not got_w[~el].any()
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32) if with_weight else None
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), _cu(dn))
        wd = fwAD.make_dual(wt.detach(), _cu(dw)) if with_weight else None
        out = hf.bounce_lighting(sc.shape, si, ray, sc.lt, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wd)
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref, tabs = B.tangent(*arrs, wgt, hit, lt, nq, sc.lights, albedo, spp, w, z, dn, dw)
    print("tangent")
    assert tan.shape == (sc.L, m // spp) and np.abs(tref).max() > 0 and _close(tan, tref, tabs, K)


@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("spp", SPPS)
def test_sky_image_adjoint_and_tangent_against_the_restatement(hf, scene, spp, with_weight):
    """rtol 1e-5, atol 1e-7, the inputs sized so that |value| <= 1 (tests/test_gpu_sky_lighting.py)"""
    sc = scene
    m = sc.n - sc.n % spp
    albedo, wmax = 0.7, 1.5
    L = 1.0 / (4.0 * albedo * wmax)
    rng = np.random.default_rng(100 * spp + 8)
    si, ray = sub(hf, sc, 0, m, requires_grad=True)
    wgt = rng.uniform(0.5, wmax, m).astype(np.float32) if with_weight else None
    wt = _cu(wgt).requires_grad_(True) if with_weight else None
    img, vis = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wt,
                               return_visibility=True)
    assert img.shape == (m // spp,) and vis.shape == (m,)
    assert np.array_equal(_np(vis).view(np.uint32), sc.words[:m])
    bits = S.unpack(_np(vis), K)
    arrs = [a[..., :m] for a in sc.arrs]
    w = sc.ws[:, :, :m]
    ref, _ = S.forward(*arrs, wgt, bits, w, L, albedo, spp)
    got = _np(img)
    print(sc.name, "spp", spp, "image: max", ref.max(), "err", np.abs(got - ref).max())
    assert 0.02 < ref.max() <= 1.0 and np.allclose(got, ref, rtol=1e-5, atol=1e-7), np.abs(got - ref).max()
    gi = rng.normal(size=m // spp).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    gn, gw = S.adjoint(*arrs, wgt, bits, w, L, albedo, spp, gi)
    got_n = _np(si.sh_frame.n.grad)
    print("grad_sh_n: max", np.abs(gn).max(), "err", np.abs(got_n - gn).max())
    assert np.abs(gn).max() > 0 and np.allclose(got_n, gn, rtol=1e-5, atol=1e-7), np.abs(got_n - gn).max()
    el = sc.eligible[:m]
    assert not got_n[:, ~el].any()                                      # exact zeros
    if with_weight:
        got_w = _np(wt.grad)
        print("grad_weight: err", np.abs(got_w - gw).max())
        assert np.allclose(got_w, gw, rtol=1e-5, atol=1e-7), np.abs(got_w - gw).max()
        assert not got_w[~el].any()
    dn = rng.uniform(-0.25, 0.25, (3, m)).astype(np.float32)
    dw = rng.uniform(-0.5, 0.5, m).astype(np.float32) if with_weight else None
    with fwAD.dual_level():
        si.sh_frame.n = fwAD.make_dual(si.sh_frame.n.detach(), _cu(dn))
        wd = fwAD.make_dual(wt.detach(), _cu(dw)) if with_weight else None
        out = hf.sky_lighting(sc.shape, si, ray, radiance=L, albedo=albedo, spp=spp, num_rays=K, seed=SEED, weight=wd)
        tan = _np(fwAD.unpack_dual(out).tangent)
    tref = S.tangent(*arrs, wgt, bits, w, L, albedo, spp, dn, dw)
    print("tangent: max", np.abs(tref).max(), "err", np.abs(tan - tref).max())
    assert np.abs(tref).max() > 0 and np.allclose(tan, tref, rtol=1e-5, atol=1e-7), np.abs(tan - tref).max()


# ---- (4) the heights -------------------------------------------------------------------------------------------------
def _lights_struct(hf, sc):
    L = (hf._capi.hf_dir_light_t * sc.L)()
    for l in range(sc.L):
        L[l].to_light[0], L[l].to_light[1], L[l].to_light[2], L[l].irradiance = sc.lights[l].tolist()
    return L


def _nq_route(sc, prim, hit, grad_nq):
    """sum over the directions of bounce_ref.face_normal_vjp of the recorded triangles under the scene's transform"""
    return sum(B.face_normal_vjp(sc.h64, np.where(hit[k], prim[k], 0), sc.max_height, grad_nq[k], sc.flip, sc.to_world)
               for k in range(len(prim)))


def test_bounce_grad_heights_of_the_c_entry(hf, scene):
    """hf_bounce_lighting_adjoint with grad_heights alone against the restatement; 1e-5 relative L2, the project's bar
    for height gradients (the order of the float atomics is what differs)"""
    sc = scene
    albedo, spp = 0.8, 4
    gi = np.random.default_rng(11).normal(size=(sc.L, sc.n // spp)).astype(np.float32)
    hit, lt = B.unpack(sc.prim, sc.lit, sc.L)
    adj = B.adjoint(*sc.arrs, None, hit, lt, _nq(sc, sc.prim, hit), sc.lights, albedo, spp, sc.w, sc.z, gi)
    want = _nq_route(sc, sc.prim, hit, adj["grad_nq"])
    rows = lambda x: (hf._capi._fp * 3)(*[x.data_ptr() + 4 * (j * x.shape[1]) for j in range(3)])
    sn, dd, tt = (x.detach().contiguous() for x in (sc.si.sh_frame.n, sc.ray.d, sc.si.t))
    gh = sc.shape._zero_heights()
    git = _cu(gi)
    hf._capi.check(hf._capi.lib().hf_bounce_lighting_adjoint(
        sc.shape._h, sc.n, spp, rows(sn), rows(dd), tt.data_ptr(), None, K, SEED, None, sc.L, _lights_struct(hf, sc), albedo,
        sc.prim_t.data_ptr(), sc.lit_t.data_ptr(), sc.n, git.data_ptr(), None, None, gh.data_ptr(),
        torch.cuda.current_stream().cuda_stream))
    got = _np(gh).astype(np.float64)
    assert got.shape == (sc.H, sc.W)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(sc.name, "grad_heights (C entry): relative L2 error", err, "norm", np.linalg.norm(want))
    assert np.linalg.norm(want) > 0 and err <= 1e-5, err


def _chain(hf, oracle, sc, face_normals):
    """(got, sh_n route, n_q route) of image -> backward() -> shape.heightfield.grad of the bounce row"""
    albedo, spp = 0.8, 4
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip,
                           face_normals=face_normals)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, prim, lit = hf.bounce_lighting(shape, si, sc.ray, sc.lt, albedo=albedo, spp=spp, num_rays=K, seed=SEED, return_records=True)
    gi = np.random.default_rng(12).normal(size=tuple(img.shape)).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad).astype(np.float64)
    sh_n, t = _np(si.sh_frame.n), _np(si.t)
    hit, lt = _records(prim, lit, sc.L)
    prim = _np(prim).view(np.uint32)
    w, z = B.directions(sh_n, np.arange(sc.n), K, SEED)
    adj = B.adjoint(sh_n, sc.np["d"], t, None, hit, lt, _nq(sc, prim, hit), sc.lights, albedo, spp, w, z, gi)
    route_nq = _nq_route(sc, prim, hit, adj["grad_nq"])
    gn = adj["grad_sh_n"].astype(np.float32)
    if face_normals:                                                      # the oracle shades flat: its adjoint carries grad_sh_n
        assert np.array_equal(prim, sc.prim)
        t_, u_, v_, prim_ = sc.field.ray_intersect_preliminary(sc.rays)
        route_sh = sc.field.adjoint(sc.rays, t_, u_, v_, prim_, {"sh_n": gn}, oracle.RAY_ALL).astype(np.float64)
    else:                                                                 # the smooth normal's adjoint (tests/test_gpu_smooth_shading.py)
        ybar = torch.zeros((18, sc.n), device="cuda"); ybar[9:12] = _cu(gn)
        pi = shape.ray_intersect_preliminary(sc.ray)
        route_sh = _np(shape.adjoint(sc.ray, pi, ybar, ray_flags=int(hf.RayFlags.All))).astype(np.float64)
    return got, route_sh, route_nq


def test_bounce_chain_to_the_heights(hf, oracle, scene):
    sc = scene
    got, route_sh, route_nq = _chain(hf, oracle, sc, True)
    want = route_sh + route_nq
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(sc.name, "bounce chain: relative L2 error", err, "norms", np.linalg.norm(route_sh), np.linalg.norm(route_nq))
    assert np.linalg.norm(route_sh) > 0 and np.linalg.norm(route_nq) > 0 and err <= 1e-5, err


def test_bounce_chain_to_the_heights_smooth(hf, oracle):
    """face_normals=False on one scene: the sh_n route is the existing composition through shape.adjoint"""
    sc = _scene(hf, oracle, "affine")
    got, route_sh, route_nq = _chain(hf, oracle, sc, False)
    want = route_sh + route_nq
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(sc.name, "bounce chain, face_normals=False: relative L2 error", err, "norms", np.linalg.norm(route_sh), np.linalg.norm(route_nq))
    assert np.linalg.norm(route_sh) > 0 and np.linalg.norm(route_nq) > 0 and err <= 1e-5, err


def test_bounce_height_tangent(hf, scene):
    """hf_bounce_lighting_tangent with dheights alone against the restatement with dn_q = face_normal_jvp, under _close;
    and <tangent(dh), gi> = <dh, adjoint(gi)> to 1e-4 relative (float32 sums), as the identity scene's test"""
    sc = scene
    spp = 4
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip)
    si, ray = sub(hf, sc, 0, sc.n)
    gi = _cu(np.random.default_rng(5).normal(size=(sc.L, sc.n // spp)).astype(np.float32))
    dh = np.random.default_rng(6).normal(size=(sc.H, sc.W)).astype(np.float32)
    shape.heightfield.requires_grad_(True)
    img = hf.bounce_lighting(shape, si, ray, sc.lt, spp=spp, num_rays=K, seed=SEED)
    (img * gi).sum().backward()
    rhs = float((shape.heightfield.grad.double() * _cu(dh).double()).sum())
    with fwAD.dual_level():
        shape.heightfield = fwAD.make_dual(shape.heightfield.detach(), _cu(dh))
        tan = fwAD.unpack_dual(hf.bounce_lighting(shape, si, ray, sc.lt, spp=spp, num_rays=K, seed=SEED)).tangent
    hit, lt = B.unpack(sc.prim, sc.lit, sc.L)
    dnq = np.stack([B.face_normal_jvp(sc.h64, np.where(hit[k], sc.prim[k], 0), sc.max_height, dh, sc.flip, sc.to_world) for k in range(K)])
    tref, tabs = B.tangent(*sc.arrs, None, hit, lt, _nq(sc, sc.prim, hit), sc.lights, 1.0, spp, sc.w, sc.z, dn_q=dnq)
    print(sc.name, "height tangent")
    assert np.abs(tref).max() > 0 and _close(_np(tan), tref, tabs, K)
    lhs = float((tan.double() * gi.double()).sum())
    print("heights: <tangent, gi>", lhs, "<dh, adjoint>", rhs)
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize("name", ["affine", "flip_below"])
def test_sky_chain_to_the_heights(hf, oracle, name):
    """image -> backward() -> shape.heightfield.grad against the restatement's grad_sh_n (fed with the GPU's bits) carried
    to the heights by the oracle's adjoint under the same to_world and flip_normals; 1e-5 relative L2"""
    sc = _scene(hf, oracle, name)
    shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip)
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(sc.ray, hf.RayFlags.All)
    img, vis = hf.sky_lighting(shape, si, sc.ray, radiance=1.3, albedo=0.8, spp=4, num_rays=K, seed=SEED, return_visibility=True)
    gi = np.random.default_rng(11).normal(size=tuple(img.shape)).astype(np.float32)
    (img * _cu(gi)).sum().backward()
    got = _np(shape.heightfield.grad).astype(np.float64)
    assert np.array_equal(_np(vis).view(np.uint32), sc.words)
    t, u, v, prim = sc.field.ray_intersect_preliminary(sc.rays)
    rec = sc.field.compute_surface_interaction(sc.rays, t, u, v, prim, oracle.RAY_ALL)
    gn, _ = S.adjoint(rec["sh_n"], sc.rays[3:6], rec["t"], None, S.unpack(sc.words, K), sc.ws, 1.3, 0.8, 4, gi)
    gh = sc.field.adjoint(sc.rays, t, u, v, prim, {"sh_n": gn.astype(np.float32)}, oracle.RAY_ALL).astype(np.float64)
    err = np.linalg.norm(got - gh) / np.linalg.norm(gh)
    print(sc.name, "sky chain: dL/dheight relative L2 error", err, "norm", np.linalg.norm(gh))
    assert np.linalg.norm(gh) > 0 and err <= 1e-5, err


# ---- (5) global ids --------------------------------------------------------------------------------------------------
def _run_both(hf, sc, lo, hi, ids, gi_b, gi_s, wgt, dn, dw, shape=None):
    """both rows on the samples [lo, hi) with stream ids `ids` (None: the position): records, spp = 4 images, grad_sh_n,
    grad_weight, the dsh_n / dweight tangents; gi_* are the image gradients of these samples' pixels"""
    shape = shape or sc.shape
    out = {}
    for row in ("bounce", "sky"):
        si, ray = sub(hf, sc, lo, hi, requires_grad=True)
        wt = wgt[lo:hi].clone().requires_grad_(True)
        if row == "bounce":
            call = lambda s, w_: hf.bounce_lighting(shape, s, ray, sc.lt, albedo=0.7, spp=4, num_rays=K, seed=SEED, weight=w_,
                                                    ray_index=ids, return_records=True)
            img, prim, lit = call(si, wt)
            out["prim"], out["lit"] = prim.clone(), lit.clone()
            (img * gi_b[:, lo // 4:hi // 4]).sum().backward()
        else:
            call = lambda s, w_: hf.sky_lighting(shape, s, ray, radiance=0.3, albedo=0.7, spp=4, num_rays=K, seed=SEED, weight=w_,
                                                 ray_index=ids, return_visibility=True)
            img, vis = call(si, wt)
            out["vis"] = vis.clone()
            (img * gi_s[lo // 4:hi // 4]).sum().backward()
        out[row + "_image"] = img.detach().clone()
        out[row + "_grad_sh_n"], out[row + "_grad_weight"] = si.sh_frame.n.grad.clone(), wt.grad.clone()
        with fwAD.dual_level():
            si2, _ = sub(hf, sc, lo, hi)
            si2.sh_frame.n = fwAD.make_dual(si2.sh_frame.n, dn[:, lo:hi].contiguous())
            wd = fwAD.make_dual(wgt[lo:hi].clone(), dw[lo:hi].contiguous())
            out[row + "_tangent"] = fwAD.unpack_dual(call(si2, wd)[0]).tangent.clone()
    return out


def _inputs(sc, seed):
    rng = np.random.default_rng(seed)
    return (_cu(rng.normal(size=(sc.L, sc.n // 4)).astype(np.float32)), _cu(rng.normal(size=sc.n // 4).astype(np.float32)),
            _cu(rng.uniform(0.5, 1.5, sc.n).astype(np.float32)), _cu(rng.uniform(-0.25, 0.25, (3, sc.n)).astype(np.float32)),
            _cu(rng.uniform(-0.5, 0.5, sc.n).astype(np.float32)))


def test_a_wavefront_cut_in_two_is_the_whole_bit_for_bit(hf, scene):
    """the samples [0, 1148) and [1148, 2300) as two calls with ray_index = their global ids (how chunked and tiled
    rendering calls these rows): no atomics are involved at spp = 4 and the film butterfly stays within a pixel, so
    everything but grad_heights is the whole wavefront's bit for bit; grad_heights (float atomics) to 1e-5 relative L2"""
    sc = scene
    inp = _inputs(sc, 21)
    whole = _run_both(hf, sc, 0, sc.n, None, *inp)
    assert np.array_equal(_np(whole["prim"]).view(np.uint32), sc.prim) and np.array_equal(_np(whole["vis"]).view(np.uint32), sc.words)
    ids = torch.arange(sc.n, dtype=torch.int32, device="cuda")
    parts = [_run_both(hf, sc, lo, hi, ids[lo:hi].contiguous(), *inp) for lo, hi in ((0, SPLIT), (SPLIT, sc.n))]
    for key, want in whole.items():
        got = torch.cat([p[key] for p in parts], dim=-1)
        assert got.shape == want.shape and torch.equal(got, want), (key, int((got != want).sum()))
    # the second part WITHOUT its ids is another result: the ids are what makes the parts the whole
    other = _run_both(hf, sc, SPLIT, sc.n, None, *inp)
    for key in ("prim", "vis", "bounce_image", "sky_image", "bounce_grad_sh_n", "sky_grad_sh_n", "bounce_tangent", "sky_tangent"):
        assert not torch.equal(other[key], parts[1][key]), key
    # grad_heights: the sum over the parts
    gi = inp[0]
    grads = []
    for chunks in (((0, sc.n, None),), ((0, SPLIT, ids[:SPLIT].contiguous()), (SPLIT, sc.n, ids[SPLIT:].contiguous()))):
        shape = hf.Heightfield(heightfield=sc.ht.clone(), max_height=sc.max_height, to_world=sc.tw64, flip_normals=sc.flip)
        shape.heightfield.requires_grad_(True)
        for lo, hi, rid in chunks:
            si, ray = sub(hf, sc, lo, hi)
            img = hf.bounce_lighting(shape, si, ray, sc.lt, spp=4, num_rays=K, seed=SEED, ray_index=rid)
            (img * gi[:, lo // 4:hi // 4]).sum().backward()
        grads.append(_np(shape.heightfield.grad).astype(np.float64))
    err = np.linalg.norm(grads[1] - grads[0]) / np.linalg.norm(grads[0])
    print(sc.name, "grad_heights, two chunks against the whole: relative L2 error", err)
    assert np.linalg.norm(grads[0]) > 0 and err <= 1e-5, err


def test_permuted_ids_are_followed_by_every_kernel(hf, scene):
    """with a permuted ray_index the forward, adjoint and tangent of both rows are the restatement's drawn with those
    ids (fed with that call's record), and not the position-indexed result"""
    sc = scene
    gi_b, gi_s, wgt, dn, dw = inp = _inputs(sc, 22)
    perm = torch.randperm(sc.n, generator=torch.Generator().manual_seed(4)).to(dtype=torch.int32)
    ids = perm.numpy()
    got = _run_both(hf, sc, 0, sc.n, perm.cuda(), *inp)
    pos = _run_both(hf, sc, 0, sc.n, None, *inp)
    npw, npdn, npdw = _np(wgt), _np(dn), _np(dw)
    # bounce
    w, z = B.directions(sc.np["sh_n"], ids, K, SEED)
    hit, lt = _records(got["prim"], got["lit"], sc.L)
    prim = _np(got["prim"]).view(np.uint32)
    for k in range(K):                                                     # the record is that of the rays drawn with the ids
        r = hf.bounce_rays(sc.shape, sc.si, sc.ray, k, seed=SEED, ray_index=perm.cuda())
        assert np.abs(_np(r.d) - w[k]).max() <= 2e-6
        tr = _np(r.maxt >= 0)
        t, _, _, op = sc.field.ray_intersect_preliminary(_rows7(r)[:, tr])
        want = np.full(sc.n, MISS, np.uint32); want[np.flatnonzero(tr)[np.isfinite(t)]] = op[np.isfinite(t)]
        assert np.array_equal(prim[k], want), k
    nq = _nq(sc, prim, hit)
    ref, _, absum = B.forward(*sc.arrs, npw, hit, lt, nq, sc.lights, 0.7, 4)
    adj = B.adjoint(*sc.arrs, npw, hit, lt, nq, sc.lights, 0.7, 4, w, z, _np(gi_b))
    tref, tabs = B.tangent(*sc.arrs, npw, hit, lt, nq, sc.lights, 0.7, 4, w, z, npdn, npdw)
    print(sc.name, "permuted ids, bounce: image, grad_sh_n, grad_weight, tangent")
    assert _close(_np(got["bounce_image"]), ref, absum, K)
    assert _close(_np(got["bounce_grad_sh_n"]), adj["grad_sh_n"], adj["abs_sh_n"], K)
    assert _close(_np(got["bounce_grad_weight"]), adj["grad_weight"], adj["abs_weight"], K)
    assert _close(_np(got["bounce_tangent"]), tref, tabs, K)
    # sky
    ws = S.directions(ids, K, SEED)
    bits = S.unpack(_np(got["vis"]), K)
    for k in range(K):
        r = hf.sky_rays(sc.si, sc.ray, k, seed=SEED, ray_index=perm.cuda())
        assert np.abs(_np(r.d) - ws[k]).max() <= 2e-6
        tr = _np(r.maxt >= 0)
        want = np.zeros(sc.n, bool); want[tr] = ~sc.field.ray_test(_rows7(r)[:, tr]).astype(bool)
        assert np.array_equal(bits[k], want), k
    ref, _ = S.forward(*sc.arrs, npw, bits, ws, 0.3, 0.7, 4)
    gn, gw = S.adjoint(*sc.arrs, npw, bits, ws, 0.3, 0.7, 4, _np(gi_s))
    tref = S.tangent(*sc.arrs, npw, bits, ws, 0.3, 0.7, 4, npdn, npdw)
    for name, g, r_ in (("sky_image", got["sky_image"], ref), ("sky_grad_sh_n", got["sky_grad_sh_n"], gn),
                        ("sky_grad_weight", got["sky_grad_weight"], gw), ("sky_tangent", got["sky_tangent"], tref)):
        print("permuted ids,", name, "err", np.abs(_np(g) - r_).max())
        assert np.abs(r_).max() > 0 and np.allclose(_np(g), r_, rtol=1e-5, atol=1e-7), (name, np.abs(_np(g) - r_).max())
    # ... and not the position-indexed result
    for key in got:
        a, b = _np(got[key]).astype(np.float64), _np(pos[key]).astype(np.float64)
        if key in ("prim", "lit", "vis"):
            assert (a != b).mean() > 0.02, key
        else:
            assert np.linalg.norm(a - b) > 0.02 * np.linalg.norm(b), (key, np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- (6) repeatability -------------------------------------------------------------------------------------------------
def test_repeatable(hf, oracle):
    """everything but grad_heights (float atomics), twice"""
    sc = _scene(hf, oracle, "affine")
    inp = _inputs(sc, 23)
    a, b = (_run_both(hf, sc, 0, sc.n, None, *inp) for _ in range(2))
    for key in a:
        assert torch.equal(a[key], b[key]), key

"""The grid-stride kernels beyond their first loop iteration.

Every kernel but the traversal walks its input in a grid-stride loop whose grid comes from grid_for(n, cap)
(csrc/hf_kernels.hip): a wave takes a second trip round its loop only when n exceeds cap x 256 items -- 4.19 M rays
for the adjoints, 1.31 M for the launches that sum dL/d(to_world), 67.1 M for the streaming kernels -- and no test
compares a launch of that size with a reference.  What such a launch carries from one iteration to the next -- the
per-wave LDS scatter tile, clean only because tile_flush clears what it flushed; the row band and the twelve
dL/d(to_world) accumulators of a lane; the wave-uniform exit and the clamp of the ragged tail, which first matter in a
later iteration; uniform Adam's running maximum -- is therefore out of every other test's sight.

The TEST HOOK HF_FORCE_GRID=<blocks> (include/hf.h) lowers the grid, so that launches of test size loop: with C blocks
forced and n = 256 C 3 + 256 + 37 items every wave does three or four iterations, the last one is ragged, and some
waves of a block leave the loop one iteration before the others.  Every test asserts through hf_grid_blocks that the
forced launch has C < n / 768 blocks and that the same launch without the hook has ceil(n / 256), so a mistyped
variable name cannot turn it into a no-op.  Every forced launch is compared with the reference its family already
uses, at the tolerance of that family's GPU test (named at each assertion); outputs that are per-lane and free of
atomics must, in addition, be bitwise those of the launch without the hook.

Inputs: incoherent rays (random_rays + inside_rays, shuffled) on a 129 x 65 field under common.affine, so that
consecutive iterations anchor their tile in different places and part of a wave's contributions falls outside the
tile (asserted from the hit triangles); a mask; rays 256 C .. 256 C + 63 miss, so that wave 0 of block 0 has an
iteration without a hit between iterations with hits; one coherent ortho_rays case.  The reparameterisation draws its
rays as its own tests do (from above, onto targets all over the field), area sampling and eval_parameterization random
samples and queries, Adam the 37 x 53 texels of tests/test_adam.py: see there.
"""
import contextlib
import functools
import os
import types

import numpy as np
import pytest
import torch

import attr_ref as AR
import common
import param_ref as PR
import reparam_backward_ref as RB
import reparam_tangent_ref as RT
import smooth_ref as R
import xform_ref as X

pytestmark = pytest.mark.gpu

W, H = 129, 65
S = 0.2            # max_height of the surface-interaction wavefront; see _wavefront
S_REPARAM = 0.4    # ... and of the reparameterisation's
RAY_ALL, RAY_BOUNDARYTEST, RAY_FOLLOWSHAPE = 0xE, 0x40, 0x80
FAMILIES = (0, 1, 2)          # hf_grid_blocks: the flat cap, the streaming cap, the cap of the to_world launches
ADJ_TILE, RB_TILE, ATTR_TILE = 32, 64, 32   # HF_ADJ_TILE, HF_RB_TILE, HF_ATTR_TILE of csrc/hf_kernels.hip


def _n(C):
    return 256 * C * 3 + 256 + 37


@contextlib.contextmanager
def _grid(blocks):
    """HF_FORCE_GRID = blocks (None: unset) for the launches inside; restored afterwards, as tests/test_gpu_parity.py
    does for HF_FORCE_GRAB"""
    old = os.environ.get("HF_FORCE_GRID")
    try:
        if blocks is None:
            os.environ.pop("HF_FORCE_GRID", None)
        else:
            os.environ["HF_FORCE_GRID"] = str(blocks)
        yield
    finally:
        if old is None:
            os.environ.pop("HF_FORCE_GRID", None)
        else:
            os.environ["HF_FORCE_GRID"] = old


def _both(n, C, run, loops=3):
    """(run() as the library sizes its grids, run() with C blocks forced), with the guards on both grids.  loops: the
    iterations every wave of the forced launch does at least"""
    from hf_amd import _capi
    lib = _capi.lib()
    with _grid(None):
        for fam in FAMILIES:
            assert lib.hf_grid_blocks(n, fam) == -(-n // 256), "the launch without the hook: one block per 256 items"
        plain = run()
        torch.cuda.synchronize()
    with _grid(C):
        for fam in FAMILIES:
            blocks = lib.hf_grid_blocks(n, fam)
            assert blocks == C and blocks < n / (256 * loops), (blocks, n)
        forced = run()
        torch.cuda.synchronize()
    return plain, forced


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ai = a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
    bi = b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b
    assert torch.equal(ai, bi), f"{what}: the forced launch differs from the unforced one in a per-lane output"


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu().reshape(-1)
    b = torch.as_tensor(b).double().cpu().reshape(-1)
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def _chunk_spans(vi, vj, live):
    """per 64-item chunk (what one wave takes in one iteration): the extent in texels of the live lanes' vertex rows
    and columns (0 for a chunk without a live lane); vi, vj [3, n]"""
    n = live.shape[0]
    rows, cols = [], []
    for c0 in range(0, n, 64):
        m = live[c0:c0 + 64]
        if not m.any():
            rows.append(0); cols.append(0)
            continue
        a, b = vi[:, c0:c0 + 64][:, m], vj[:, c0:c0 + 64][:, m]
        rows.append(int(a.max() - a.min()) + 1); cols.append(int(b.max() - b.min()) + 1)
    return np.array(rows), np.array(cols)


def _assert_wave_shape(C, hit, vi, vj, live, tile):
    """what the launch shape is for: a hit fraction strictly between 0.2 and 0.9; the wave that takes chunk 4 C (wave 0
    of block 0, second iteration) has no hit there and hits in its first and third iteration; some wave's contributions
    span more than the tile"""
    assert 0.2 < live.mean() < 0.9, live.mean()
    assert not hit[256 * C:256 * C + 64].any() and live[0:64].any() and live[512 * C:512 * C + 64].any()
    rows, cols = _chunk_spans(vi, vj, live)
    assert max(rows.max(), cols.max()) > tile, (rows.max(), cols.max(), tile)


def _miss_block(n_rays=64):
    """object-space rays beside the field that point away from it"""
    o = np.stack([np.full(n_rays, 3.0), np.linspace(-0.5, 0.5, n_rays), np.full(n_rays, 0.3)])
    d = np.repeat(np.array([[1.0], [0.0], [0.1]]) / np.sqrt(1.01), n_rays, 1)
    return np.concatenate([o, d, np.full((1, n_rays), np.inf)])


def _ray(hf, r):
    rt = torch.from_numpy(r).cuda()
    return hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())


# ---- the wavefront of the surface-interaction families: computed once, shared, never changed ------------------------

@functools.lru_cache(maxsize=None)
def _wavefront(oracle, C, kind):
    """max_height 0.2 under common.affine(1): at 65 rows the sine field's seven-cycle term is coarse (nine rows a period),
    and where neighbouring vertex normals differ most the float32 rounding of the smooth kernels' sh_n grows with
    max_height and with the transform's translation.  Measured on these rays: 5.9e-6 here, 1.3e-5 with max_height 0.4
    under common.affine(2) -- over the family's 1e-5 bound with and without the hook, which give the same bytes."""
    import hf_amd
    rng = np.random.default_rng(100 + C)
    n = _n(C)
    h = common.heights("sine", W, H, rng)
    tw = common.affine(1)
    if kind == "incoherent":
        k = (3 * n) // 5
        r = np.concatenate([common.random_rays(k, rng, S), common.inside_rays(n - k, rng, S)], 1)[:, rng.permutation(n)]
    else:   # neighbouring pixels of the orthographic camera, four samples each: a wave stays within a few cells
        r = hf_amd.workload.ortho_rays(128, 128, 4, "cpu", start=60 * 128 * 4, count=n).numpy().astype(np.float64)
    r[:, 256 * C:256 * C + 64] = _miss_block()
    r = common.to_world_rays(r, tw)
    active = rng.uniform(size=n) < 0.85
    f = oracle.OracleField(h, max_height=S, to_world=tw)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    hit = np.isfinite(t)
    live = hit & active
    vi, vj = RT.tri_vertices(W, np.where(hit, prim, 0))
    if kind == "incoherent":
        _assert_wave_shape(C, hit, vi, vj, live, ADJ_TILE)
    else:
        assert 0.2 < live.mean() < 0.9, live.mean()
        rows, cols = _chunk_spans(vi, vj, live)
        assert 0 < max(rows.max(), cols.max()) <= ADJ_TILE   # coherent: every wave's scatter stays inside its tile
    # hits away from grazing incidence and from the sign switch of coordinate_system carry the upstream gradients that
    # are compared with float64 (as tests/test_gpu_ray_flags.py: _steady)
    idx = np.nonzero(live)[0]
    o64, d64 = torch.from_numpy(r[0:3, idx].T.astype(np.float64)), torch.from_numpy(r[3:6, idx].T.astype(np.float64))
    b = (torch.from_numpy(u[idx].astype(np.float64)), torch.from_numpy(v[idx].astype(np.float64)))
    p64 = torch.from_numpy(prim[idx].astype(np.int64))
    ref = R.surface(torch.from_numpy(h.astype(np.float64)), S, torch.from_numpy(tw.astype(np.float64)), False, o64, d64,
                    p64, b, "default", RAY_ALL, False)
    cos = (ref["n"] * d64).sum(-1).abs() / d64.norm(dim=-1)
    steady = ((cos > 5e-2) & (ref["n"][:, 2].abs() > 1e-2)).numpy()
    assert steady.mean() > 0.7
    g = rng.normal(size=(18, n)).astype(np.float32)          # upstream gradients on every lane, misses included
    gs = np.zeros_like(g)
    gs[:, idx[steady]] = g[:, idx[steady]]                    # ... and on the steady live hits alone
    return types.SimpleNamespace(
        C=C, n=n, h=h, tw=tw, r=r, active=active, f=f, t=t, u=u, v=v, prim=prim, hit=hit, live=live, vi=vi, vj=vj, idx=idx,
        o64=o64, d64=d64, b=b, p64=p64, steady=steady, g=g, gs=gs,
        dh=rng.normal(size=(H, W)).astype(np.float32), do=rng.normal(size=(3, n)).astype(np.float32),
        dd=rng.normal(size=(3, n)).astype(np.float32), dM=rng.normal(size=12).astype(np.float32))


def _device_scene(hf, wf, smooth, diff_tw=False):
    shape = hf.Heightfield(heightfield=torch.from_numpy(wf.h).cuda(), max_height=S, to_world=np.asarray(wf.tw, np.float64),
                           face_normals=not smooth, differentiable_to_world=diff_tw)
    ray = _ray(hf, wf.r)
    pi = shape.ray_intersect_preliminary(ray)      # (the traversal: not a grid_for launch)
    assert np.array_equal(wf.prim, pi.prim_index.cpu().numpy().view(np.uint32))
    assert np.array_equal(wf.hit, np.isfinite(pi.t.cpu().numpy()))
    return shape, ray, pi, torch.from_numpy(wf.active).cuda()


def _block_fn(wf, smooth, flags=RAY_ALL):
    """the 18-row block of the live hits as a float64 function of (heights, o, d, to_world)"""
    def fn(hh, o, d, tw):
        return X.si_block(hh, S, tw, False, o, d, wf.p64, wf.b, "default", smooth, flags=flags)
    return fn


def _float64_grads(wf, smooth, g):
    """autograd of the restatement for the upstream rows g [18, n]: dL/dheights [H, W], dL/do, dL/dd [3, live]"""
    hh = torch.from_numpy(wf.h.astype(np.float64)).requires_grad_(True)
    oo, dd = wf.o64.clone().requires_grad_(True), wf.d64.clone().requires_grad_(True)
    tw = torch.from_numpy(wf.tw.astype(np.float64))
    (_block_fn(wf, smooth)(hh, oo, dd, tw) * torch.from_numpy(g[:, wf.idx].astype(np.float64))).sum().backward()
    return hh.grad, oo.grad.T, dd.grad.T


def _expected_band(wf, smooth, live=None):
    live = wf.live if live is None else live
    lo, hi = int(wf.vi[:, live].min()), int(wf.vi[:, live].max()) + 1
    return [max(lo - 1, 0), min(hi + 1, H)] if smooth else [lo, hi]   # the vertex normals reach one row further


def _inner_mask(wf):
    """the live hits whose cell row lies in [12, 41): a band that is not the whole texture"""
    cy = (wf.prim.astype(np.int64) >> 1) // (W - 1)
    return wf.live & (cy >= 12) & (cy < 41)


def _check_heights_and_rays(wf, smooth, g, gh, go, gd, what):
    """flat with every lane's upstream gradient: the oracle, at the bars of tests/test_gpu_parity.py; otherwise float64
    autograd of the restatement, at those of tests/test_gpu_ray_flags.py and tests/test_gpu_smooth_shading.py"""
    gh = gh.cpu().numpy()
    if not smooth and g is wf.g:
        from oracle import hf_oracle as O
        gd_in = {nm: g[a:a + c] for (nm, c), a in zip(O.GRAD_FIELDS, np.cumsum([0] + [c for _, c in O.GRAD_FIELDS])[:-1])}
        gh_o, go_o, gd_o = wf.f.adjoint(wf.r, wf.t, wf.u, wf.v, wf.prim, gd_in, RAY_ALL, active=wf.active, ray_grads=True)
        scale = np.abs(gh_o).max()
        assert scale > 0
        err, l2 = np.abs(gh_o - gh).max(), np.linalg.norm(gh_o - gh) / np.linalg.norm(gh_o)
        print(f"{what}: heights vs the oracle max {err / scale:.3g} of the scale, L2 {l2:.3g}")
        assert err <= 2e-5 * scale + 1e-12, (what, err / scale)
        assert l2 <= 1e-5, (what, l2)
        if go is not None:
            assert np.allclose(go_o, go.cpu().numpy(), rtol=1e-4, atol=1e-4 * np.abs(go_o).max()), what
            assert np.allclose(gd_o, gd.cpu().numpy(), rtol=1e-4, atol=1e-4 * np.abs(gd_o).max()), what
        return
    gref, oref, dref = _float64_grads(wf, smooth, g)
    scale = float(gref.abs().max())
    assert scale > 0
    err = float((torch.from_numpy(gh).double() - gref).abs().max())
    print(f"{what}: heights vs float64 autograd max {err / scale:.3g} of the scale")
    assert torch.allclose(torch.from_numpy(gh).double(), gref, rtol=2e-4, atol=2e-4 * scale), (what, err / scale)
    if go is not None:
        live = torch.from_numpy(wf.live)
        for got, want in ((go, oref), (gd, dref)):
            sc = float(want.abs().max()) + 1e-30
            assert torch.allclose(got.cpu().double()[:, live], want, rtol=2e-4, atol=2e-4 * sc), what
            assert bool((got.cpu()[:, ~live] == 0).all()), what


# ---- hf_adjoint, hf_adjoint_rows -------------------------------------------------------------------------------------

@pytest.mark.parametrize("raygrad", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("C,kind", [(1, "incoherent"), (3, "incoherent"), (3, "coherent")])
def test_adjoint_and_adjoint_rows(hf, oracle, C, kind, smooth, raygrad):
    wf = _wavefront(oracle, C, kind)
    shape, ray, pi, act = _device_scene(hf, wf, smooth)
    g_np = wf.gs if smooth else wf.g
    g = torch.from_numpy(g_np).cuda()
    act_inner = torch.from_numpy(_inner_mask(wf)).cuda()

    def run():
        band = shape.new_row_band()
        rows = shape.adjoint(ray, pi, g, ray_flags=RAY_ALL, active=act, ray_grads=raygrad, row_band=band)   # hf_adjoint_rows
        plain = shape.adjoint(ray, pi, g, ray_flags=RAY_ALL, active=act, ray_grads=raygrad)                 # hf_adjoint
        inner = shape.new_row_band()
        shape.adjoint(ray, pi, g, ray_flags=RAY_ALL, active=act_inner, row_band=inner)
        return (rows if raygrad else (rows, None, None)), (plain if raygrad else (plain, None, None)), band, inner

    plain, ((gh, go, gd), (gh1, go1, gd1), band, inner) = _both(wf.n, C, run)
    for label, a, b, c in (("hf_adjoint_rows", gh, go, gd), ("hf_adjoint", gh1, go1, gd1)):
        _check_heights_and_rays(wf, smooth, g_np, a, b, c, f"{label} C={C} {kind} smooth={smooth}")
    # the band: exactly the rows the live hits' triangles touch, with and without the hook
    assert band.cpu().tolist() == _expected_band(wf, smooth) == plain[2].cpu().tolist()
    want = _expected_band(wf, smooth, _inner_mask(wf))
    assert inner.cpu().tolist() == want == plain[3].cpu().tolist() and 0 < want[0] < want[1] < H
    lo, hi = band.cpu().tolist()
    assert float(gh[:lo].abs().sum()) == 0 and float(gh[hi:].abs().sum()) == 0
    if raygrad:
        for k, label in ((0, "hf_adjoint_rows"), (1, "hf_adjoint")):
            _same_bytes((go, go1)[k], plain[k][1], f"grad_o of {label}")
            _same_bytes((gd, gd1)[k], plain[k][2], f"grad_d of {label}")


# ---- hf_adjoint_transform, hf_tangent_transform ------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_adjoint_transform_and_tangent_transform(hf, oracle, C, smooth):
    wf = _wavefront(oracle, C, "incoherent")
    shape, ray, pi, act = _device_scene(hf, wf, smooth, diff_tw=True)
    g = torch.from_numpy(wf.gs).cuda()
    dh, do, dd, dM = (torch.from_numpy(x).cuda() for x in (wf.dh, wf.do, wf.dd, wf.dM))

    def run():
        gtw, band = torch.zeros(12, device="cuda"), shape.new_row_band()
        gh, go, gd = shape.adjoint(ray, pi, g, ray_flags=RAY_ALL, active=act, ray_grads=True, row_band=band, grad_to_world=gtw)
        tan = shape.tangent(ray, pi, dh, do, dd, ray_flags=RAY_ALL, active=act, d_to_world=dM)
        return gh, go, gd, band, gtw, tan

    plain, (gh, go, gd, band, gtw, tan) = _both(wf.n, C, run)
    what = f"hf_adjoint_transform C={C} smooth={smooth}"
    _check_heights_and_rays(wf, smooth, wf.gs, gh, go, gd, what)
    assert band.cpu().tolist() == _expected_band(wf, smooth) == plain[3].cpu().tolist()
    _same_bytes(go, plain[1], "grad_o"); _same_bytes(gd, plain[2], "grad_d"); _same_bytes(tan, plain[5], "hf_tangent_transform")
    # dL/d(to_world): float64 central differences of the restatement, 2e-3 of the gradient's norm
    # (tests/test_gpu_transform_grad.py::test_adjoint_matches_float64_fd)
    fn = _block_fn(wf, smooth)
    h64, gl = torch.from_numpy(wf.h.astype(np.float64)), torch.from_numpy(wf.gs[:, wf.idx].astype(np.float64))
    fd = X.fd_to_world(lambda t: (fn(h64, wf.o64, wf.d64, t) * gl).sum(), wf.tw)
    got = gtw.cpu().double().numpy().reshape(3, 4)
    err = np.linalg.norm(got - fd) / np.linalg.norm(fd)
    print(f"{what}: grad_to_world vs float64 central differences {err:.3g}; vs the unforced launch {_rel(gtw, plain[4]):.3g}")
    assert err < 2e-3, (err, got, fd)
    # hf_tangent_transform is the transpose of hf_adjoint_transform: 1e-4 of the terms' scale (test_gpu_transform_grad._transpose,
    # test_gpu_tangent._transpose_check)
    per_ray = (g.double() * tan.double()).sum(0)
    lhs, scale = float(per_ray.sum()), float(per_ray.abs().sum())
    rhs = float((gh.double() * dh.double()).sum() + (go.double() * do.double()).sum() + (gd.double() * dd.double()).sum()
                + (gtw.double() * dM.double()).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    assert bool((tan[:, ~torch.from_numpy(wf.live).cuda()] == 0).all())


# ---- hf_compute_surface_interaction, hf_tangent, hf_shading_derivatives ----------------------------------------------

def _record(si):
    return {"t": si.t, "p": si.p, "n": si.n, "uv": si.uv, "sh_n": si.sh_frame.n, "dp_du": si.dp_du, "dp_dv": si.dp_dv,
            "boundary_test": si.boundary_test, "sh_s": si.sh_frame.s, "sh_t": si.sh_frame.t, "wi": si.wi}


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_surface_interaction_tangent_and_shading_derivatives(hf, oracle, C, smooth):
    wf = _wavefront(oracle, C, "incoherent")
    shape, ray, pi, act = _device_scene(hf, wf, smooth)
    flags = RAY_ALL | RAY_BOUNDARYTEST
    dh, do, dd = (torch.from_numpy(x).cuda() for x in (wf.dh, wf.do, wf.dd))

    def run():
        rec = _record(shape.compute_surface_interaction(ray, pi, flags, active=act))
        tan = shape.tangent(ray, pi, dh, do, dd, ray_flags=RAY_ALL, active=act)
        du, dv = shape.shading_derivatives(pi, act)
        return {k: v.detach().clone() for k, v in rec.items()}, tan, du, dv

    (rec0, tan0, du0, dv0), (rec, tan, du, dv) = _both(wf.n, C, run)
    for k in rec:
        _same_bytes(rec[k], rec0[k], f"si.{k}")
    _same_bytes(tan, tan0, "hf_tangent"); _same_bytes(du, du0, "dn_du"); _same_bytes(dv, dv0, "dn_dv")
    # the record: the oracle, rtol 1e-5 / atol 2e-6 (tests/test_gpu_parity.py::test_surface_interaction_and_adjoint); with
    # smooth shading sh_n against the restatement, 1e-5 (tests/test_gpu_smooth_shading.py::_check_forward), the frame
    # built on it by the bitwise comparison above
    si_o = wf.f.compute_surface_interaction(wf.r, wf.t, wf.u, wf.v, wf.prim, flags, active=wf.active)
    names = ("t", "p", "n", "uv", "dp_du", "dp_dv", "boundary_test") + (() if smooth else ("sh_n", "sh_s", "sh_t", "wi"))
    for k in names:
        a, b = si_o[k], rec[k].cpu().numpy()
        assert np.allclose(a, b, rtol=1e-5, atol=2e-6), (k, np.abs(a - b)[np.isfinite(a)].max())
    live = torch.from_numpy(wf.live)
    h64, tw64 = torch.from_numpy(wf.h.astype(np.float64)), torch.from_numpy(wf.tw.astype(np.float64))
    ref = R.surface(h64, S, tw64, False, wf.o64, wf.d64, wf.p64, wf.b, "default", RAY_ALL, smooth)
    if smooth:
        assert float((rec["sh_n"].cpu()[:, live].T.double() - ref["sh_n"]).abs().max()) <= 1e-5
        assert bool((rec["sh_n"].cpu()[:, ~live] == 0).all())
        assert float((rec["sh_n"] - rec["n"]).abs().max()) > 1e-3
    # the tangent: the JVP of the restatement, per ray (tests/test_gpu_ray_flags.py, tests/test_gpu_tangent.py)
    fn = _block_fn(wf, smooth)
    _, jv = torch.func.jvp(lambda hh, o, d: fn(hh, o, d, tw64), (h64, wf.o64, wf.d64),
                           (torch.from_numpy(wf.dh.astype(np.float64)), torch.from_numpy(wf.do[:, wf.idx].T.astype(np.float64)).contiguous(),
                            torch.from_numpy(wf.dd[:, wf.idx].T.astype(np.float64)).contiguous()))
    keep = torch.from_numpy(wf.steady)
    got, want = tan.cpu()[:, live].double()[:, keep], jv[:, keep]
    tol = 2e-4 * want.abs() + 2e-4 * (1 + want.abs().amax(0, keepdim=True))
    assert bool(((got - want).abs() <= tol).all()), float(((got - want).abs() / tol).max())
    assert bool((tan.cpu()[:, ~live] == 0).all())
    # dn_du, dn_dv: 1e-5 (tests/test_gpu_smooth_shading.py::test_shading_derivatives); zero with flat shading and off the hits
    assert float(du.cpu()[:, ~live].abs().max()) == 0 and float(dv.cpu()[:, ~live].abs().max()) == 0
    if smooth:
        rdu, rdv = R.shading_derivatives(ref["N"], wf.b[0], wf.b[1])
        assert float((du.cpu()[:, live].T.double() - rdu).abs().max()) < 1e-5
        assert float((dv.cpu()[:, live].T.double() - rdv).abs().max()) < 1e-5
        assert float(du.abs().max()) > 1e-3
    else:
        assert float(du.abs().max()) == 0 and float(dv.abs().max()) == 0


# ---- hf_reparam_backward, hf_reparam_tangent, hf_reparam_backward_full -------------------------------------------------

REPARAM = dict(num_rays=4, kappa=1e5, exponent=3.0, antithetic=True, seed=9)
HEIGHTS_ATOMICS = 2e-6      # the same sums in another atomics order (tests/test_reparam.py, tests/test_gpu_reparam_backward_full.py)


@functools.lru_cache(maxsize=None)
def _reparam_case(oracle, C, xform):
    rng = np.random.default_rng(200 + C)
    n, K = _n(C), REPARAM["num_rays"]
    h = common.heights("sine", W, H, rng)
    M = common.affine(2).astype(np.float64) if xform else np.eye(4)[:3]
    # Rays from above onto targets all over the field and a little beside it, as the family's own tests draw them
    # (test_gpu_reparam_tangent._rays_np): incoherent, so the tile moves from one iteration to the next.  random_rays +
    # inside_rays graze silhouettes, where one sample's weight (1 / (D - 1 + B))^3 D carries most of the gradient's norm
    # and float32 parts from the float64 oracle in the fourth digit (prb_reparam): measured on such rays, 3.5e-4
    # on the heights against the 3e-5 bound, the same with and without the hook.
    tgt = np.stack([rng.uniform(-1.1, 1.1, n), rng.uniform(-1.1, 1.1, n), np.full(n, 0.25)])
    org = tgt + np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(1.0, 2.0, n)])
    r = np.concatenate([org, tgt - org, np.full((1, n), np.inf)])
    r[:, 256 * C:256 * C + 64] = _miss_block()
    r = common.to_world_rays(r, M if xform else None).astype(np.float64)
    o, d = r[0:3].astype(np.float32), (r[3:6] / np.linalg.norm(r[3:6], axis=0)).astype(np.float32)   # unit directions
    active = (rng.uniform(size=n) > 0.1).astype(np.uint8)
    ids = rng.permutation(1 << 20)[:n].astype(np.uint32)
    f = oracle.OracleField(h, max_height=S_REPARAM, to_world=M)
    with oracle.with_ray_ids(ids):
        Sm, act = RT.samples(oracle, f, o, d, K, REPARAM["kappa"], REPARAM["exponent"], REPARAM["antithetic"], REPARAM["seed"], active)
    hit = np.stack([s[1] for s in Sm])                                     # [K, n], inactive rays excluded
    share = hit[:, act].mean()
    assert 0.2 < share < 0.9, share                                        # auxiliary hits and active misses
    m = slice(256 * C, 256 * C + 64)
    assert not hit[:, m].any() and hit[:, 0:64].any() and hit[:, 512 * C:512 * C + 64].any()
    rows, cols = _chunk_spans(Sm[0][4], Sm[0][5], Sm[0][1])
    assert max(rows.max(), cols.max()) > RB_TILE, (rows.max(), cols.max())
    return types.SimpleNamespace(
        C=C, n=n, h=h, M=M, xform=xform, o=o, d=d, active=active, ids=ids, f=f, S=Sm, act=act,
        gd=rng.normal(size=(3, n)).astype(np.float32), gdiv=rng.normal(size=n).astype(np.float32),
        dh=rng.normal(size=(H, W)).astype(np.float32), do=rng.normal(size=(3, n)).astype(np.float32),
        dd=rng.normal(size=(3, n)).astype(np.float32), dM=(0.1 * rng.normal(size=12)).astype(np.float32))


def _reparam_shape(hf, c):
    kw = dict(to_world=c.M, differentiable_to_world=True) if c.xform else {}
    return hf.Heightfield(heightfield=torch.from_numpy(c.h).cuda(), max_height=S_REPARAM, **kw)


@pytest.mark.parametrize("xform", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_reparam_backward_tangent_and_backward_full(hf, oracle, monkeypatch, C, xform):
    c = _reparam_case(oracle, C, xform)
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(o=c.o, d=c.d, gd=c.gd, gdiv=c.gdiv, active=c.active,
                                                         ids=c.ids.view(np.int32), dh=c.dh, do=c.do, dd=c.dd, dM=c.dM).items()}
    shape = _reparam_shape(hf, c)
    ray = hf.Ray3f(t["o"], t["d"])
    kw = dict(active=t["active"], ray_index=t["ids"], **REPARAM)

    def run():
        # hf_reparam_backward: what backward() runs when only the heights are differentiated
        shape.heightfield.requires_grad_(True)
        dirn, det = hf.reparameterize_ray(shape, ray, **kw)
        ((dirn * t["gd"]).sum() + (det * t["gdiv"]).sum()).backward()
        gh_b, shape.heightfield.grad = shape.heightfield.grad, None
        shape.heightfield.requires_grad_(False)
        # hf_reparam_tangent: the heights alone (the oracle's forward mode), and every tangent at once
        th = hf.reparameterize_ray_tangent(shape, ray, dheights=t["dh"], **kw)
        ta = hf.reparameterize_ray_tangent(shape, ray, dheights=t["dh"], d_o=t["do"], d_d=t["dd"],
                                           d_to_world=t["dM"] if xform else None, **kw)
        # hf_reparam_backward_full: all its outputs
        full = hf.reparameterize_ray_adjoint(shape, ray, t["gd"], t["gdiv"], heights=True, o=True, d=True, to_world=xform, **kw)
        return gh_b, th, ta, full

    plain, (gh_b, th, ta, (gh, go, gd, gM)) = _both(c.n, C, run)
    for k in range(2):
        _same_bytes(th[k], plain[1][k], "hf_reparam_tangent (heights)"); _same_bytes(ta[k], plain[2][k], "hf_reparam_tangent")
    _same_bytes(go, plain[3][1], "grad_o"); _same_bytes(gd, plain[3][2], "grad_d")
    with oracle.with_ray_ids(c.ids):
        rh, ro, rd = oracle.reparam_backward(c.f, c.o, c.d, c.gd, c.gdiv, active=c.active, ray_grads=True, **REPARAM)
    assert np.linalg.norm(rh) > 0 and np.linalg.norm(ro) > 0 and np.linalg.norm(rd) > 0
    what = f"reparam C={C} to_world={xform}"
    # the heights against the oracle, 3e-5 (tests/test_reparam.py::test_gpu_reparameterize_ray_matches_oracle,
    # tests/test_gpu_reparam_backward_full.py::test_matches_the_oracle)
    e_b, e_h = _rel(gh_b, rh), _rel(gh, rh)
    print(f"{what}: heights vs the oracle: hf_reparam_backward {e_b:.3g}, hf_reparam_backward_full {e_h:.3g}"
          f" (without the hook {_rel(plain[0], rh):.3g}, {_rel(plain[3][0], rh):.3g})")
    assert e_b <= 3e-5 and e_h <= 3e-5, (e_b, e_h)
    off = t["active"] == 0
    assert bool((go[:, off] == 0).all()) and bool((gd[:, off] == 0).all())
    assert bool((th[0][:, off] == 0).all()) and bool((th[1][off] == 0).all())
    if not xform:
        # the ray against the oracle, 2e-4 (test_matches_the_oracle); the heights' tangent against the oracle's forward
        # mode, 2e-4 (tests/test_gpu_reparam_tangent.py::test_heights_tangent_matches_the_oracle)
        e_o, e_d = _rel(go, ro), _rel(gd, rd)
        with oracle.with_ray_ids(c.ids):
            rV, rdiv = oracle.reparam_forward(c.f, c.o, c.d, c.dh.astype(np.float64), active=c.active, **REPARAM)
        e_V, e_div = _rel(th[0], rV), _rel(th[1], rdiv)
        print(f"{what}: grad_o {e_o:.3g} grad_d {e_d:.3g} V_theta {e_V:.3g} div {e_div:.3g}")
        assert e_o <= 2e-4 and e_d <= 2e-4, (e_o, e_d)
        assert np.abs(rV).max() > 0 and e_V <= 2e-4 and e_div <= 2e-4, (e_V, e_div)
        return
    # to_world, and the ray under a transform: no bound exists for the twelve sums, so the error of the per-sample path
    # against the same float64 values is measured on the same inputs and the fused error may be at most twice that
    # (tests/test_gpu_reparam_backward_full.py::_fused_vs_per_sample); the heights of the two paths: the same sums
    from hf_amd import shape as sh
    with _grid(None), monkeypatch.context() as mp:
        mp.setattr(sh, "REPARAM_FUSED", False)
        ps = _reparam_shape(hf, c)
        ps.heightfield.requires_grad_(True)
        ol, dl = t["o"].clone().requires_grad_(True), t["d"].clone().requires_grad_(True)
        tw = torch.as_tensor(c.M, dtype=torch.float64).requires_grad_(True)
        ps.to_world = tw
        ps.parameters_changed(["to_world"])
        dirn, det = hf.reparameterize_ray(ps, hf.Ray3f(ol, dl), **kw)
        ((dirn * t["gd"]).sum() + (det * t["gdiv"]).sum()).backward()
        ph, po, pd, pM = ps.heightfield.grad, ol.grad, dl.grad, tw.grad
    _, _, _, rM = RB.reparam_backward(c.f, c.S, c.act, c.o, c.d, c.M, c.h, c.gd, c.gdiv)
    assert np.linalg.norm(rM) > 0
    for name, fused, per, ref, unforced in (("grad_to_world", gM.reshape(3, 4), pM, rM, plain[3][3].reshape(3, 4)),
                                            ("grad_o", go, po, ro, plain[3][1]), ("grad_d", gd, pd, rd, plain[3][2])):
        ef, ep = _rel(fused, ref), _rel(per, ref)
        print(f"{what} {name}: forced {ef:.3g} unforced {_rel(unforced, ref):.3g} per-sample {ep:.3g}")
        assert ef <= 2 * ep, (name, ef, ep)
    print(f"{what}: heights vs the per-sample path {_rel(gh, ph):.3g} (without the hook {_rel(plain[3][0], ph):.3g})")
    assert _rel(gh, ph) <= HEIGHTS_ATOMICS, _rel(gh, ph)


# ---- hf_adam_step ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask_updates,uniform", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_adam_step_bit_for_bit(hf, oracle, C, mask_updates, uniform):
    """37 x 53 = 1961 texels: 8 blocks without the hook.  One or two blocks forced: three or four iterations per wave
    (1961 > 768 C); three blocks: two or three, the ragged last block among them.  Uniform Adam's maximum of the second
    moments is then built across the iterations of a lane before the waves and blocks are combined."""
    from hf_amd import _capi
    lib = _capi.lib()
    rng = np.random.default_rng(5)
    Hh, Ww = 37, 53
    n = Hh * Ww
    h0 = rng.uniform(0.2, 0.8, (Hh, Ww)).astype(np.float32)
    with _grid(None):
        assert lib.hf_grid_blocks(n, 0) == -(-n // 256) == 8
    with _grid(C):
        blocks = lib.hf_grid_blocks(n, 0)
        assert blocks == C and (blocks < n / 768 if C < 3 else blocks < n / 512)
        shape = hf.Heightfield(heightfield=torch.from_numpy(h0).cuda(), max_height=0.5)
        opt = hf.Adam(shape, lr=0.03, beta_1=0.9, beta_2=0.99, epsilon=1e-8, mask_updates=mask_updates, uniform=uniform)
        h, m, v = h0.copy(), np.zeros_like(h0), np.zeros_like(h0)
        for step in range(1, 4):
            g = rng.normal(size=(Hh, Ww)).astype(np.float32)
            g[rng.uniform(size=(Hh, Ww)) < 0.3] = 0.0
            g[5, 0:64] = 0.0                                   # (a wave's worth of texels without a gradient)
            shape.heightfield.grad = torch.from_numpy(g).cuda()
            opt.step()
            h, m, v = oracle.adam_step(h, g, m, v, 0.03, 0.9, 0.99, 1e-8, step, mask_updates, uniform)
            assert np.array_equal(shape.heightfield.detach().cpu().numpy(), h), f"heights differ at step {step}"
            assert np.array_equal(opt.state[0].cpu().numpy(), m) and np.array_equal(opt.state[1].cpu().numpy(), v), step
        torch.cuda.synchronize()


# ---- hf_sample_position and its adjoint / tangent / _transform forms ---------------------------------------------------

@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_sample_position_and_its_derivatives(hf, C, smooth):
    import test_gpu_area_sampling as TA
    n = _n(C)
    rng = np.random.default_rng(300 + C)
    h = common.heights("sine", W, H, rng)
    T = common.affine(5)
    s = 0.6
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).cuda(), max_height=s, to_world=np.asarray(T, np.float64),
                           face_normals=not smooth, differentiable_to_world=True)
    T64 = T.astype(np.float64)
    # the forward: index exactness and b, p, n, uv against the restatement, as test_gpu_area_sampling._check_samples does
    p0, p1 = _both(n, C, lambda: TA._check_samples(shape, h, s, T64, False, smooth, n, seed=C))
    for k in ("p", "n", "uv", "pdf", "prim_index", "b"):
        _same_bytes(getattr(p1, k), getattr(p0, k), f"sample_position {k}")
    # a mask (one wave's worth of inactive lanes in its second iteration), the adjoints and the tangents
    act_np = rng.uniform(size=n) < 0.85
    act_np[256 * C:256 * C + 64] = False
    assert 0.2 < act_np.mean() < 0.9
    act, smp = torch.from_numpy(act_np).cuda(), TA._samples(n, 7 + C)
    gen = torch.Generator(device="cpu").manual_seed(8)
    gp, gn = torch.randn((3, n), generator=gen).cuda(), torch.randn((3, n), generator=gen).cuda()
    dh, dM = torch.randn((H, W), generator=gen).cuda(), torch.randn(12, generator=gen).cuda()

    def run():
        ps = shape.sample_position(0.0, smp, act)
        gtw = torch.zeros(12, device="cuda")
        grad_x = shape.sample_position_adjoint(ps, gp, gn, active=act, grad_to_world=gtw)   # _adjoint_transform
        grad = shape.sample_position_adjoint(ps, gp, gn, active=act)                          # _adjoint
        tan = shape.sample_position_tangent(ps, dh, active=act)                               # _tangent
        tan_x = shape.sample_position_tangent(ps, dh, active=act, d_to_world=dM)              # _tangent_transform
        return ps, grad_x, grad, gtw, tan, tan_x

    plain, (ps, grad_x, grad, gtw, tan, tan_x) = _both(n, C, run)
    for k in ("p", "n", "uv", "pdf", "prim_index", "b"):
        _same_bytes(getattr(ps, k), getattr(plain[0], k), f"masked sample_position {k}")
    for k in range(2):
        _same_bytes(tan[k], plain[4][k], "sample_position_tangent"); _same_bytes(tan_x[k], plain[5][k], "sample_position_tangent_transform")
    prim, bx, by = ps.prim_index.long()[act], ps.b[0].double()[act], ps.b[1].double()[act]
    g6 = torch.cat([gp, gn])[:, act].double()

    def block(hd, tw):
        return X.sample_block(hd, s, tw, False, prim, bx, by, smooth)
    # heights: float64 autograd, 1e-4 of the largest entry (test_gpu_area_sampling.py::test_adjoint_and_tangent_against_float64)
    hd = torch.from_numpy(h).double().cuda().requires_grad_(True)
    (block(hd, torch.from_numpy(T64).cuda()) * g6).sum().backward()
    for got in (grad, grad_x):
        assert float((got.double() - hd.grad).abs().max()) <= 1e-4 * float(hd.grad.abs().max())
    _, jv = torch.func.jvp(lambda x: block(x, torch.from_numpy(T64).cuda()), (hd.detach(),), (dh.double(),))
    got = torch.cat([tan[0], tan[1]])
    assert float((got[0:3, act].double() - jv[0:3]).abs().max()) <= 1e-4 * float(jv[0:3].abs().max())
    assert float((got[3:6, act].double() - jv[3:6]).abs().max()) <= 1e-4 * float(jv[3:6].abs().max())
    assert bool((got[:, ~act] == 0).all())
    # to_world: float64 central differences, 2e-3 of the norm; the tangent is the transpose, 1e-4 of the terms' scale
    # (test_gpu_transform_grad.py::test_sample_position_adjoint_fd_and_tangent_transpose)
    hc, gc = torch.from_numpy(h).double(), g6.cpu()
    pc, bxc, byc = prim.cpu(), bx.cpu(), by.cpu()
    fd = X.fd_to_world(lambda t: (X.sample_block(hc, s, t, False, pc, bxc, byc, smooth) * gc).sum(), T64)
    got = gtw.double().cpu().numpy().reshape(3, 4)
    assert np.linalg.norm(got - fd) <= 2e-3 * np.linalg.norm(fd), (got, fd)
    per = (torch.cat([tan_x[0], tan_x[1]]).double() * torch.cat([gp, gn]).double()).sum(0)
    lhs = float(per.sum())
    rhs = float((grad_x.double() * dh.double()).sum() + (gtw.double() * dM.double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * float(per.abs().sum()), (lhs, rhs)


# ---- hf_eval_attribute and its adjoint / tangent ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vertex_a1", "vertex_a3", "face_a1", "face_a3"])
@pytest.mark.parametrize("C", [1, 3])
def test_eval_attribute_and_its_derivatives(hf, C, name):
    import test_gpu_attributes as TA
    n = _n(C)
    shape, h, s, T, ray, active = TA._setup(hf, W, H, "affine", n=n, seed=C)     # a 129 x 65 noise field, random rays, a mask
    mb = common.to_world_rays(_miss_block().astype(np.float32), T.astype(np.float32))
    ray.o[:, 256 * C:256 * C + 64] = torch.from_numpy(mb[0:3]).cuda()
    ray.d[:, 256 * C:256 * C + 64] = torch.from_numpy(mb[3:6]).cuda()
    si = shape.ray_intersect(ray)                                                # (the traversal: not a grid_for launch)
    hit = si.is_valid() & active
    hit_np = hit.cpu().numpy()
    vi, vj = RT.tri_vertices(W, np.where(si.is_valid().cpu().numpy(), si.prim_index.cpu().numpy().view(np.uint32), 0))
    _assert_wave_shape(C, si.is_valid().cpu().numpy(), vi, vj, hit_np, ATTR_TILE)
    kind, size = name.split("_")[0], shape._attr_meta[name][1]
    gen = torch.Generator(device="cuda").manual_seed(9 + size)
    g = torch.randn((size, n), device="cuda", generator=gen)
    da = torch.randn(shape.attributes[name].numel(), device="cuda", generator=gen)
    dp, dh = torch.randn((3, n), device="cuda", generator=gen), torch.randn((H, W), device="cuda", generator=gen)

    def run():
        val = shape.eval_attribute_1(name, si, active)[None] if size == 1 else shape.eval_attribute_3(name, si, active)
        ga, gp, gh = shape.eval_attribute_adjoint(name, si, g, active)
        tan = shape.eval_attribute_tangent(name, si, da, dp, dh, active)
        return val, ga, gp, gh, tan

    plain, (val, ga, gp, gh, tan) = _both(n, C, run)
    _same_bytes(val, plain[0], "eval_attribute"); _same_bytes(tan, plain[4], "eval_attribute_tangent")
    # forward: 1e-5 of the largest value, misses and inactive lanes 0, a face attribute exact
    # (test_gpu_attributes.py::test_forward_parity)
    ref = TA._ref(shape, name, h, s, T, si, hit, device_rounding=True).T
    assert float((val.double() - ref).abs().max() / ref.abs().max()) <= 1e-5
    assert bool((val[:, ~hit] == 0).all())
    if kind == "face":
        assert torch.equal(val[:, hit].double(), ref[:, hit])
    # reverse: float64 autograd, 1e-5 relative L2 (2e-5 for the heights) (test_gpu_attributes.py::test_adjoint_against_float64_autograd)
    attr = shape.attributes[name].double().reshape(-1, size).requires_grad_(True)
    h64 = torch.from_numpy(h).double().cuda().requires_grad_(True)
    p64 = si.p.T.double().contiguous().requires_grad_(True)
    (AR.value(kind, attr, h64, s, T, si.prim_index.long(), p64, hit) * g.T.double()).sum().backward()
    e_a = _rel(ga, attr.grad.reshape(-1))
    print(f"eval_attribute_adjoint {name} C={C}: dL/dattr {e_a:.3g}")
    assert e_a <= 1e-5, (name, e_a)
    if kind == "vertex":
        _same_bytes(gp, plain[2], "dL/dp")
        e_p, e_h = _rel(gp.T, p64.grad), _rel(gh, h64.grad)
        print(f"eval_attribute_adjoint {name} C={C}: dL/dp {e_p:.3g} dL/dheight {e_h:.3g}")
        assert e_p <= 1e-5 and e_h <= 2e-5, (name, e_p, e_h)
        assert bool((gp[:, ~hit] == 0).all())
    else:
        assert gp is None and gh is None
    # forward mode: the transpose of the adjoint (test_gpu_attributes.py::test_tangent_is_the_transpose_and_repeatable)
    lhs = float((ga.double() * da.double()).sum())
    if gp is not None:
        lhs += float((gp.double() * dp.double()).sum() + (gh.double() * dh.double()).sum())
    rhs = float((g.double() * tan.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(rhs), 1e-3), (name, lhs, rhs)


# ---- hf_eval_parameterization and its adjoint / tangent ----------------------------------------------------------------

@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_eval_parameterization_and_its_derivatives(hf, C, smooth):
    import math
    import test_gpu_parameterization as TP
    n = _n(C)
    shape, h, s, T = TP._field(hf, W, H, "sine", tw="affine", smooth=smooth, seed=C, differentiable_to_world=True)
    rng = np.random.default_rng(400 + C)
    uvn = rng.uniform(-0.12, 1.12, (2, n)).astype(np.float32)        # queries all over the field, a fifth of them outside
    uvn[:, 256 * C:256 * C + 64] = 2.0
    act_np = rng.uniform(size=n) < 0.85
    valid, rprim, b1, b2 = PR.lookup(uvn[0], uvn[1], W, H, act_np)
    vi, vj = RT.tri_vertices(W, rprim)
    _assert_wave_shape(C, valid, vi, vj, valid, ADJ_TILE)
    uv, act = torch.from_numpy(uvn).cuda(), torch.from_numpy(act_np).cuda()
    act_u8 = act.to(torch.uint8)
    vm = torch.from_numpy(valid).cuda()
    flags = RAY_ALL | (0x20 if smooth else 0)
    g = TP._grads(n, 6)
    g[:, ~vm] = 0.0
    gen = torch.Generator(device="cpu").manual_seed(9)
    dh, dtw = torch.randn((H, W), generator=gen).cuda(), torch.randn(12, generator=gen).cuda()

    def run():
        rec, prim = TP._param(shape, uv, flags, act_u8)
        gtw = torch.zeros(12, device="cuda")
        gh_x = shape.eval_parameterization_adjoint(uv, g, flags, active=act, grad_to_world=gtw)
        gh = shape.eval_parameterization_adjoint(uv, g, flags, active=act)
        tan = shape.eval_parameterization_tangent(uv, dh, flags, active=act)
        tan_x = shape.eval_parameterization_tangent(uv, dh, flags, active=act, d_to_world=dtw)
        return rec, prim, gh_x, gh, gtw, tan, tan_x

    plain, (rec, prim, gh_x, gh, gtw, tan, tan_x) = _both(n, C, run)
    _same_bytes(rec, plain[0], "the record"); _same_bytes(prim, plain[1], "out_prim_index")
    _same_bytes(tan, plain[5], "eval_parameterization_tangent"); _same_bytes(tan_x, plain[6], "... with d_to_world")
    # the lookup bit for bit, the miss record, the record within 1e-5 of the restatement
    # (test_gpu_parameterization.py::test_lookup_bitwise_and_the_miss_record, ::test_record_bitwise_against_compute_surface_interaction)
    assert np.array_equal(prim.cpu().numpy().astype(np.int64), rprim)
    assert bool((rec[0][~vm] == math.inf).all()) and bool((rec[1:, ~vm] == 0).all()) and bool((rec[0][vm] == 1.0).all())
    hd = torch.from_numpy(h).double().requires_grad_(True)
    td = torch.from_numpy(T).requires_grad_(True)
    r = PR.record(hd, s, td, False, uvn[0][valid], uvn[1][valid], rprim[valid], b1[valid], b2[valid], flags, smooth)
    blk = PR.block(r)
    err = float((rec[:18, vm].cpu().double() - blk.detach()).abs().max())
    assert err <= 1e-5 * max(1.0, float(blk.detach().abs().max())), err
    # the adjoint: float64 autograd of the restatement, 2e-4 relative L2 for the heights and to_world
    # (test_gpu_parameterization.py::test_adjoint_against_hf_adjoint_and_float64)
    gv = g[:, vm].double().cpu()
    gv[0] = 0.0
    gv[7:9] = 0.0
    (blk * gv).sum().backward()
    e_x, e_h, e_tw = _rel(gh_x, hd.grad), _rel(gh, hd.grad), _rel(gtw.reshape(3, 4), td.grad)
    print(f"eval_parameterization_adjoint C={C} smooth={smooth}: heights {e_x:.3g} / {e_h:.3g}, to_world {e_tw:.3g}")
    assert e_x <= 2e-4 and e_h <= 2e-4 and e_tw <= 2e-4, (e_x, e_h, e_tw)
    # the tangent: bitwise hf_tangent(FollowShape)'s on the UV-space rays (::test_tangent_against_hf_tangent_and_repeatable)
    o, d, maxt, t, bb, pp = TP._synth(uv, torch.from_numpy(rprim).int().cuda(), torch.from_numpy(np.stack([b1, b2])).cuda())
    t = torch.where(vm, t, torch.full_like(t, math.inf))
    with _grid(None):
        ref = shape.tangent(hf.Ray3f(o, d, maxt), hf.PreliminaryIntersection3f(t, bb, pp, shape), dh,
                            ray_flags=flags | RAY_FOLLOWSHAPE, d_to_world=dtw)
    assert bool((tan_x[0] == 0).all()) and bool((tan_x[7:9] == 0).all()) and bool((tan_x[:, ~vm] == 0).all())
    assert torch.equal(tan_x[1:7], ref[1:7]) and torch.equal(tan_x[9:], ref[9:])

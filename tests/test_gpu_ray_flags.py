"""Every RayFlags set on the GPU: the record, its adjoint and its tangent on flat and smooth handles, flipped normals and
three transforms (identity, a general affine, a mirror with shear: world-space normals up and down), against
  * each other: the fused trace on the wide and on the ordinary path, the unfused hf_compute_surface_interaction and
    the lean (incoherent) kernels give the same bytes in every row, hits and misses;
  * the oracle: t, prim_index and prim_uv bit-exact;
  * the float64 restatement of tests/smooth_ref.py (itself checked against the oracle and central differences on the
    CPU, tests/test_oracle_gradients_fd.py): every row a flag set defines, and the documented contents of the others;
    autograd of it for hf_adjoint / hf_adjoint_rows (heights and rays), its JVP for hf_tangent, central differences over
    to_world (xform_ref.fd_to_world) for the transform derivatives, and the Python mirror's sh_frame / wi backward.
Without dPdUV, dp_du / dp_dv = coordinate_system(n) of the face normal before flip_normals (mesh.cpp:762), attached.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import common
import si_numpy as S
import smooth_ref as R
import xform_ref as X

pytestmark = pytest.mark.gpu

FLAGS = S.FLAG_SUBSETS + [S.RAY_MINIMAL]
NO_DPDUV = [f for f in FLAGS if not f & S.RAY_DPDUV]
MODES = {"default": 0, "follow": S.RAY_FOLLOWSHAPE, "detach": S.RAY_DETACHSHAPE}
# 28 rows of the raw record: name -> rows
REC = {"t": [0], "boundary_test": [1], "uv": [2, 3], "p": [4, 5, 6], "n": [7, 8, 9], "sh_n": [10, 11, 12],
       "dp_du": [13, 14, 15], "dp_dv": [16, 17, 18], "sh_s": [19, 20, 21], "sh_t": [22, 23, 24], "wi": [25, 26, 27]}
SENTINEL = 7.0


TRANSFORMS = {"identity": np.eye(4)[:3].astype(np.float32), "affine": common.affine(4), "mirror_shear": common.mirror_shear()}
# (W, H, transform, flip, smooth, blocks of 256 rays that hit / that pass beside the field)
SCENES = [(2, 2, "identity", False, False, 4, 2), (9, 7, "affine", True, True, 6, 2), (9, 7, "mirror_shear", False, False, 6, 2),
          (33, 17, "mirror_shear", True, True, 8, 4), (33, 17, "affine", False, False, 8, 4),
          (257, 257, "identity", True, True, 8, 4)]


def _scene(hf, W, H, xf, flip, smooth, nhit, nmiss, seed, diff_tw=False):
    rng = np.random.default_rng(seed)
    s = 0.6
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32) if W < 100 else common.heights("sine", W, H, rng)
    tw = TRANSFORMS[xf]
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).cuda(), max_height=s, to_world=np.asarray(tw, np.float64),
                           flip_normals=flip, face_normals=not smooth, differentiable_to_world=diff_tw)
    blocks = []
    for b in range(nhit + nmiss):
        if b % 3 == 1 and nmiss > 0:       # 256 rays beside the field: one fetch that misses as a whole
            nmiss -= 1
            c = np.stack([rng.uniform(1.5, 4.0) * rng.choice([-1, 1]) + rng.uniform(-0.1, 0.1, 256),
                          rng.uniform(-0.9, 0.9, 256), np.full(256, 2.0)])
            d = np.array([[1e-3], [2e-3], [-1.0]]) + rng.normal(size=(3, 256)) * 1e-4
            blocks.append(np.concatenate([c, d, np.full((1, 256), np.inf)]).astype(np.float32))
        else:
            blocks.append(common.random_rays(256, rng, s))
    r = common.to_world_rays(np.concatenate(blocks, 1), tw)
    return rng, h, s, tw, shape, r


def _ray(hf, r):
    rt = torch.from_numpy(r).cuda()
    return hf.Ray3f(rt[0:3].contiguous(), rt[3:6].contiguous(), rt[6].contiguous())


def _launch(shape, r, flags, shift, pi_in=None):
    """the raw record of hf_ray_intersect (pi_in None) or of hf_compute_surface_interaction on pi_in [4, n], every
    row starting `shift` floats into its allocation; the buffers are filled with SENTINEL first"""
    from hf_amd import _capi
    lib = _capi.lib()
    n = r.shape[1]
    P = n + 8
    rays = torch.zeros((7, P), device="cuda"); rays[:, shift:shift + n] = torch.from_numpy(r).cuda()
    pib = torch.full((4, P), SENTINEL, device="cuda"); sib = torch.full((28, P), SENTINEL, device="cuda")
    if pi_in is not None:
        pib[:, shift:shift + n] = pi_in
    base = lambda b, k: b.data_ptr() + 4 * (P * k + shift)
    rs = _capi.hf_rays_t()
    for k in range(3):
        rs.o[k] = base(rays, k); rs.d[k] = base(rays, 3 + k)
    rs.maxt = base(rays, 6)
    pi = _capi.hf_pi_t(); pi.t, pi.prim_uv[0], pi.prim_uv[1], pi.prim_index = (base(pib, k) for k in range(4))
    si = _capi.hf_si_t()
    rows = [base(sib, k) for k in range(28)]
    si.t, si.boundary_test, si.uv[0], si.uv[1] = rows[0], rows[1], rows[2], rows[3]
    for c in range(3):
        si.p[c], si.n[c], si.sh_n[c], si.dp_du[c] = rows[4 + c], rows[7 + c], rows[10 + c], rows[13 + c]
        si.dp_dv[c], si.sh_s[c], si.sh_t[c], si.wi[c] = rows[16 + c], rows[19 + c], rows[22 + c], rows[25 + c]
    if pi_in is None:
        _capi.check(lib.hf_ray_intersect(shape._h, n, C.byref(rs), flags, None, C.byref(pi), C.byref(si), None))
    else:
        _capi.check(lib.hf_compute_surface_interaction(shape._h, n, C.byref(rs), C.byref(pi), flags, None, C.byref(si), None))
    torch.cuda.synchronize()
    assert bool((sib[:, :shift] == SENTINEL).all()) and bool((sib[:, shift + n:] == SENTINEL).all())
    return pib[:, shift:shift + n].clone(), sib[:, shift:shift + n].clone()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _ref_inputs(r, pib):
    t = pib[0].cpu().numpy()
    hit = np.isfinite(t)
    o = torch.from_numpy(r[0:3, hit].T.astype(np.float64))
    d = torch.from_numpy(r[3:6, hit].T.astype(np.float64))
    prim = torch.from_numpy(pib[3].view(torch.int32).cpu().numpy()[hit].astype(np.int64))
    uv = pib[1:3].cpu().double()[:, torch.from_numpy(hit)]
    return hit, o, d, prim, (uv[0], uv[1])


def _steady(ref, d):
    """hits away from grazing incidence and from the sign switch of coordinate_system (|n.z| small)"""
    n = ref["n"]
    cos = (n * d).sum(-1).abs() / d.norm(dim=-1)
    return (cos > 1e-2) & (n[:, 2].abs() > 1e-2)


# ---- 1. forward ---------------------------------------------------------------------------------------------------

def test_record_of_every_flag_set(hf, oracle):
    """per scene and flag set (17 x with / without BoundaryTest x three modes): the four launches bitwise equal; t,
    prim_index, prim_uv bit-exact against the oracle; the defined rows against the float64 restatement; the undefined
    ones as documented; the miss records"""
    old = os.environ.get("HF_FORCE_GRAB")
    checked = 0
    try:
        for si_, (W, H, xf, flip, smooth, nhit, nmiss) in enumerate(SCENES):
            rng, h, s, tw, shape, r = _scene(hf, W, H, xf, flip, smooth, nhit, nmiss, seed=100 + si_)
            n = r.shape[1]
            f = oracle.OracleField(h, max_height=s, to_world=tw, flip_normals=flip)
            t_o, u_o, v_o, prim_o = f.ray_intersect_preliminary(r)
            hit = np.isfinite(t_o)
            assert 0.1 < hit.mean() < 0.95
            h64 = torch.from_numpy(h.astype(np.float64))
            for mode, mb in MODES.items():
                for sub in FLAGS:
                    for bt in (0, S.RAY_BOUNDARYTEST):
                        flags = sub | mb | bt
                        os.environ["HF_FORCE_GRAB"] = "256"
                        pw, sw = _launch(shape, r, flags, 0)            # aligned rows: the wide path
                        po, so = _launch(shape, r, flags, 1)            # shifted rows: the ordinary path
                        if old is None:
                            del os.environ["HF_FORCE_GRAB"]
                        else:
                            os.environ["HF_FORCE_GRAB"] = old
                        pu, su = _launch(shape, r, flags, 0, pi_in=pw)  # unfused
                        shape.set_ray_coherence(hf.Heightfield.COHERENCE_INCOHERENT)
                        try:
                            pl, sl = _launch(shape, r, flags, 1)        # the lean kernels
                        finally:
                            shape.set_ray_coherence(hf.Heightfield.COHERENCE_AUTO)
                        for p_, s_ in ((po, so), (pl, sl)):
                            assert torch.equal(_bits(pw), _bits(p_)) and torch.equal(_bits(sw), _bits(s_)), (xf, flags)
                        assert torch.equal(_bits(sw), _bits(su)), (xf, flags)
                        if sub == FLAGS[0] and bt == 0:
                            assert np.array_equal(pw[0].cpu().numpy().view(np.uint32), t_o.view(np.uint32))
                            assert np.array_equal(pw[1].cpu().numpy().view(np.uint32), u_o.view(np.uint32))
                            assert np.array_equal(pw[2].cpu().numpy().view(np.uint32), v_o.view(np.uint32))
                            assert np.array_equal(pw[3].view(torch.int32).cpu().numpy().view(np.uint32), prim_o)
                        rec = sw.cpu()
                        m = torch.from_numpy(~hit)
                        # misses: t = inf, wi = -d, boundary_test = 1e8 (BoundaryTest) else untouched, the rest 0
                        assert torch.all(torch.isinf(rec[0, m]))
                        assert torch.equal(rec[25:28][:, m], -torch.from_numpy(r[3:6])[:, m])
                        assert torch.all(rec[1, m] == (1e8 if bt else SENTINEL))
                        assert torch.all(rec[2:25][:, m] == 0)
                        # hits: the rows a flag set does not define
                        hm = torch.from_numpy(hit)
                        if not bt:
                            assert torch.all(rec[1, hm] == SENTINEL)
                        else:
                            assert torch.all(rec[1, hm] >= 0) and torch.all(rec[1, hm] <= 1e3)
                        if not sub & S.RAY_SHADINGFRAME:
                            assert torch.all(rec[19:25][:, hm] == 0)
                        if not sub & (S.RAY_UV | S.RAY_DPDUV):
                            assert torch.equal(_bits(rec[2:4][:, hm]), _bits(pw[1:3].cpu()[:, hm]))
                        # the defined rows against the restatement (the three modes give the same record up to the
                        # rounding of FollowShape's t: checked in every mode)
                        hit_, o, d, prim, b = _ref_inputs(r, pw)
                        ref = R.surface(h64, s, torch.from_numpy(tw.astype(np.float64)), flip, o, d, prim, b, "follow",
                                        flags, smooth)
                        ok = _steady(ref, d)
                        for nm in ("t", "p", "n", "uv", "sh_n", "dp_du", "dp_dv", "sh_s", "sh_t", "wi"):
                            got = rec[REC[nm]][:, hm].double().T
                            want = ref[nm].reshape(got.shape)
                            sel = ok if nm in ("dp_du", "dp_dv", "sh_s", "sh_t", "wi") else torch.ones_like(ok)
                            assert torch.allclose(got[sel], want[sel], rtol=1e-4, atol=2e-5), \
                                (xf, flags, nm, float((got[sel] - want[sel]).abs().max()))
                        checked += 1
    finally:
        if old is None:
            os.environ.pop("HF_FORCE_GRAB", None)
        else:
            os.environ["HF_FORCE_GRAB"] = old
    assert checked == len(SCENES) * len(MODES) * len(FLAGS) * 2


# ---- 2. adjoint, 3. tangent -----------------------------------------------------------------------------------------

def _block_fn(h, s, tw, flip, prim, b, mode, flags, smooth):
    tw64 = torch.from_numpy(tw.astype(np.float64))

    def fn(hh, o, d):
        return X.si_block(hh, s, tw64, flip, o, d, prim, b, mode, smooth, flags=flags)
    return fn


def test_adjoint_and_tangent_of_every_flag_set(hf):
    """hf_adjoint_rows (and hf_adjoint, and the smooth adjoint on smooth handles) against autograd of the restatement
    on all 18 rows, heights and rays; hf_tangent against its JVP; both per flag set, mode, scene"""
    from hf_amd import _capi
    lib = _capi.lib()
    for si_, (W, H, xf, flip, smooth, nhit, nmiss) in enumerate(SCENES[:5]):
        rng, h, s, tw, shape, r = _scene(hf, W, H, xf, flip, smooth, nhit, 0, seed=200 + si_)
        ray = _ray(hf, r)
        n = r.shape[1]
        pi = shape.ray_intersect_preliminary(ray)
        pib = torch.cat([pi.t[None], pi.prim_uv, pi.prim_index.view(torch.float32)[None]])
        hit, o, d, prim, b = _ref_inputs(r, pib)
        hm = torch.from_numpy(hit)
        h64 = torch.from_numpy(h.astype(np.float64))
        for mode, mb in MODES.items():
            for sub in FLAGS:
                flags = sub | mb
                fn = _block_fn(h, s, tw, flip, prim, b, mode, flags, smooth)
                ref = R.surface(h64, s, torch.from_numpy(tw.astype(np.float64)), flip, o, d, prim, b, mode, flags, smooth)
                keep = _steady(ref, d)
                g = torch.from_numpy(rng.normal(size=(18, n))).float()
                g[:, ~hm] = 0
                g[:, torch.where(hm)[0][~keep]] = 0          # grazing / sign-switch hits carry no upstream gradient
                gh, go, gd = shape.adjoint(ray, pi, g.cuda(), ray_flags=flags, ray_grads=True)
                hh = h64.clone().requires_grad_(True)
                oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
                (fn(hh, oo, dd) * g[:, hm].double()).sum().backward()
                gref = hh.grad if hh.grad is not None else torch.zeros_like(h64)
                scale = float(gref.abs().max()) + 1e-30
                if mode == "detach":
                    assert torch.all(gh == 0)
                else:
                    assert torch.allclose(gh.cpu().double(), gref, rtol=2e-4, atol=2e-4 * scale), \
                        (xf, flags, float((gh.cpu().double() - gref).abs().max()) / scale)
                for got, want in ((go, oo.grad), (gd, dd.grad)):
                    want = want.T
                    sc = float(want.abs().max()) + 1e-30
                    assert torch.allclose(got.cpu().double()[:, hm], want, rtol=2e-4, atol=2e-4 * sc), (xf, flags)
                if not smooth and sub in (NO_DPDUV[1], S.RAY_SHADINGFRAME):   # hf_adjoint = hf_adjoint_rows
                    gh2 = torch.zeros_like(gh)
                    gs = shape._rays_struct(ray.o, ray.d, ray.maxt)
                    gg = g.cuda().contiguous()
                    from hf_amd.shape import _fill, _rows, _DIFF_ROWS
                    gst = _fill(_capi.hf_si_grad_t(), _DIFF_ROWS, _rows(gg, n))
                    pis = shape._pi_struct(pi.t, pi.prim_uv, pi.prim_index)
                    _capi.check(lib.hf_adjoint(shape._h, n, C.byref(gs), C.byref(pis), flags, None, C.byref(gst),
                                               gh2.data_ptr(), None, None, None))
                    torch.cuda.synchronize()
                    assert torch.allclose(gh2, gh, rtol=1e-5, atol=1e-5 * float(gh.abs().max() + 1e-30))
                # tangent: the JVP of the restatement
                dh = torch.from_numpy(rng.normal(size=(H, W)))
                do = torch.from_numpy(rng.normal(size=(3, n))); ddd = torch.from_numpy(rng.normal(size=(3, n)))
                tg = shape.tangent(ray, pi, dh.float().cuda(), do.float().cuda(), ddd.float().cuda(), ray_flags=flags).cpu()
                assert torch.all(tg[:, ~hm] == 0)
                _, jv = torch.func.jvp(fn, (h64, o, d), (dh, do.T[hm].contiguous(), ddd.T[hm].contiguous()))
                got = tg[:, hm].double()[:, keep]
                want = jv[:, keep]
                tol = 2e-4 * want.abs() + 2e-4 * (1 + want.abs().amax(0, keepdim=True))   # per ray, as test_gpu_tangent
                assert bool(((got - want).abs() <= tol).all()), (xf, flags, mode, float((got - want).abs().max()))


def _transpose_check(shape, ray, pi, flags, seed):
    n = len(ray)
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    ybar = torch.randn((18, n), device="cuda", generator=gen)
    dh = torch.randn((shape.height, shape.width), device="cuda", generator=gen)
    do = torch.randn((3, n), device="cuda", generator=gen)
    dd = torch.randn((3, n), device="cuda", generator=gen)
    per_ray = (ybar.double() * shape.tangent(ray, pi, dh, do, dd, ray_flags=flags).double()).sum(0)
    lhs, scale = float(per_ray.sum()), float(per_ray.abs().sum())
    gh, go, gd = shape.adjoint(ray, pi, ybar, ray_flags=flags, ray_grads=True)
    rhs = float((dh.double() * gh.double()).sum() + (do.double() * go.double()).sum() + (dd.double() * gd.double()).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (flags, lhs, rhs, scale)


def test_tangent_is_the_transpose_of_the_adjoint(hf):
    """<ybar, J delta> = <J^T ybar, delta> for every flag set and mode on flat and smooth handles, and at configs[1]
    size (1024^2 sine field, 512^2 x 16 rays) for UV | ShadingFrame, ShadingFrame | dNSdUV and dNSdUV"""
    for si_, (W, H, xf, flip, smooth, nhit, nmiss) in enumerate(SCENES[1:4]):
        rng, h, s, tw, shape, r = _scene(hf, W, H, xf, flip, smooth, nhit, nmiss, seed=300 + si_)
        ray = _ray(hf, r)
        pi = shape.ray_intersect_preliminary(ray)
        for mb in MODES.values():
            for k, sub in enumerate(FLAGS):
                _transpose_check(shape, ray, pi, sub | mb, seed=k)
    h = hf.workload.sine_heights(1024, 1024, device="cuda")
    rays = hf.workload.ortho_rays(512, 512, 16, "cuda")
    ray = hf.Ray3f(rays[0:3].contiguous(), rays[3:6].contiguous(), rays[6].contiguous())
    for smooth in (False, True):
        shape = hf.Heightfield(heightfield=h, max_height=0.5, face_normals=not smooth)
        pi = shape.ray_intersect_preliminary(ray)
        assert int(pi.is_valid().sum()) > 100000
        for sub in (S.RAY_UV | S.RAY_SHADINGFRAME, S.RAY_SHADINGFRAME | S.RAY_DNSDUV, S.RAY_DNSDUV):
            _transpose_check(shape, ray, pi, sub, seed=sub)


# ---- 4. transform derivatives ---------------------------------------------------------------------------------------

def test_transform_derivatives_without_dpduv(hf):
    """hf_adjoint_transform against central differences over to_world of the restatement, and hf_tangent_transform
    by transposition with it, for the flag sets without dPdUV, flat and smooth"""
    for smooth in (False, True):
        rng, h, s, tw, shape, r = _scene(hf, 9, 7, "mirror_shear" if smooth else "affine", smooth, smooth, 4, 0,
                                         seed=400 + smooth, diff_tw=True)
        ray = _ray(hf, r)
        pi = shape.ray_intersect_preliminary(ray)
        pib = torch.cat([pi.t[None], pi.prim_uv, pi.prim_index.view(torch.float32)[None]])
        hit, o, d, prim, b = _ref_inputs(r, pib)
        hm = torch.from_numpy(hit)
        hd = torch.from_numpy(h).double()
        ref = R.surface(hd, s, torch.from_numpy(tw.astype(np.float64)), smooth, o, d, prim, b, "default", S.RAY_ALL, smooth)
        keep = _steady(ref, d)
        for mode in ("default", "follow"):
            for sub in NO_DPDUV:
                flags = sub | MODES[mode]
                g = torch.from_numpy(rng.normal(size=(18, len(ray)))).float()
                g[:, ~hm] = 0
                g[:, torch.where(hm)[0][~keep]] = 0
                gtw = torch.zeros(12, dtype=torch.float32, device="cuda")
                shape.adjoint(ray, pi, g.cuda(), ray_flags=flags, grad_to_world=gtw)
                got = gtw.cpu().double().numpy().reshape(3, 4)
                gh = g[:, hm].double()
                fd = X.fd_to_world(lambda t: (X.si_block(hd, s, t, smooth, o, d, prim, b, mode, smooth, flags=flags)
                                              * gh).sum(), tw)
                err = np.linalg.norm(got - fd) / np.linalg.norm(fd)
                assert err < 2e-3, (smooth, mode, flags, err)
                for k in (0, 6, 10):
                    dM = torch.zeros(12, device="cuda"); dM[k] = 1.0
                    jd = shape.tangent(ray, pi, d_to_world=dM, ray_flags=flags)
                    assert abs(float((jd.double() * g.cuda().double()).sum()) - got.reshape(-1)[k]) \
                        <= 1e-4 * np.abs(got).sum() + 1e-6, (smooth, mode, flags, k)


# ---- 5. the Python mirror -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [False, True])
def test_shading_frame_backward_without_dpduv(hf, smooth):
    """ray_intersect(ray, UV | ShadingFrame), a loss on sh_frame.s, sh_frame.t and wi, backward(): heightfield.grad
    equals the same chain in torch float64"""
    W, H = 33, 17
    rng, h, s, tw, shape, r = _scene(hf, W, H, "affine", True, smooth, 8, 0, seed=500 + smooth)
    ray = _ray(hf, r)
    flags = S.RAY_UV | S.RAY_SHADINGFRAME
    shape.heightfield.requires_grad_(True)
    si = shape.ray_intersect(ray, flags)
    hit = si.is_valid()
    n = len(ray)
    w = torch.from_numpy(rng.normal(size=(9, n))).float().cuda() * hit[None]
    pib = torch.cat([si.t.detach()[None], si.prim_uv, si.prim_index.view(torch.float32)[None]])
    _, o, d, prim, b = _ref_inputs(r, pib)
    hd = torch.from_numpy(h.astype(np.float64))
    ref = R.surface(hd, s, torch.from_numpy(tw.astype(np.float64)), True, o, d, prim, b, "default", flags, smooth)
    keep = torch.zeros(n, dtype=torch.bool)
    keep[torch.where(hit.cpu())[0][_steady(ref, d)]] = True
    w = w * keep.cuda()[None]
    loss = (w[0:3] * si.sh_frame.s).sum() + (w[3:6] * si.sh_frame.t).sum() + (w[6:9] * si.wi).sum()
    loss.backward()
    got = shape.heightfield.grad.double().cpu()
    hh = hd.clone().requires_grad_(True)
    ref = R.surface(hh, s, torch.from_numpy(tw.astype(np.float64)), True, o, d, prim, b, "default", flags, smooth)
    wh = w[:, hit].double().cpu().T
    ((ref["sh_s"] * wh[:, 0:3]).sum() + (ref["sh_t"] * wh[:, 3:6]).sum() + (ref["wi"] * wh[:, 6:9]).sum()).backward()
    scale = float(hh.grad.abs().max())
    assert scale > 0
    assert torch.allclose(got, hh.grad, rtol=2e-4, atol=2e-4 * scale), float((got - hh.grad).abs().max()) / scale

"""The sensor on the GPU (hf_sensor_rays, _tangent, _adjoint, hf_sensor_project, _tangent, _adjoint; PerspectiveCamera,
OrthographicCamera) on the scenes of tests/sensor_ref.py: film 13 x 7, the crop window (3, 2, 5, 4) and none, spp 1, 3, 4
(n <= 364), both types under a generic look_at pose.
  (1) the rays against the float64 restatement (the reference's route through the five matrices), the orthographic type
      against workload.ortho_rays on the device, the perspective type against examples/inverse_pose.pinhole / film_position;
  (2) indexing, bit for bit: start / count, a shuffled pixel list, n = 0, guard bands with every optional pointer NULL in
      turn, both store variants on aligned and unaligned rows, a captured graph, repeatability; one HF_FORCE_GRID case
      per kernel; the reducer over more rows than it has threads;
  (3) the way back: masks exact, uv and weight against the restatement, project(ray(t)) = pos;
  (4) tangent and adjoint against the restatement, the transposition gap on the device through the public functions,
      backward and jvp through sample_rays -> ray_intersect -> sum(si.p[2]) against central differences;
  (5) examples/inverse_camera.py descends.

Tolerances.  Rays: the kernel forms everything in double and rounds once, so d is within 2^-23 (|d| <= 1), o within 2^-23
times its scale (max|c| + near max|v|; orthographic: max_k(|c_k| + |A_k0| + |A_k1| / a + |A_k2| near), a bound of |o|
from the inputs), maxt and pos within one float32 ulp -- a rounding plus double
noise.  Derivatives and the way back: scripts/sensor_f32_error.py runs the restatement in float32 against float64 on
exactly these scenes (profiles/sensor/f32_error.json; the maxima are F32 below) and the GPU is allowed four times that,
the project's rule.  The measured worst is printed by every test and recorded in DESIGN 4.23."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import sensor_ref as R
from row_helpers import _cu, guarded, intact, rows, transposition_gap

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

F32 = {"tangent_do": 7.68e-08, "tangent_dd": 8.18e-08, "adjoint": 2.29e-07, "project_uv": 2.42e-05, "project_weight": 5.07e-06,
       "project_duv": 1.70e-06, "project_dweight": 3.92e-05, "project_grad_p": 1.31e-06, "project_adjoint": 1.17e-06}
TOL = {k: 4 * v for k, v in F32.items()}
TYPES = [R.PERSPECTIVE, R.ORTHOGRAPHIC]
CROPS = [R.CROP, None]
EPS = 2.0 ** -23


def _np(x):
    return x.detach().cpu().numpy()


def _camera(hf, s, to_world=None, fov=None):
    tw = torch.tensor(s.to_world) if to_world is None else to_world
    kw = dict(film=s.film, near_clip=s.near, far_clip=s.far, crop=s.crop)
    if s.type == R.PERSPECTIVE:
        return hf.PerspectiveCamera(tw, s.fov if fov is None else fov, **kw)
    return hf.OrthographicCamera(tw, **kw)


def _ulp(ref):
    return np.spacing(np.abs(np.asarray(ref, np.float32))).astype(np.float64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


# ---- (1) the rays -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", R.SPPS)
@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("type_", TYPES)
def test_rays_equal_the_restatement(hf, type_, crop, spp):
    s = R.scene(type_, crop)
    ids, pos = R.wavefront(s, spp)
    ray, gpos, index = _camera(hf, s).sample_rays(spp, seed=R.SEED)
    assert len(ray) == len(ids) <= 364 and np.array_equal(_np(index), ids.astype(np.int32))
    o, d, maxt, _, _ = R.rays(s, pos)
    if type_ == R.PERSPECTIVE:
        wx, wy = R.closed_w(s, pos)
        tau = np.tan(s.fov * np.pi / 360)
        scale = np.abs(s.to_world[:, 3]).max() + s.near * np.sqrt((wx * tau) ** 2 + (wy * tau) ** 2 + 1).max()
    else:   # |o_k| <= |c_k| + |A_k0| |w.x| + |A_k1| |w.y| + |A_k2| near with |w.x| <= 1, |w.y| <= 1 / a: from the inputs alone
        M, a = np.abs(s.to_world), s.film[0] / s.film[1]
        scale = (M[:, 3] + M[:, 0] + M[:, 1] / a + M[:, 2] * s.near).max()
    worst = {"d": np.abs(_np(ray.d) - d).max() / EPS, "o": np.abs(_np(ray.o) - o).max() / (EPS * scale),
             "maxt": (np.abs(_np(ray.maxt) - maxt) / _ulp(maxt)).max(), "pos": (np.abs(_np(gpos) - pos) / _ulp(pos)).max()}
    print("worst error in units of the bound:", worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.abs(d).max() <= 1 + 1e-12 and (np.linalg.norm(_np(ray.d), axis=0) > 0.999).all()


@pytest.mark.parametrize("spp", R.SPPS)
def test_orthographic_equals_ortho_rays_on_the_device(hf, spp):
    kw = dict(origin=(1.5, 1.2, 1.1), target=(0.0, 0.1, 0.125), up=(0.0, 0.0, 1.0), scale=(1.6, 1.3, 1.0))
    want = hf.workload.ortho_rays(13, 7, spp, "cuda", seed=5, **kw)
    ray, pos, _ = hf.OrthographicCamera.look_at(film=(13, 7), **kw).sample_rays(spp, seed=5)
    assert _same(ray.d, want[3:6]) and _same(ray.maxt, want[6])
    gap = (np.abs(_np(ray.o).astype(np.float64) - _np(want[0:3])) / _ulp(_np(want[0:3]))).max()
    print("o: worst difference in ulps", gap)
    assert gap <= 1.0
    assert _same(pos, hf.workload.film_positions(13, 7, spp, "cuda", seed=5))


def test_perspective_equals_the_pinhole_of_inverse_pose(hf):
    """PerspectiveCamera.look_at((0, 0, EYE), (0, 0, 0), up = y) with fov = 2 atan(half / EYE) gives pinhole()'s rays and
    film_position()'s positions within 1e-6 at unit scale: those are float32 torch chains of about six roundings of
    quantities of order one, and film_position multiplies its last such quantity, d.x s / half + 1 in [0, 2], by film / 2
    to get pixels -- so the positions are compared in that unit, pixels over film / 2 (a deviation from a flat 1e-6 pixels,
    which is less than the chain's one ulp at 16 pixels, 1.9e-6).  The sensor's origin is on the near plane: it is carried back along the
    ray by near / d_c.z, to the pinhole, before it is compared."""
    import inverse_pose as ip
    film, spp, half, near = 16, 3, 1.3, 1e-2
    want, wpos = ip.pinhole(film, spp, "cuda", half)
    cam = hf.PerspectiveCamera.look_at((0.0, 0.0, ip.EYE), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0),
                                       float(np.degrees(2 * np.arctan(half / ip.EYE))), film=(film, film), near_clip=near)
    ray, pos, _ = cam.sample_rays(spp, seed=0)
    assert _same(pos, wpos)
    assert float((ray.d - want.d).abs().max()) <= 1e-6
    eye = ray.o.double() - ray.d.double() * (near / -ray.d[2].double())
    assert float((eye - want.o.double()).abs().max()) <= 1e-6
    uv, valid, _ = cam.sample_direction(ray(torch.full_like(ray.maxt, 2.0)))
    assert bool(valid.all())
    gap = float((uv - ip.film_position(want.d, film, half)).abs().max()) / (0.5 * film)
    print("film position: worst difference over film / 2", gap)
    assert gap <= 1e-6


# ---- (2) indexing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_", TYPES)
def test_start_count_pixels_and_an_empty_wavefront(hf, type_):
    s = R.scene(type_, R.CROP)
    cam, spp = _camera(hf, s), 3
    full, fpos, findex = cam.sample_rays(spp, seed=R.SEED)
    part, ppos, pindex = cam.sample_rays(spp, seed=R.SEED, start=5, count=37)
    for a, b in ((part.o, full.o[:, 5:42]), (part.d, full.d[:, 5:42]), (part.maxt, full.maxt[5:42]), (ppos, fpos[:, 5:42]),
                 (pindex, findex[5:42])):
        assert _same(a, b.contiguous())
    pix = torch.randperm(s.crop[2] * s.crop[3], generator=torch.Generator().manual_seed(1))[:11]
    sub, spos, sindex = cam.sample_rays(spp, seed=R.SEED, pixels=pix)
    take = sindex.long()
    assert np.array_equal(_np(take), (_np(pix)[:, None] * spp + np.arange(spp)).reshape(-1))
    for a, b in ((sub.o, full.o[:, take]), (sub.d, full.d[:, take]), (sub.maxt, full.maxt[take]), (spos, fpos[:, take])):
        assert _same(a, b.contiguous())
    none, npos, nindex = cam.sample_rays(spp, count=0)
    assert len(none) == 0 and npos.shape == (2, 0) and nindex.numel() == 0


def _raw(hf, s, n, spp, start=1, ray_id=None):
    """the three ray entries through the C ABI on guarded rows; returns a function of the optional pointers to leave out"""
    lib, check = hf._capi.lib(), hf._capi.check
    st = _camera(hf, s)._struct(torch.tensor(s.to_world), s.fov)
    stream = torch.cuda.current_stream().cuda_stream
    dtw, dfov = R.directions()
    go, gd = R.cotangents(n)
    dev = dict(dtw=_cu(dtw), dfov=_cu(np.array([dfov], np.float32)), go=_cu(go), gd=_cu(gd))
    ws = torch.empty(lib.hf_sensor_workspace_floats(), dtype=torch.float32, device="cuda")
    G = 7

    def run(null=()):
        ptr = lambda k: None if k in null else dev[k].data_ptr()
        rid = None if ray_id is None or "ray_id" in null else ray_id.data_ptr()
        o, op = guarded(n, G, 3); d, dp = guarded(n, G, 3); m, mp = guarded(n, G); pos, pp = guarded(n, G, 2)
        check(lib.hf_sensor_rays(st, n, start, spp, R.SEED, rid, op, dp, mp[0], None if "out_pos" in null else pp, stream))
        do, dop = guarded(n, G, 3); dd, ddp = guarded(n, G, 3)
        check(lib.hf_sensor_rays_tangent(st, n, start, spp, R.SEED, rid, ptr("dtw"), ptr("dfov"), dop, ddp, stream))
        g12, gf = torch.full((12,), 0.5, device="cuda"), torch.full((1,), 0.25, device="cuda")
        check(lib.hf_sensor_rays_adjoint(st, n, start, spp, R.SEED, rid, None if "go" in null else rows(dev["go"]),
                                         None if "gd" in null else rows(dev["gd"]), None if "g12" in null else g12.data_ptr(),
                                         None if "gf" in null else gf.data_ptr(), ws.data_ptr(), stream))
        torch.cuda.synchronize()
        for buf in (o, d, m, do, dd) + (() if "out_pos" in null else (pos,)):
            assert intact(buf, n, G), null
        if "out_pos" in null:
            assert bool((pos == -12345.0).all())
        cut = lambda b: b[:, G:G + n].clone()
        return dict(o=cut(o), d=cut(d), maxt=cut(m), pos=cut(pos), do=cut(do), dd=cut(dd), g12=g12, gf=gf)
    return run, dev


@pytest.mark.parametrize("type_", TYPES)
def test_guard_bands_and_optional_pointers(hf, type_):
    """n = 151 spp samples from an odd start on rows with guard bands; every optional pointer NULL in turn"""
    spp = 3
    n = 151 * spp
    s = R.sensor(type_, R.ORTHO_POSE if type_ == R.ORTHOGRAPHIC else R.POSE, None if type_ == R.ORTHOGRAPHIC else R.FOV, (31, 17))
    run, dev = _raw(hf, s, n, spp)
    base = run()
    persp = type_ == R.PERSPECTIVE
    assert float(base["gf"]) != 0.25 if persp else float(base["gf"]) == 0.25       # the orthographic type leaves grad_fov alone
    assert not _same(base["g12"], torch.full((12,), 0.5, device="cuda"))
    again = run()
    for k in base:
        assert _same(base[k], again[k]), f"{k} is not repeatable"
    ids = torch.arange(1, 1 + n, dtype=torch.int32, device="cuda")
    with_ids = _raw(hf, s, n, spp, start=77, ray_id=ids)[0]()                       # ray_id overrides start
    for k in base:
        assert _same(base[k], with_ids[k]), k
    got = run(null=("out_pos",))
    for k in ("o", "d", "maxt", "do", "dd", "g12", "gf"):
        assert _same(base[k], got[k]), k
    zero = {"dtw": torch.zeros(12, device="cuda"), "dfov": torch.zeros(1, device="cuda"), "go": torch.zeros((3, n), device="cuda"),
            "gd": torch.zeros((3, n), device="cuda")}
    for k in zero:                                                                  # NULL = zero
        got = run(null=(k,))
        keep, dev[k] = dev[k], zero[k]
        want = run()
        dev[k] = keep
        for j in want:
            assert _same(want[j], got[j]), (k, j)
    for k, other in (("g12", "gf"), ("gf", "g12")):                                 # NULL = not wanted
        got = run(null=(k,))
        assert _same(base[other], got[other]) and float(got[k].flatten()[0]) == (0.5 if k == "g12" else 0.25)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(value)
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("type_", TYPES)
def test_both_store_variants_write_the_same_bytes(hf, type_, with_ids):
    """HF_SENSOR_STORE = dword / wide on n = 151 * 3 samples from an odd start.  The guarded rows start 7 elements into
    rows of n + 14 = 467 elements, so consecutive rows have every alignment modulo 16 bytes: the wide kernel takes its
    16-byte store on the rows that share out_o[0]'s alignment and its dword path on the others, on the head and on the
    tail; then rows that are all aligned, rows offset by 4 bytes from a 16-byte boundary, and out_pos NULL."""
    spp = 3
    n = 151 * spp
    s = R.sensor(type_, R.ORTHO_POSE if type_ == R.ORTHOGRAPHIC else R.POSE, None if type_ == R.ORTHOGRAPHIC else R.FOV, (31, 17))
    ids = torch.randperm(31 * 17 * spp, generator=torch.Generator().manual_seed(3))[:n].to(torch.int32).cuda() if with_ids else None
    got = {}
    for store in ("dword", "wide"):
        with _env("HF_SENSOR_STORE", store):
            run, _ = _raw(hf, s, n, spp, start=5, ray_id=ids)
            got[store] = [run(), run(null=("out_pos",))]
            lib, check = hf._capi.lib(), hf._capi.check
            st = _camera(hf, s)._struct(torch.tensor(s.to_world), s.fov)
            for off in (0, 1):                                         # rows on / 4 bytes past a 16-byte boundary
                L = 464                                                # rows of L elements, each starting `off` elements in
                buf = torch.full((9, L), -7.0, device="cuda")
                assert buf.data_ptr() % 16 == 0 and L % 4 == 0 and L >= n + off
                r9 = (hf._capi._fp * 9)(*[buf.data_ptr() + 4 * (k * L + off) for k in range(9)])
                check(lib.hf_sensor_rays(st, n, 5, spp, R.SEED, None if ids is None else ids.data_ptr(),
                                         (hf._capi._fp * 3)(*r9[0:3]), (hf._capi._fp * 3)(*r9[3:6]), r9[6], (hf._capi._fp * 2)(*r9[7:9]),
                                         torch.cuda.current_stream().cuda_stream))
                torch.cuda.synchronize()
                assert bool((buf[:, :off] == -7.0).all()) and bool((buf[:, off + n:] == -7.0).all())
                got[store].append({"rows": buf[:, off:off + n].clone()})
    for a, b in zip(got["dword"], got["wide"]):
        for k in a:
            assert _same(a[k], b[k]), k
    assert _same(got["dword"][2]["rows"], got["dword"][3]["rows"]) and _same(got["dword"][2]["rows"][:3], got["dword"][0]["o"])


@pytest.mark.parametrize("type_", TYPES)
def test_the_reducer_adds_more_rows_than_it_has_threads(hf, type_):
    """n = 256 * 300 + 37 samples: the adjoint launches 301 blocks, so hf_sensor_sum_kernel's 256 threads go round their
    row loop twice; the 13 reduced numbers against the float64 restatement and against the launch forced to 3 blocks"""
    n = 256 * 300 + 37
    s = R.sensor(type_, R.ORTHO_POSE if type_ == R.ORTHOGRAPHIC else R.POSE, None if type_ == R.ORTHOGRAPHIC else R.FOV, (320, 241))
    go, gd = R.cotangents(n)
    pos = R.film_positions(s, np.arange(n, dtype=np.uint64), 1, R.SEED)
    g12, gf = R.rays_adjoint(s, pos, go, gd)
    want = np.append(g12, gf)
    got = {}
    for blocks in (None, 3):
        with _env("HF_FORCE_GRID", blocks):
            assert hf._capi.lib().hf_grid_blocks(n, 2) == (301 if blocks is None else 3)
            tw = torch.tensor(s.to_world, requires_grad=True)
            fov = torch.tensor(s.fov, dtype=torch.float64, requires_grad=True) if type_ == R.PERSPECTIVE else None
            ray, _, _ = _camera(hf, s, tw, fov).sample_rays(1, seed=R.SEED, count=n)
            ((ray.o * _cu(go)).sum() + (ray.d * _cu(gd)).sum()).backward()
            got[blocks] = np.append(_np(tw.grad).reshape(-1), float(fov.grad) if fov is not None else 0.0)
    print("reduced gradients: error", R.err_l2(got[None], want), "forced grid", R.err_l2(got[3], want), "allowed", TOL["adjoint"])
    assert R.err_l2(got[None], want) <= TOL["adjoint"] and R.err_l2(got[3], want) <= TOL["adjoint"]


def test_captured_graph_replays_to_the_same_bits(hf):
    s = R.scene(R.PERSPECTIVE, R.CROP, near=R.PROJECT_CLIP[0], far=R.PROJECT_CLIP[1])
    lib, check = hf._capi.lib(), hf._capi.check
    st = _camera(hf, s)._struct(torch.tensor(s.to_world), s.fov)
    spp = 4
    n = s.crop[2] * s.crop[3] * spp
    dtw, dfov = R.directions()
    go, gd = R.cotangents(n)
    dtw, dfov, go, gd = _cu(dtw), _cu(np.array([dfov], np.float32)), _cu(go), _cu(gd)
    o, d, do, dd, gp, pts = (torch.zeros((3, n), device="cuda") for _ in range(6))
    maxt, w = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pos, uv = torch.zeros((2, n), device="cuda"), torch.zeros((2, n), device="cuda")
    valid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    g = torch.zeros(26, device="cuda")
    ws = torch.empty(lib.hf_sensor_workspace_floats(), dtype=torch.float32, device="cuda")
    outs = (o, d, maxt, pos, do, dd, uv, valid, w, gp, g)

    def launch():
        stream = torch.cuda.current_stream().cuda_stream
        g.zero_()
        check(lib.hf_sensor_rays(st, n, 0, spp, R.SEED, None, rows(o), rows(d), maxt.data_ptr(), rows(pos), stream))
        check(lib.hf_sensor_rays_tangent(st, n, 0, spp, R.SEED, None, dtw.data_ptr(), dfov.data_ptr(), rows(do), rows(dd), stream))
        check(lib.hf_sensor_rays_adjoint(st, n, 0, spp, R.SEED, None, rows(go), rows(gd), g.data_ptr(), g.data_ptr() + 48,
                                         ws.data_ptr(), stream))
        torch.add(o, d, out=pts)                                     # points of the rays, beyond the near plane
        check(lib.hf_sensor_project(st, n, rows(pts), None, rows(uv), valid.data_ptr(), w.data_ptr(), stream))
        check(lib.hf_sensor_project_adjoint(st, n, rows(pts), None, rows(pos), maxt.data_ptr(), rows(gp), g.data_ptr() + 52,
                                            g.data_ptr() + 100, ws.data_ptr(), stream))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [v.clone() for v in outs]
    assert float(g.abs().sum()) > 0 and bool(valid.all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for v in outs:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert _same(a, b)


@contextlib.contextmanager
def _grid(blocks):
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


@pytest.mark.parametrize("store", ["dword", "wide"])
@pytest.mark.parametrize("type_", TYPES)
def test_forced_grid_goes_round_the_loops(hf, type_, store):
    """n = 256 C 3 + 256 + 37 samples with C blocks forced (tests/test_gpu_grid_stride.py): every wave of the rays, tangent
    and adjoint kernels and of the projection, its tangent and its adjoint loops at least three times and the waves of a block leave the loop at different
    iterations.  Per-lane outputs equal the unforced launch bit for bit; the reduced gradients, whose order of summation
    follows the grid, within the adjoint's tolerance"""
    C = 3
    n = 4 * (256 * C * 3 + 256 + 37)      # (the wide rays kernel takes four samples per lane: its groups are a quarter of n)
    lib = hf._capi.lib()
    s = R.sensor(type_, R.ORTHO_POSE if type_ == R.ORTHOGRAPHIC else R.POSE, None if type_ == R.ORTHOGRAPHIC else R.FOV, (64, 41),
                 near=R.PROJECT_CLIP[0], far=R.PROJECT_CLIP[1])
    cam = _camera(hf, s, torch.tensor(s.to_world, requires_grad=True), None if s.fov is None else torch.tensor(s.fov, requires_grad=True))
    go, gd = (_cu(v) for v in R.cotangents(n))

    def run():
        cam.to_world.grad = None
        ray, pos, _ = cam.sample_rays(4, seed=R.SEED, start=3, count=n)
        if cam.fov is not None:
            cam.fov.grad = None
        ((ray.o * go).sum() + (ray.d * gd).sum()).backward()
        out = [ray.o.detach(), ray.d.detach(), ray.maxt, pos,
               torch.cat([cam.to_world.grad.reshape(-1), cam.fov.grad.reshape(1) if cam.fov is not None else torch.zeros(1, dtype=torch.float64)])]
        with fwAD.dual_level():
            dual = _camera(hf, s, fwAD.make_dual(torch.tensor(s.to_world), torch.tensor(R.directions()[0].reshape(3, 4).astype(np.float64))))
            r2, _, _ = dual.sample_rays(4, seed=R.SEED, start=3, count=n)
            out += [fwAD.unpack_dual(r2.o).tangent, fwAD.unpack_dual(r2.d).tangent]
        if type_ == R.PERSPECTIVE:
            p = ray(torch.full_like(ray.maxt, 0.7)).detach().requires_grad_(True)
            cam.to_world.grad, cam.fov.grad = None, None
            uv, valid, w = cam.sample_direction(p)
            ((uv * go[:2]).sum() + (w * gd[0]).sum()).backward()
            out += [uv.detach(), valid, w.detach(), p.grad.clone(), cam.to_world.grad.clone(), cam.fov.grad.clone()]
            with fwAD.dual_level():
                dual = _camera(hf, s, fwAD.make_dual(torch.tensor(s.to_world), torch.tensor(R.directions()[0].reshape(3, 4).astype(np.float64))),
                               fwAD.make_dual(torch.tensor(s.fov, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)))
                duv, _, dw = dual.sample_direction(fwAD.make_dual(p.detach(), gd))
                out += [fwAD.unpack_dual(duv).tangent, fwAD.unpack_dual(dw).tangent]
        return out
    with _env("HF_SENSOR_STORE", store):
        with _grid(None):
            for fam in (1, 2):
                assert lib.hf_grid_blocks(n, fam) == -(-n // 256) and lib.hf_grid_blocks(n // 4, fam) == -(-(n // 4) // 256)
            plain = run()
            torch.cuda.synchronize()
        with _grid(C):
            for fam in (1, 2):
                assert lib.hf_grid_blocks(n, fam) == C and lib.hf_grid_blocks(n // 4, fam) == C and C < (n // 4) / (256 * 3)
            forced = run()
            torch.cuda.synchronize()
    reduced = (4, 11, 12)      # to_world's and fov's gradients of the rays, to_world's and fov's of the way back
    for k, (a, b) in enumerate(zip(plain, forced)):
        if k in reduced:
            assert float(b.abs().max()) > 0 and R.err_l2(_np(b), _np(a)) <= TOL["adjoint"], k
        else:
            assert _same(a, b), f"output {k}: the forced launch differs from the unforced one"


# ---- (3) the way back -------------------------------------------------------------------------------------------------
_PROJECT = {}


def _project_case(crop):
    if crop not in _PROJECT:
        s = R.scene(R.PERSPECTIVE, crop, near=R.PROJECT_CLIP[0], far=R.PROJECT_CLIP[1])
        _PROJECT[crop] = (s,) + R.project_case(s)
    return _PROJECT[crop]


@pytest.mark.parametrize("crop", CROPS)
def test_projection_and_its_derivatives_equal_the_restatement(hf, crop):
    """the points are built so that no mask is decided by rounding (sensor_ref.project_points): valid is exact and no
    lane is left out"""
    s, p, active, ref = _project_case(crop)
    assert ref.inside.any() and (active & ~ref.inside).any() and ref.valid.any() and (ref.inside & ~ref.valid).any() and (~active).any()
    tw = torch.tensor(s.to_world, requires_grad=True)
    fov = torch.tensor(s.fov, dtype=torch.float64, requires_grad=True)
    cam = _camera(hf, s, tw, fov)
    pp = _cu(p).requires_grad_(True)
    uv, valid, w = cam.sample_direction(pp, active=_cu(active))
    assert np.array_equal(_np(valid), ref.valid)
    assert not _np(uv)[:, ~ref.inside].any() and not _np(w)[~ref.valid].any()
    ((uv * _cu(ref.guv)).sum() + (w * _cu(ref.gw)).sum()).backward()
    dtw, dfov = R.directions()
    with fwAD.dual_level():
        dual = _camera(hf, s, fwAD.make_dual(torch.tensor(s.to_world), torch.tensor(dtw.reshape(3, 4).astype(np.float64))),
                       fwAD.make_dual(torch.tensor(s.fov, dtype=torch.float64), torch.tensor(float(dfov), dtype=torch.float64)))
        duv, _, dw = dual.sample_direction(fwAD.make_dual(_cu(p), _cu(ref.dp)), active=_cu(active))
        duv, dw = fwAD.unpack_dual(duv).tangent, fwAD.unpack_dual(dw).tangent
    assert not _np(duv)[:, ~ref.inside].any() and not _np(dw)[~ref.valid].any() and not _np(pp.grad)[:, ~ref.inside].any()
    import types
    got = types.SimpleNamespace(uv=_np(uv).astype(np.float64), weight=np.where(ref.valid, _np(w).astype(np.float64), ref.weight),
                                duv=_np(duv), dweight=np.where(ref.valid, _np(dw).astype(np.float64), ref.dweight), grad_p=_np(pp.grad),
                                grad13=np.append(_np(tw.grad).reshape(-1), float(fov.grad)))
    err = R.project_errors(s, p, active, got, ref)
    print("worst errors", err, "allowed", {k: TOL[k] for k in err})
    assert all(err[k] <= TOL[k] for k in err), {k: (err[k], TOL[k]) for k in err if err[k] > TOL[k]}
    # transposition on the device: <J u, v> = <u, J^T v> over (p, to_world, fov) -> (uv, weight)
    gap = transposition_gap([(_np(duv), ref.guv), (_np(dw), ref.gw)],
                            [(ref.dp, _np(pp.grad)), (dtw, _np(tw.grad).reshape(-1)), (dfov, float(fov.grad))])
    m = ref.inside
    bound = (TOL["project_duv"] * max(1, np.abs(ref.duv[:, m]).max()) * np.abs(ref.guv[:, m]).sum()
             + TOL["project_dweight"] * np.abs(ref.weight * ref.gw)[ref.valid].sum()
             + TOL["project_grad_p"] * np.linalg.norm(ref.grad_p) * np.linalg.norm(ref.dp)
             + TOL["project_adjoint"] * np.linalg.norm(ref.grad13) * np.linalg.norm(np.append(dtw, dfov)))
    print("transposition gap", gap, "bound", bound)
    assert gap <= bound


@pytest.mark.parametrize("crop", CROPS)
def test_projecting_a_point_of_a_ray_returns_its_film_position(hf, crop):
    s = R.scene(R.PERSPECTIVE, crop, near=R.PROJECT_CLIP[0], far=R.PROJECT_CLIP[1])
    cam = _camera(hf, s)
    ray, pos, _ = cam.sample_rays(4, seed=R.SEED)
    for t in (0.5, 3.0):
        uv, valid, w = cam.sample_direction(ray(torch.full_like(ray.maxt, t)))
        gap = float((uv - pos).abs().max())
        print("t", t, "worst |uv - pos|", gap, "allowed", TOL["project_uv"])
        assert gap <= TOL["project_uv"]
        m = _np(valid)
        assert m.mean() > 0.9 and (_np(w)[m] > 0).all()      # (a sample on the window's edge may round out of it)


# ---- (4) the derivatives of the rays -------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", R.SPPS)
@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("type_", TYPES)
def test_ray_derivatives_equal_the_restatement_and_transpose(hf, type_, crop, spp):
    s = R.scene(type_, crop)
    n = s.crop[2] * s.crop[3] * spp
    dtw, dfov = R.directions()
    go, gd = R.cotangents(n)
    persp = type_ == R.PERSPECTIVE
    tw = torch.tensor(s.to_world, requires_grad=True)
    fov = torch.tensor(s.fov, dtype=torch.float64, requires_grad=True) if persp else None
    ray, _, _ = _camera(hf, s, tw, fov).sample_rays(spp, seed=R.SEED)
    ((ray.o * _cu(go)).sum() + (ray.d * _cu(gd)).sum()).backward()
    gf = float(fov.grad) if persp else 0.0
    with fwAD.dual_level():
        dual = _camera(hf, s, fwAD.make_dual(torch.tensor(s.to_world), torch.tensor(dtw.reshape(3, 4).astype(np.float64))),
                       fwAD.make_dual(torch.tensor(s.fov, dtype=torch.float64), torch.tensor(float(dfov), dtype=torch.float64)) if persp else None)
        r2, _, _ = dual.sample_rays(spp, seed=R.SEED)
        do, dd = _np(fwAD.unpack_dual(r2.o).tangent), _np(fwAD.unpack_dual(r2.d).tangent)
        assert _same(fwAD.unpack_dual(r2.o).primal, ray.o.detach())
    err = R.ray_derivative_errors(s, spp, (do, dd), (_np(tw.grad).reshape(-1), gf))
    print("worst errors", err, "allowed", {k: TOL[k] for k in err})
    assert all(err[k] <= TOL[k] for k in err), err
    u13, g13 = np.append(dtw, dfov if persp else 0.0), np.append(_np(tw.grad).reshape(-1), gf)
    gap = transposition_gap([(do, go), (dd, gd)], [(u13, g13)])
    bound = (TOL["tangent_do"] * max(1, np.abs(do).max()) * np.abs(go).sum() + TOL["tangent_dd"] * max(1, np.abs(dd).max()) * np.abs(gd).sum()
             + TOL["adjoint"] * np.linalg.norm(g13) * np.linalg.norm(u13))
    print("transposition gap", gap, "bound", bound)
    assert gap <= bound


def _smooth_field(hf, n=64):
    """a tilted plane with a gentle bump: slopes of about 0.18, curvature 0.05 / 0.4^2 = 0.31"""
    u = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device="cuda")
    X, Y = u[None, :], u[:, None]
    return (0.3 + 0.15 * X - 0.1 * Y + 0.05 * torch.exp(-(X ** 2 + Y ** 2) / (2 * 0.4 ** 2))).to(torch.float32)


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def _rotation(w):
    """Rodrigues: exp([w]x)"""
    th = np.linalg.norm(w)
    K = _skew(np.asarray(w, np.float64) / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def test_backward_and_jvp_through_the_intersection_equal_central_differences(hf):
    """loss = sum(si.p[2]) of sample_rays -> ray_intersect on an interior view of a smooth field (every ray hits), along a
    direction that keeps to_world a rigid motion -- to_world(e) = [A exp(e [w]x) | c + e dc], fov + e dfov -- so that the
    perspective type's scale rule holds at every step.  Central differences with e = 3e-4 carry
      * the rounding of the 2 x 273 float32 heights they subtract, half an ulp of 0.5 each: at most 546 * 1.5e-8 / 6e-4 =
        0.014, absolute;
      * the kinks of the triangulated surface: a hit moves by e |dp| with |dp| about 1.5, across a kink the slope changes
        by cell * curvature, and the share of hits that cross one is e |dp| / cell: e |dp| curvature / (2 slope) =
        3e-4 * 1.5 * 0.31 / 0.36 = 4e-4 of the derivative (their own truncation, e^2, is far below).
    Allowed: 1e-3 of the derivative plus 0.015.  backward and jvp are the same float32 kernels' transposes of each other:
    1e-5 of the derivative between them."""
    shape = hf.Heightfield(heightfield=_smooth_field(hf), max_height=0.5)
    A0 = R.look_at((0.3, -0.2, 2.5), (0.05, 0.0, 0.25), (0.0, 1.0, 0.0))[:3]
    w, dc, dfov, fov0, e = np.array([0.5, -0.2, 0.3]), np.array([1.0, -0.6, 0.2]), 0.8, 20.0, 3e-4

    def pose(k):
        m = A0.copy()
        if k:
            m[:, :3] = A0[:, :3] @ _rotation(w * k * e)
        m[:, 3] = A0[:, 3] + k * e * dc
        return m

    def loss(tw, fov):
        cam = hf.PerspectiveCamera(tw, fov, film=R.FILM)
        ray, _, _ = cam.sample_rays(3, seed=R.SEED)
        si = shape.ray_intersect(ray, hf.RayFlags.All)
        assert len(ray) == 273 and bool(si.is_valid().all())
        return si.p[2].double().sum()
    f = {k: float(loss(torch.tensor(pose(k)), fov0 + k * e * dfov)) for k in (-1, 1)}
    fd = (f[1] - f[-1]) / (2 * e)
    dtw = np.concatenate([A0[:, :3] @ _skew(w), dc[:, None]], axis=1)
    tw = torch.tensor(A0, requires_grad=True)
    fov = torch.tensor(fov0, dtype=torch.float64, requires_grad=True)
    loss(tw, fov).backward()
    back = float((tw.grad * torch.tensor(dtw)).sum() + fov.grad * dfov)
    assert abs(float(fov.grad)) > 0 and float(tw.grad.abs().min()) > 0
    with fwAD.dual_level():
        out = loss(fwAD.make_dual(torch.tensor(A0), torch.tensor(dtw)),
                   fwAD.make_dual(torch.tensor(fov0, dtype=torch.float64), torch.tensor(dfov, dtype=torch.float64)))
        fwd = float(fwAD.unpack_dual(out).tangent)
    print("central differences", fd, "backward", back, "jvp", fwd)
    assert abs(fd) > 20.0
    assert abs(back - fd) <= 1e-3 * abs(fd) + 0.015 and abs(fwd - fd) <= 1e-3 * abs(fd) + 0.015
    assert abs(back - fwd) <= 1e-5 * abs(fd)


# ---- (5) the example ----------------------------------------------------------------------------------------------------
def test_inverse_camera_example_descends(hf):
    import inverse_camera
    target, start, final, losses = inverse_camera.recover(steps=31, film=48, spp=4)
    print("start", start, "final", final, "loss", losses[0], "->", losses[30])
    assert np.isfinite(losses[-1]) and losses[30] < losses[0], (losses[0], losses[30])
    for t, a, b in zip(target, start, final):
        assert abs(b - t) < abs(a - t), (target, start, final)

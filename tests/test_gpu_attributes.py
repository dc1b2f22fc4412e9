"""Shape attributes (hf_eval_attribute and its adjoint / tangent) on the GPU, against the float64 restatement
tests/attr_ref.py:
  * the known answers of the reference's mesh_attribute test01 through the library, and its error messages;
  * forward parity on noise fields with traced rays, vertex and face attributes of size 1 and 3; misses and inactive
    lanes are exactly 0;
  * reverse mode (dL/dattr, dL/dp, dL/dheight) against float64 autograd; the whole chain ray_intersect + eval_attribute +
    backward against float64 central differences, in the default and FollowShape modes;
  * forward mode: the transpose of the adjoint, bitwise repeatable, and the autograd Function under forward_ad;
  * a captured forward + adjoint replays to eager; existing outputs do not move when attributes are present;
  * joint recovery of heights and a reflectance map from four-light renders.
"""
import math

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import attr_ref as R
import common
import smooth_ref as S
import test_attributes_abi as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LIGHTS = torch.tensor([[0.5, 0.2, 0.84], [-0.5, 0.3, 0.81], [0.1, -0.6, 0.79], [0.0, 0.0, 1.0]])  # examples/inverse_heights.py


def _si(hf, p, prim, t):
    si = hf.SurfaceInteraction3f()
    si.p, si.prim_index, si.t = p, prim, t
    return si


# ---- 1. known answers ---------------------------------------------------------------------------------------------

def test_known_answers_of_the_reference_rectangle(hf):
    shape = hf.Heightfield(heightfield=torch.zeros((2, 2), device=DEV), max_height=1.0)
    for name, (_, data) in K.RECT.items():
        d = torch.tensor(data)
        shape.add_attribute(name, d.shape[1], d.reshape(-1))
    uv, p, prim = K.rectangle_hits()
    n = len(uv)
    si = _si(hf, p.T.float().contiguous().to(DEV), prim.int().to(DEV), torch.zeros(n, device=DEV))
    for name in K.RECT:
        ref = K.expected(name, uv, prim).T.float()
        size = ref.shape[0]
        assert shape.has_attribute(name)
        v = shape.eval_attribute(name, si).cpu()
        assert torch.allclose(v, ref.expand(3, -1), atol=1e-6), (name, v, ref)
        if size == 1:
            assert torch.allclose(shape.eval_attribute_1(name, si).cpu(), ref[0], atol=1e-6), name
            with pytest.raises(RuntimeError, match=f'eval_attribute_3\\(\\): Attribute "{name}" requested but had size 1'):
                shape.eval_attribute_3(name, si)
        else:
            assert torch.allclose(shape.eval_attribute_3(name, si).cpu(), ref, atol=1e-6), name
            with pytest.raises(RuntimeError, match="requested but had size 3"):
                shape.eval_attribute_1(name, si)
    assert not shape.has_attribute("vertex_colorr")
    with pytest.raises(RuntimeError, match="Invalid attribute requested vertex_colorr"):
        shape.eval_attribute("vertex_colorr", si)
    with pytest.raises(RuntimeError, match='attribute name must start with either "vertex_" of "face_"'):
        shape.add_attribute("color", 1, [0.0] * 4)
    with pytest.raises(RuntimeError, match="attribute vertex_mono already exists"):
        shape.add_attribute("vertex_mono", 1, [0.0] * 4)
    # an attribute of another size (the reference's "had size %u" of eval_attribute) and the ABI's size check
    shape.add_attribute("vertex_two", 2, [0.0] * 8)
    with pytest.raises(RuntimeError, match='eval_attribute\\(\\): Attribute "vertex_two" requested but had size 2'):
        shape.eval_attribute("vertex_two", si)


def test_constructor_properties_traverse_and_resize(hf):
    H, W = 5, 4
    vc = torch.rand((H, W, 3))
    fm = torch.rand((2 * (H - 1) * (W - 1), 1))
    shape = hf.Heightfield(heightfield=torch.rand((H, W), device=DEV), vertex_color=vc, face_mono=fm)
    assert torch.equal(shape.attributes["vertex_color"].cpu(), vc.reshape(-1))
    assert shape._attr_meta["face_mono"] == (1, 1)

    class CB:
        def __init__(self):
            self.p = {}

        def put_parameter(self, k, v, flags):
            self.p[k] = (v, flags)
    cb = CB()
    shape.traverse(cb)
    assert cb.p["vertex_color"][1] == hf.ParamFlags.Differentiable and cb.p["face_mono"][1] == hf.ParamFlags.Differentiable
    shape.attributes["vertex_color"] = torch.ones(7, device=DEV)     # the wrong size: reset to zeros (mesh.cpp:103-110)
    shape.parameters_changed(["vertex_color"])
    assert torch.equal(shape.attributes["vertex_color"], torch.zeros(H * W * 3, device=DEV))


def test_a_buffer_of_the_wrong_size_never_reaches_the_kernels(hf):
    """an attribute tensor replaced behind parameters_changed's back is refused before any launch, and every
    parameters_changed resets it, whatever its keys (mesh.cpp:103-110)"""
    shape = hf.Heightfield(heightfield=torch.rand((5, 4), device=DEV), vertex_color=torch.rand((5, 4, 3)))
    si = _si(hf, torch.zeros((3, 2), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV))
    shape.attributes["vertex_color"] = torch.ones(3 * 4, device=DEV)   # one row of vertices only
    with pytest.raises(RuntimeError, match="vertex_color: expected a contiguous float32 buffer of 20 x 3 values"):
        shape.eval_attribute_3("vertex_color", si)
    shape.parameters_changed(["heightfield"])
    assert torch.equal(shape.attributes["vertex_color"], torch.zeros(60, device=DEV))
    assert torch.equal(shape.eval_attribute_3("vertex_color", si), torch.zeros((3, 2), device=DEV))


# ---- 2. forward parity --------------------------------------------------------------------------------------------

FIELDS = [(33, 21, "identity"), (33, 21, "affine"), (257, 257, "affine")]


def _setup(hf, W, H, tw_kind, n=8192, seed=0):
    rng = np.random.default_rng(seed + W + 7 * H)
    h = rng.uniform(0.1, 0.9, (H, W)).astype(np.float32)            # noise field
    # max_height shrinks with the cell size, so that the cells' slopes (and the conditioning of the least-squares
    # solve of barycentric_coordinates, which the reference shares in float32) do not grow with the resolution
    s = 0.3 * 32.0 / (W - 1)
    T = np.eye(4, dtype=np.float32)[:3] if tw_kind == "identity" else common.affine(3)
    shape = hf.Heightfield(heightfield=torch.from_numpy(h).to(DEV), max_height=s, to_world=torch.from_numpy(T))
    r = common.to_world_rays(common.random_rays(n, rng), T)
    ray = hf.Ray3f(torch.from_numpy(r[0:3]).to(DEV), torch.from_numpy(r[3:6]).to(DEV), torch.from_numpy(r[6]).to(DEV))
    active = torch.from_numpy(rng.uniform(size=n) < 0.85).to(DEV)
    for kind in ("vertex", "face"):
        count = W * H if kind == "vertex" else 2 * (W - 1) * (H - 1)
        for size in (1, 3):
            shape.add_attribute(f"{kind}_a{size}", size, torch.from_numpy(rng.uniform(0.5, 1.5, count * size)))
    return shape, h, s, T.astype(np.float64), ray, active


def _ref(shape, name, h, s, T, si, hit, **kw):
    kind, size = name.split("_")[0], shape._attr_meta[name][1]
    attr = shape.attributes[name].double().reshape(-1, size)
    return R.value(kind, attr, torch.from_numpy(h).double().to(DEV), s, T, si.prim_index.long(), si.p.T.double(),
                   hit, **kw)


@pytest.mark.parametrize("W,H,tw", FIELDS)
def test_forward_parity(hf, W, H, tw):
    shape, h, s, T, ray, active = _setup(hf, W, H, tw)
    si = shape.ray_intersect(ray)
    hit = si.is_valid() & active
    assert int(hit.sum()) > 1000 and int((~si.is_valid()).sum()) > 100
    for name in ("vertex_a1", "vertex_a3", "face_a1", "face_a3"):
        size = shape._attr_meta[name][1]
        got = (shape.eval_attribute_1(name, si, active)[None] if size == 1 else shape.eval_attribute_3(name, si, active))
        ref = _ref(shape, name, h, s, T, si, hit, device_rounding=True).T
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        assert err <= 1e-5, (name, err)
        assert torch.all(got[:, ~hit] == 0), name
        if name.startswith("face"):
            assert torch.equal(got[:, hit].double(), ref[:, hit]), name   # a gather: exact


# ---- 3. reverse mode ----------------------------------------------------------------------------------------------

def _rel(a, b):
    return float(torch.linalg.norm((a.double() - b.double()).reshape(-1)) / torch.linalg.norm(b.double().reshape(-1)))


@pytest.mark.parametrize("W,H,tw", FIELDS)
def test_adjoint_against_float64_autograd(hf, W, H, tw):
    shape, h, s, T, ray, active = _setup(hf, W, H, tw, seed=1)
    si = shape.ray_intersect(ray)
    hit = si.is_valid() & active
    n = len(ray)
    for name in ("vertex_a1", "vertex_a3", "face_a1", "face_a3"):
        size = shape._attr_meta[name][1]
        g = torch.randn((size, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(size))
        ga, gp, gh = shape.eval_attribute_adjoint(name, si, g, active)
        attr = shape.attributes[name].double().reshape(-1, size).requires_grad_(True)
        h64 = torch.from_numpy(h).double().to(DEV).requires_grad_(True)
        p64 = si.p.T.double().contiguous().requires_grad_(True)
        kind = name.split("_")[0]
        val = R.value(kind, attr, h64, s, T, si.prim_index.long(), p64, hit)
        (val * g.T.double()).sum().backward()
        assert _rel(ga, attr.grad.reshape(-1)) <= 1e-5, name
        if kind == "vertex":
            assert _rel(gp.T, p64.grad) <= 1e-5, name
            # dL/dheight goes through M^-1 of the solve a second time (the vertices move, p does not): on the 257^2
            # field its float32 per-lane rounding measured 1.02e-5 relative L2, hence 2e-5 here
            assert _rel(gh, h64.grad) <= 2e-5, name
            assert torch.all(gp[:, ~hit] == 0)
        else:
            assert gp is None and gh is None


def _pipeline64(h64, attr64, s, T, o, d, prim, b, mode, w):
    """float64 loss of the whole chain for fixed hit triangles: the surface point of smooth_ref.surface, then the
    attribute at it"""
    sf = S.surface(h64, s, T, False, o, d, prim, b, mode)
    V = S.world_vertices(h64, s, T)
    return (R.vertex(attr64, V, prim, sf["p"]) * w).sum()


@pytest.mark.parametrize("mode", ["default", "follow"])
def test_chain_against_central_differences(hf, mode):
    W, H = 33, 21
    shape, h, s, T, ray, _ = _setup(hf, W, H, "affine", n=4096, seed=2)
    flags = hf.RayFlags.All | (hf.RayFlags.FollowShape if mode == "follow" else 0)
    name = "vertex_a3"
    shape.heightfield.requires_grad_(True)
    attr = shape.attributes[name].requires_grad_(True)
    si = shape.ray_intersect(ray, flags)
    hit = si.is_valid()
    # grazing hits are where float32 and float64 part ways: weight 0 (as test_gpu_full_size)
    cos = (si.n.detach() * ray.d).sum(0).abs() / ray.d.norm(dim=0)
    w = torch.where(hit & (cos > 0.1), torch.rand(len(ray), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)),
                    torch.zeros(len(ray), device=DEV))
    wv = torch.stack([w, 0.5 * w, -w])
    v = shape.eval_attribute_3(name, si)
    (v * wv).sum().backward()
    gh, ga = shape.heightfield.grad.clone(), attr.grad.clone()
    shape.heightfield.requires_grad_(False)
    attr.requires_grad_(False)

    sel = hit.nonzero()[:, 0]
    prim = si.prim_index[sel].long()
    o, d = ray.o[:, sel].T.double(), ray.d[:, sel].T.double()
    b = (si.prim_uv[0, sel].double(), si.prim_uv[1, sel].double())
    wsel = wv[:, sel].T.double()
    h64 = torch.from_numpy(h).double().to(DEV)
    attr64 = shape.attributes[name].double().reshape(-1, 3)
    # dL/dattr: the loss is linear in the attribute, so central differences are exact up to rounding: autograd
    a64 = attr64.clone().requires_grad_(True)
    _pipeline64(h64, a64, s, T, o, d, prim, b, mode, wsel).backward()
    assert _rel(ga, a64.grad.reshape(-1)) <= 1e-5
    # dL/dheight: central differences on the texels with the largest gradients
    hg = h64.clone().requires_grad_(True)
    _pipeline64(hg, attr64, s, T, o, d, prim, b, mode, wsel).backward()
    if mode == "follow":
        # with frozen barycentrics, p moves with the triangle and the weights of the attribute stay put: the direct
        # path (the vertices) and the path through si.p cancel
        ref_scale = float(torch.linalg.norm(hg.grad))
        assert ref_scale <= 1e-8
        shape2, *_ = _setup(hf, W, H, "affine", n=4096, seed=2)
        shape2.heightfield.requires_grad_(True)
        si2 = shape2.ray_intersect(ray)
        (shape2.eval_attribute_3(name, si2) * wv).sum().backward()
        assert float(torch.linalg.norm(gh)) <= 1e-4 * float(torch.linalg.norm(shape2.heightfield.grad))
        return
    top = hg.grad.abs().reshape(-1).topk(48).indices
    eps = 1e-5
    fd = []
    for k in top.tolist():
        hp, hm = h64.clone(), h64.clone()
        hp.view(-1)[k] += eps
        hm.view(-1)[k] -= eps
        fd.append(float(_pipeline64(hp, attr64, s, T, o, d, prim, b, mode, wsel) -
                        _pipeline64(hm, attr64, s, T, o, d, prim, b, mode, wsel)) / (2 * eps))
    fd = torch.tensor(fd, dtype=torch.float64)
    dev_g = gh.reshape(-1)[top].double().cpu()
    rel = float(torch.linalg.norm(dev_g - fd) / torch.linalg.norm(fd))
    print("attribute chain: rel L2 vs central differences", rel)
    assert rel <= 2e-3, rel


# ---- 4. forward mode ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,tw", FIELDS[1:])
def test_tangent_is_the_transpose_and_repeatable(hf, W, H, tw):
    shape, h, s, T, ray, active = _setup(hf, W, H, tw, seed=3)
    si = shape.ray_intersect(ray)
    n = len(ray)
    gen = torch.Generator(device=DEV).manual_seed(9)
    dh = torch.randn((H, W), device=DEV, generator=gen)
    dp = torch.randn((3, n), device=DEV, generator=gen)
    for name in ("vertex_a1", "vertex_a3", "face_a1", "face_a3"):
        size = shape._attr_meta[name][1]
        da = torch.randn(shape.attributes[name].numel(), device=DEV, generator=gen)
        g = torch.randn((size, n), device=DEV, generator=gen)
        tan = shape.eval_attribute_tangent(name, si, da, dp, dh, active)
        assert torch.equal(tan, shape.eval_attribute_tangent(name, si, da, dp, dh, active)), name
        ga, gp, gh = shape.eval_attribute_adjoint(name, si, g, active)
        lhs = float((ga.double() * da.double()).sum())
        if gp is not None:
            lhs += float((gp.double() * dp.double()).sum() + (gh.double() * dh.double()).sum())
        rhs = float((g.double() * tan.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * max(abs(rhs), 1e-3), (name, lhs, rhs)


def test_forward_ad_through_the_function(hf):
    shape, h, s, T, ray, active = _setup(hf, 33, 21, "affine", seed=4)
    si = shape.ray_intersect(ray)
    n = len(ray)
    gen = torch.Generator(device=DEV).manual_seed(11)
    name = "vertex_a3"
    buf = shape.attributes[name]
    da = torch.randn(buf.numel(), device=DEV, generator=gen)
    dp = torch.randn((3, n), device=DEV, generator=gen)
    dh = torch.randn((21, 33), device=DEV, generator=gen)
    ref = shape.eval_attribute_tangent(name, si, da, dp, dh, active)
    h = shape.heightfield
    with fwAD.dual_level():
        shape.attributes[name] = fwAD.make_dual(buf, da)
        shape.heightfield = fwAD.make_dual(h, dh)
        si2 = _si(hf, fwAD.make_dual(si.p.detach(), dp), si.prim_index, si.t)
        out = shape.eval_attribute_3(name, si2, active)
        tan = fwAD.unpack_dual(out).tangent
    shape.attributes[name], shape.heightfield = buf, h
    assert tan is not None and torch.allclose(tan, ref, rtol=0, atol=1e-6 * float(ref.abs().max()))


# ---- 5. capture, and nothing else moves -----------------------------------------------------------------------------

def test_graph_capture_replays_to_eager(hf):
    shape, h, s, T, ray, active = _setup(hf, 257, 257, "affine", seed=5)
    si = shape.ray_intersect(ray)
    n = len(ray)
    g = torch.randn((3, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    name = "vertex_a3"
    attr = shape.attributes[name]
    p, prim, t = shape._attr_si(si)
    ga, gh = torch.zeros_like(attr), torch.zeros((257, 257), device=DEV)

    def step():
        v = shape._attr_forward_raw(name, attr, p, prim, t, None)
        _, gp, _ = shape._attr_adjoint_raw(name, attr, p, prim, t, None, g, grad_attr=ga, grad_h=gh)
        return v, gp
    v_e, gp_e = step()
    ga_e, gh_e = ga.clone(), gh.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v_g, gp_g = step()
    ga.zero_(); gh.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(v_g, v_e) and torch.equal(gp_g, gp_e)
    assert torch.allclose(ga, ga_e, rtol=1e-5, atol=1e-6) and torch.allclose(gh, gh_e, rtol=1e-4, atol=1e-5)
    del graph


def test_existing_outputs_do_not_move(hf):
    rng = np.random.default_rng(6)
    hn = rng.uniform(0.1, 0.9, (65, 65)).astype(np.float32)
    plain = hf.Heightfield(heightfield=torch.from_numpy(hn).to(DEV), max_height=0.6)
    with_attr = hf.Heightfield(heightfield=torch.from_numpy(hn).to(DEV), max_height=0.6,
                               vertex_color=torch.rand((65, 65, 3)), face_mono=torch.rand((2 * 64 * 64, 1)))
    r = common.random_rays(8192, rng)
    ray = hf.Ray3f(torch.from_numpy(r[0:3]).to(DEV), torch.from_numpy(r[3:6]).to(DEV), torch.from_numpy(r[6]).to(DEV))
    a, b = plain.ray_intersect(ray), with_attr.ray_intersect(ray)
    for k in ("t", "p", "n", "uv", "dp_du", "dp_dv", "prim_index"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    with_attr.eval_attribute("vertex_color", b)
    pa = hf.PreliminaryIntersection3f(a.t, a.prim_uv, a.prim_index, plain)
    g = torch.zeros((18, len(ray)), device=DEV)
    g[0] = a.is_valid().float()
    g[4:7] = torch.rand((3, len(ray)), device=DEV)
    ga = plain.adjoint(ray, pa, g)
    gb = with_attr.adjoint(ray, pa, g)
    # (float atomics: the order of the adds differs from launch to launch, so equal up to that)
    assert torch.allclose(ga, gb, rtol=1e-5, atol=1e-6 * float(ga.abs().max()))


# ---- 6. joint recovery ----------------------------------------------------------------------------------------------

def test_joint_recovery_of_heights_and_reflectance(hf):
    """65^2 field, four lights, spp 1, box film: heights (hf_amd.Adam) and a vertex_reflectance map
    (torch.optim.Adam) from a flat start.  Measured on an MI355X: loss 1.84e-2 -> 4.79e-4 (38x), reflectance RMS error
    over the vertices the camera sees 0.164 -> 0.089; the thresholds are 10x and 0.6x."""
    N, film, steps = 65, 128, 300
    u = torch.linspace(0, 1, N)
    true_h = (0.5 + 0.2 * torch.sin(2 * math.pi * u)[None, :] * torch.cos(2 * math.pi * u)[:, None]).to(DEV)
    true_a = (0.6 + 0.25 * torch.sin(3 * math.pi * u)[:, None] * torch.sin(2 * math.pi * u)[None, :]).to(DEV)
    lights = torch.cat([LIGHTS / LIGHTS.norm(dim=1, keepdim=True), torch.full((4, 1), math.pi)], 1)
    rays = hf.workload.ortho_rays(film, film, 1, DEV, seed=0, origin=(0.6, 0.35, 2.0), target=(0.0, 0.0, 0.25),
                                  scale=(0.95, 0.95, 1.0))
    ray = hf.Ray3f(rays[0:3], rays[3:6], rays[6])

    def render(shape):
        si = shape.ray_intersect(ray)
        shading = hf.direct_lighting(si, ray, lights, albedo=1.0, spp=1)       # [4, n]
        return shading * shape.eval_attribute_1("vertex_reflectance", si)[None]

    target = hf.Heightfield(heightfield=true_h, max_height=0.5, vertex_reflectance=true_a[:, :, None])
    with torch.no_grad():
        tgt = render(target)
    shape = hf.Heightfield(heightfield=torch.full_like(true_h, 0.5), max_height=0.5,
                           vertex_reflectance=torch.full((N, N, 1), 0.5))
    shape.heightfield.requires_grad_(True)
    attr = shape.attributes["vertex_reflectance"].requires_grad_(True)
    opt_h = hf.Adam(shape, lr=0.01)
    opt_a = torch.optim.Adam([attr], lr=0.02)
    seen = torch.zeros(N * N, dtype=torch.bool, device=DEV)   # vertices some hit reads: the others keep their start
    losses = []
    for _ in range(steps):
        opt_h.zero_grad(); opt_a.zero_grad()
        loss = ((render(shape) - tgt) ** 2).mean()
        loss.backward()
        seen |= attr.grad != 0
        opt_h.step(); opt_a.step()
        losses.append(float(loss.detach()))
    err0 = (0.5 - true_a.reshape(-1))[seen]
    err = (attr.detach() - true_a.reshape(-1))[seen]
    rms0, rms = float(err0.pow(2).mean().sqrt()), float(err.pow(2).mean().sqrt())
    print(f"joint recovery: loss {losses[0]:.3e} -> {losses[-1]:.3e}, albedo rms {rms0:.4f} -> {rms:.4f} "
          f"over {int(seen.sum())} of {N * N} vertices")
    assert losses[-1] <= losses[0] / 10
    assert rms <= 0.6 * rms0

"""Forward mode (hf_tangent and the two lighting tangents), the parts that need no GPU:
  * include/hf.h declares the three entry points, libhf.so exports them and _capi.SYMBOLS binds them;
  * the shipped gfx950 code object holds their kernels, without spills and within the private-segment rule;
  * the Mitsuba adapter's CustomOp::forward() runs hf_tangent instead of throwing;
  * the yardstick of tests/test_gpu_tangent.py checked against itself: the float64 directional finite difference of
    tests/si_numpy.py is the transpose of the C oracle's adjoint, <ybar, J delta> = <J^T ybar, delta>, ray by ray,
    in all three modes, with flipped normals and a general affine to_world."""
import os
import re
import tempfile

import numpy as np
import pytest

import common
import si_numpy as S
from test_code_object import LLVM, MAX_PRIVATE_BYTES, _code_object, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hf_tangent", "hf_direct_lighting_weighted_tangent", "hf_point_lighting_tangent"]


def test_header_declares_and_library_exports_the_tangents():
    import ctypes as C
    import hf_amd
    hdr = open(os.path.join(ROOT, "include", "hf.h")).read()
    lib = C.CDLL(hf_amd.build.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), f"{name} not declared in hf.h"
        assert name in hf_amd._capi.SYMBOLS, f"{name} missing from _capi.SYMBOLS"
        getattr(lib, name)   # AttributeError if not exported
    assert "hf_si_tangent_t" in hdr
    # the header's HIP-graph section names them among the capturable entry points
    graphs = hdr[hdr.index("HIP graphs"):hdr.index("#ifndef HF_H")]
    assert all(name in graphs for name in NEW)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(_code_object())
    yield {k["name"]: k for k in _kernels(f.name)}
    os.unlink(f.name)


@pytest.mark.parametrize("frag", ["hf_tangent_kernelILb0", "hf_tangent_kernelILb1",
                                  "hf_direct_tangent_kernelILb0", "hf_direct_tangent_kernelILb1"])
def test_tangent_kernels_in_the_code_object_without_spills(kernels, frag):
    hit = [k for n, k in kernels.items() if frag in n]
    assert len(hit) == 1, f"kernel {frag} not found in {sorted(kernels)}"
    k = hit[0]
    assert int(k["vgpr_spill_count"]) == 0 and int(k.get("sgpr_spill_count", 0)) == 0, k
    assert int(k["private_segment_fixed_size"]) <= MAX_PRIVATE_BYTES
    assert k.get("uses_dynamic_stack", "false") == "false"
    assert int(k["vgpr_count"]) <= 128


def test_adapter_forward_runs_hf_tangent():
    src = open(os.path.join(ROOT, "adapters", "mitsuba3", "heightfield.cpp")).read()
    body = src[src.index("void forward() override"):src.index("const char *name() const override")]
    assert "Throw(" not in body, "CustomOp::forward() still refuses forward mode"
    assert "grad_in<0>" in body and "set_grad_out" in body and "si_tangent" in body
    tangent = src[src.index("void si_tangent("):src.index("std::string to_string()")]
    assert re.search(r"\bhf_tangent\s*\(", tangent)


# ---- the yardstick: directional finite differences of si_numpy vs the oracle's adjoint -------------------------

def fd_directional(h, s, tw, flip, o, d, prim, flags, uv_fixed, dh, do, dd, eps=1e-6):
    """float64 central difference of the 18 differentiable rows along (dh, do, dd)"""
    def rows(e):
        si = S.surface_interaction(h + e * dh, s, tw, flip, o + e * do, d + e * dd, prim, flags, uv_fixed, h)
        return np.concatenate([np.atleast_1d(np.asarray(si[nm], np.float64)) for nm, _ in S.GRAD_FIELDS])
    return (rows(eps) - rows(-eps)) / (2 * eps)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("mode", ["default", "follow", "detach"])
def test_fd_yardstick_is_the_transpose_of_the_oracle_adjoint(oracle, mode, flip):
    rng = np.random.default_rng(11)
    W, H, s = 9, 7, 0.6
    h = rng.uniform(0.2, 0.8, (H, W)).astype(np.float32)
    tw = common.affine(5)
    f = oracle.OracleField(h, max_height=s, to_world=tw, flip_normals=flip)
    n = 32
    r = common.to_world_rays(common.random_rays(n, rng, s), tw)
    t, u, v, prim = f.ray_intersect_preliminary(r)
    flags = S.RAY_ALL | {"default": 0, "follow": S.RAY_FOLLOWSHAPE, "detach": S.RAY_DETACHSHAPE}[mode]
    si = f.compute_surface_interaction(r, t, u, v, prim, flags)
    h64 = h.astype(np.float64)
    checked = 0
    for k in np.where(np.isfinite(t))[0]:
        if abs(float(si["n"][:, k] @ r[3:6, k])) < 1e-2 * np.linalg.norm(r[3:6, k]):
            continue   # grazing rays (as the existing FD tests)
        dh = rng.normal(size=(H, W)); do = rng.normal(size=3); dd = rng.normal(size=3)
        ybar = rng.normal(size=18)
        jd = fd_directional(h64, s, tw, flip, r[0:3, k].astype(np.float64), r[3:6, k].astype(np.float64), prim[k],
                            flags, (u[k], v[k]), dh, do, dd)
        g = {}
        i = 0
        for nm, c in S.GRAD_FIELDS:
            g[nm] = np.zeros((c, n), np.float32)
            g[nm][:, k] = ybar[i:i + c]
            i += c
        gh, go, gd = f.adjoint(r, t, u, v, prim, g, flags, ray_grads=True)
        lhs = float(ybar @ jd)
        rhs = float(np.sum(dh * gh) + do @ go[:, k] + dd @ gd[:, k])
        scale = float(np.abs(ybar * jd).sum()) + 1e-12
        assert abs(lhs - rhs) <= 2e-4 * scale, (mode, flip, k, lhs, rhs)
        if mode == "detach":   # the height direction contributes nothing, the ray direction does
            jh = fd_directional(h64, s, tw, flip, r[0:3, k].astype(np.float64), r[3:6, k].astype(np.float64), prim[k],
                                flags, (u[k], v[k]), dh, 0 * do, 0 * dd)
            assert np.all(jh == 0)
        checked += 1
    assert checked >= 8

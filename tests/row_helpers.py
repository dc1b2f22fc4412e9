"""Shared pieces of the lighting rows' GPU tests (tests/test_gpu_sky_lighting.py, _bounce_lighting, _envmap_lighting,
_caustic, _reflect, _glossy): conversions, the records of a scene as leaves of their own, the scene every row starts
from, the guard-band kit and the transposition gap.  Plain functions; nothing here caches: the _SCENES dicts and the
module-scoped fixtures stay with the files that own them."""
import types

import numpy as np
import torch

import envmap_ref as E
from lighting_scenes import _np

GUARD = -12345.0
# a mask is decided by the sign of a float32 quantity; a sample on which rounding may decide it (the row's own MARGIN) is
# left out of mask comparisons, and at most this share of the samples may be left out
UNSURE_CAP = 1e-3


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / np.linalg.norm(ref))


def _fold(gd):
    """the gradient of the [H, W] map folded onto the [H, W - 1] texels: the seam column is a copy of column 0"""
    out = gd[:, :-1].copy()
    out[:, 0] += gd[:, -1]
    return out


def leaf_si(hf, sc, sh_n=None):
    """the records of sc.si detached, with sh_n a leaf that requires a gradient (or the given tensor, a dual for instance)"""
    si = hf.SurfaceInteraction3f()
    si.p, si.n, si.t = sc.si.p.detach(), sc.si.n.detach(), sc.si.t.detach()
    si.sh_frame = hf.Frame3f(None, None, sc.si.sh_frame.n.detach().clone().requires_grad_(True) if sh_n is None else sh_n)
    return si


def sub(hf, sc, lo, hi, requires_grad=False):
    """(si, ray) of the samples [lo, hi) as records of their own"""
    si = hf.SurfaceInteraction3f()
    cut = lambda x: x.detach()[..., lo:hi].contiguous()
    si.p, si.n, si.t = cut(sc.si.p), cut(sc.si.n), cut(sc.si.t)
    si.sh_frame = hf.Frame3f(None, None, cut(sc.si.sh_frame.n).requires_grad_(requires_grad))
    return si, hf.Ray3f(cut(sc.ray.o), cut(sc.ray.d))


def envmap(hf, sizes, rots, name, rname, requires_grad=False):
    """(Envmap, the [H, W] map with its seam column as numpy, the rotation): the map envmap_ref.MAPS[name] at the size
    sizes[name] = (W, H) under the rotation rots[rname]"""
    full = E.MAPS[name](*sizes[name])
    data = _cu(full[:, :-1].astype(np.float32))
    if requires_grad:
        data.requires_grad_(True)
    return hf.Envmap(data, to_world=rots[rname]), full, rots[rname]


def base_scene(hf, oracle, film, origin, face_normals=True):
    """sine_heights(96, 96) at max_height 0.5 in the given shading mode, the orthographic wavefront `film` = (width,
    height, spp) from `origin`, its surface interactions, the records as numpy (sc.np: p, n, sh_n, d, t), the hit mask and
    the oracle's field.  A row's file adds its own members on top and owns the cache."""
    h = hf.workload.sine_heights(96, 96, device="cuda")
    shape = hf.Heightfield(heightfield=h, max_height=0.5, face_normals=face_normals)
    rays = hf.workload.ortho_rays(*film, "cuda", seed=1, origin=origin, target=(0.0, 0.0, 0.25), scale=(0.9, 0.9, 1.0))
    ray = hf.Ray3f(rays[0:3], rays[3:6], rays[6])
    si = shape.ray_intersect(ray, hf.RayFlags.All)
    sc = types.SimpleNamespace(h=h, shape=shape, rays=rays, ray=ray, si=si, n=len(ray))
    sc.np = {k: _np(v) for k, v in (("p", si.p), ("n", si.n), ("sh_n", si.sh_frame.n), ("d", ray.d), ("t", si.t))}
    sc.hit = np.isfinite(sc.np["t"])
    sc.field = oracle.OracleField(_np(h), max_height=0.5)
    return sc


# ---- the guard-band kit: output rows of n elements with G guard elements on either side -------------------------------
def rows(x):
    """the row pointers of a contiguous [k, n] float32 tensor"""
    from hf_amd import _capi
    return (_capi._fp * x.shape[0])(*[x.data_ptr() + 4 * (k * x.shape[1]) for k in range(x.shape[0])])


def guarded(n, G, k=1, dtype=torch.float32):
    """(a [k, G + n + G] buffer of 4-byte elements filled with GUARD, the k pointers to element G of each row)"""
    from hf_amd import _capi
    buf = torch.full((k, n + 2 * G), GUARD, device="cuda").to(dtype)
    return buf, (_capi._fp * k)(*[buf.data_ptr() + 4 * (j * (n + 2 * G) + G) for j in range(k)])


def intact(buf, n, G):
    """both guard bands of every row still hold GUARD and no element between them does"""
    return bool((buf[:, :G] == GUARD).all()) and bool((buf[:, G + n:] == GUARD).all()) and bool((buf[:, G:G + n] != GUARD).all())


def transposition_gap(lhs_terms, rhs_terms):
    """|<J u, v> - <u, J^T v>|: each term is a pair of arrays, float32 results among them, multiplied and added up in
    float64.  The bound it is compared with is built from a row's own tolerances and stays in that row's test."""
    side = lambda terms: sum((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum() for a, b in terms)
    return abs(side(lhs_terms) - side(rhs_terms))

"""The float64 restatement of the bump map (tests/bumpmap_ref.py) against itself and against hand-placed lanes, on the CPU:
the tangent against Richardson-extrapolated central differences in each of tex, uv, sh_n, dp_du and dp_dv, the adjoint (a
reverse sweep written on its own) against the tangent by transposition, N unit, the known answers of a ramp and of a flipped
geometric normal, the flat and the 1 x 1 texture, scale against a scaled texture, the pass-through lanes, and the conditions
on the oracle's records of the GPU test's scenes that make those scenes a test: asserted here and, on the GPU's own
records, in tests/test_gpu_bumpmap.py before anything is compared.  Last, the table bumpmap_ref.F32 against the record of
scripts/bumpmap_f32_error.py."""
import json
import os

import numpy as np
import pytest

import bumpmap_ref as R
import row_scenes as RS
from row_helpers import UNSURE_CAP

NAN, INF = float("nan"), float("inf")


def _lanes(n, seed=5):
    """well-conditioned lanes: b unit, dp_du and dp_dv of length 0.5 .. 2 at 50 .. 130 degrees to each other in a plane
    tilted against b by at most about 35 degrees, n_geo the unit normal of that plane on b's side, uv over [-0.5, 1.5]^2
    (outside [0, 1]: where the wrap decides)"""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(3, n))
    b /= np.linalg.norm(b, axis=0)
    ng = b + 0.35 * rng.normal(size=(3, n))
    ng /= np.linalg.norm(ng, axis=0)
    e0 = np.cross(ng.T, rng.normal(size=(n, 3))).T
    e0 /= np.linalg.norm(e0, axis=0)
    e1 = np.cross(ng.T, e0.T).T
    ang = np.radians(rng.uniform(50, 130, n))
    u = e0 * rng.uniform(0.5, 2.0, n)
    v = (e0 * np.cos(ang) + e1 * np.sin(ang)) * rng.uniform(0.5, 2.0, n)
    uv = rng.uniform(-0.5, 1.5, size=(2, n))
    return uv, b, ng, u, v


def _away_from_edges(uv, TW, TH, margin):
    pos = R.positions(uv, TW, TH)
    f = (pos - 0.5) - np.floor(pos - 0.5)
    return (np.minimum(f, 1 - f) > margin).all(0)


@pytest.fixture(scope="module", params=["clamp", "repeat"])
def case(request):
    TW, TH, scale = 7, 5, 1.5
    wrap = R.WRAPS[request.param]
    uv, b, ng, u, v = _lanes(400)
    keep = _away_from_edges(uv, TW, TH, 0.02)               # strictly inside their cells
    uv, b, ng, u, v = (a[:, keep] for a in (uv, b, ng, u, v))
    tex = R.texture(TW, TH, seed=2, amplitude=0.1).astype(np.float64)
    # ... and away from the flip of sigma and from short c, where a finite difference would cross a jump or divide by little
    _, _, s = R.forward(tex, uv, b, ng, u, v, None, wrap, scale)
    keep = (np.abs(s.cosine) > 0.3) & (s.rC < 10)
    assert keep.sum() > 250
    uv, b, ng, u, v = (a[:, keep] for a in (uv, b, ng, u, v))
    x = R.inputs(uv.shape[1], tex.shape)
    for k, val in vars(x).items():        # (float64: a step times a float32 array would be rounded to float32)
        setattr(x, k, val.astype(np.float64))
    return tex, uv, b, ng, u, v, wrap, scale, x


def _richardson(f, h):
    """the central difference of f at 0 with steps h and h / 2, extrapolated: error O(h^4)"""
    d = lambda s: (f(s) - f(-s)) / (2 * s)
    return (4 * d(h / 2) - d(h)) / 3


def test_tangent_against_richardson_extrapolated_central_differences(case):
    """each of tex, uv, sh_n, dp_du, dp_dv alone.  h = 1e-4: the extrapolated difference is off by about h^4 / 30 times a
    fifth derivative along the direction, which is of the order of the first one to the fifth power -- |dN| reaches 40 for
    the texels, whose tangent is multiplied by TW, TH and scale: 1e-16 x 1e8 / 30, some 1e-10 (at h = 1e-3 it is 1e-6 to 1e-5
    and was measured as 2e-5) --, plus rounding 1e-16 / h = 1e-12; the bound 1e-8 of the largest |dN| (DESIGN 4.28's) leaves
    both a margin and is far below any term of the tangent.  The samples stay strictly inside their cells (0.02 of a texel
    against steps of 1e-6 in uv), away from the flip of sigma and from short c"""
    tex, uv, b, ng, u, v, wrap, scale, x = case
    N, mask, s = R.forward(tex, uv, b, ng, u, v, None, wrap, scale)
    assert mask.all() and np.abs(s.cosine).min() > 0.3
    zero = dict(dtex=None, duv=None, db=None, ddu=None, ddv=None)
    moves = {"dtex": lambda h: (tex + h * x.dtex, uv, b, ng, u, v), "duv": lambda h: (tex, uv + h * x.duv, b, ng, u, v),
             "db": lambda h: (tex, uv, b + h * x.db, ng, u, v), "ddu": lambda h: (tex, uv, b, ng, u + h * x.ddu, v),
             "ddv": lambda h: (tex, uv, b, ng, u, v + h * x.ddv)}
    for k, move in moves.items():
        dN = R.tangent(tex, uv, b, ng, u, v, None, wrap, scale, **dict(zero, **{k: getattr(x, k)}))
        fd = _richardson(lambda h: R.forward(*move(h), None, wrap, scale)[0], 1e-4)
        err = np.abs(dN - fd).max()
        print(k, "largest |dN|", np.abs(dN).max(), "difference", err)
        assert np.abs(dN).max() > 1e-2 and err <= 1e-8 * max(1.0, np.abs(dN).max()), (k, err)


def test_the_adjoint_is_the_transpose_of_the_tangent(case):
    tex, uv, b, ng, u, v, wrap, scale, x = case
    dN = R.tangent(tex, uv, b, ng, u, v, None, wrap, scale, x.dtex, x.duv, x.db, x.ddu, x.ddv)
    g = R.adjoint(tex, uv, b, ng, u, v, None, wrap, scale, x.gout)
    lhs = (dN * x.gout).sum()
    rhs = (g.gtex * x.dtex).sum() + (g.guv * x.duv).sum() + (g.gn * x.db).sum() + (g.gpu * x.ddu).sum() + (g.gpv * x.ddv).sum()
    size = np.linalg.norm(dN) * np.linalg.norm(x.gout)
    print("<J u, v>", lhs, "<u, J^T v>", rhs, "size", size)
    assert size > 0 and abs(lhs - rhs) <= 1e-12 * size
    for k in ("gtex", "guv", "gn", "gpu", "gpv"):
        assert np.abs(getattr(g, k)).max() > 0, k


def test_the_result_is_unit_and_on_the_side_of_the_geometric_normal(case):
    tex, uv, b, ng, u, v, wrap, scale, _ = case
    N, _, s = R.forward(tex, uv, b, ng, u, v, None, wrap, scale)
    assert np.abs(np.linalg.norm(N, axis=0) - 1).max() <= 1e-14
    assert ((N * ng).sum(0) > 0).all()
    # N is orthogonal to both projected tangents
    assert np.abs((N * s.Pu).sum(0)).max() <= 1e-13 and np.abs((N * s.Pv).sum(0)).max() <= 1e-13


def _axis_lanes(n, Sx, Sy, z=1.0, seed=9):
    rng = np.random.default_rng(seed)
    one = np.ones(n)
    b = np.stack([0 * one, 0 * one, one])
    return rng.uniform(0.1, 0.9, size=(2, n)), b, b * z, np.stack([Sx * one, 0 * one, 0 * one]), np.stack([0 * one, Sy * one, 0 * one])


@pytest.mark.parametrize("axis", ["u", "v"])
def test_a_ramp_tilts_the_normal_by_its_slope_and_a_flipped_geometric_normal_negates_it(axis):
    """b = n_geo = (0, 0, 1), dp_du = (Sx, 0, 0), dp_dv = (0, Sy, 0), under clamp a ramp tex[iy][ix] = k (ix + 0.5) / TW:
    at interior positions Lx = k / TW, g = (scale k, 0), P_u = (Sx, 0, scale k), P_v = (0, Sy, 0) and
    N = (-scale k, 0, Sx) / sqrt(scale^2 k^2 + Sx^2); a ramp in v likewise with Sy.  With n_geo = (0, 0, -1): -N"""
    TW, TH, k, scale, Sx, Sy = 9, 6, 0.8, 1.75, 1.5, 0.6
    y, x = np.meshgrid((np.arange(TH) + 0.5) / TH, (np.arange(TW) + 0.5) / TW, indexing="ij")
    tex = k * (x if axis == "u" else y)
    uv, b, ng, u, v = _axis_lanes(200, Sx, Sy)
    N, mask, _ = R.forward(tex, uv, b, ng, u, v, None, R.CLAMP, scale)
    S = Sx if axis == "u" else Sy
    want = np.zeros(3)
    want[0 if axis == "u" else 1], want[2] = -scale * k, S
    want /= np.hypot(scale * k, S)
    assert mask.all() and np.abs(N - want[:, None]).max() <= 1e-14
    Nf, maskf, sf = R.forward(tex, uv, b, -ng, u, v, None, R.CLAMP, scale)
    assert maskf.all() and (sf.sigma == -1).all() and np.array_equal(Nf, -N)


@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
def test_flat_and_one_texel_textures_give_the_base_normal_to_rounding(wrap):
    """g = 0: c = (u - b <b, u>) x (v - b <b, v>) is parallel to b, so N = +-b within 1e-14 in float64; the sign is n_geo's
    side, which is b's wherever <b, n_geo> > 0 (for a right-handed dp_du, dp_dv about n_geo, as _lanes builds them)"""
    uv, b, ng, u, v = _lanes(300, seed=7)
    same_side = (b * ng).sum(0) > 0
    assert same_side.sum() > 200
    for tex in (np.full((3, 5), 0.25), np.zeros((3, 5)), np.array([[0.7]])):
        N, mask, _ = R.forward(tex, uv, b, ng, u, v, None, R.WRAPS[wrap], 2.0)
        assert mask.all() and np.abs(N - b)[:, same_side].max() <= 1e-14
        dN_duv = R.tangent(tex, uv, b, ng, u, v, None, R.WRAPS[wrap], 2.0, duv=np.ones((2, 300)))
        assert not dN_duv.any()                                        # C = 0: no slope to move along
        # a b that is not unit -- a float32 normal is unit only to rounding -- is projected out exactly: N = b / |b|, however far
        # b leans against the tangents' normal
        for length in (1 + 3e-7, 0.999, 1.7):
            N, mask, _ = R.forward(tex, uv, length * b, ng, u, v, None, R.WRAPS[wrap], 2.0)
            assert mask.all() and np.abs(N - b)[:, same_side].max() <= 1e-14, length


def test_scale_two_is_the_texture_doubled(case):
    tex, uv, b, ng, u, v, wrap, _, x = case
    a = R.evaluate(tex, uv, b, ng, u, v, None, wrap, 2.0, x, np.ones(uv.shape[1], bool))
    d = R.evaluate(2 * tex, uv, b, ng, u, v, None, wrap, 1.0, x, np.ones(uv.shape[1], bool))
    for k in ("N", "grad_sh_n", "grad_dp_du", "grad_dp_dv"):
        assert np.abs(a[k] - d[k]).max() <= 1e-14 * max(1.0, np.abs(a[k]).max()), k
    # the texels' gradient: d/dtex of f(2 tex) is twice d/d(2 tex)
    assert np.abs(a["grad_tex"] - 2 * d["grad_tex"]).max() <= 1e-13 * np.abs(a["grad_tex"]).max()


def pass_through_lanes(TW=4, TH=3):
    """(tex, uv, b, n_geo, dp_du, dp_dv, active, names): a good lane first, then the hand-placed lanes that must pass through"""
    tex = R.texture(TW, TH, seed=4, amplitude=0.2)
    names = ("good", "inactive", "parallel", "zero_dp_du", "zero_dp_dv", "zero_b", "nan_u", "inf_v", "nan_b", "inf_n_geo", "inf_dp_du", "nan_dp_dv")
    n = len(names)
    col = lambda *a: np.tile(np.array(a, np.float32)[:, None], (1, n))
    uv, b, ng = col(0.3, 0.7), col(0.6, 0.0, 0.8), col(0.0, 0.0, 1.0)
    u, v = col(1.0, 0.5, -0.25), col(-0.25, 1.5, 0.5)
    active = np.ones(n, np.uint8)
    k = names.index
    active[k("inactive")] = 0
    v[:, k("parallel")] = -1.5 * u[:, k("parallel")]          # (the bump only moves both along b: put b into their line)
    b[:, k("parallel")] = u[:, k("parallel")] / np.linalg.norm(u[:, k("parallel")])
    u[:, k("zero_dp_du")] = 0
    v[:, k("zero_dp_dv")] = 0
    b[:, k("zero_b")] = 0
    uv[0, k("nan_u")] = NAN
    uv[1, k("inf_v")] = INF
    b[1, k("nan_b")] = NAN
    ng[0, k("inf_n_geo")] = INF
    u[2, k("inf_dp_du")] = -INF
    v[0, k("nan_dp_dv")] = NAN
    return tex, uv, b, ng, u, v, active, names


@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
def test_pass_through_lanes_give_exact_copies_and_identity_gradients(wrap):
    tex, uv, b, ng, u, v, active, names = pass_through_lanes()
    w = R.WRAPS[wrap]
    n = len(names)
    for dtype in (np.float64, np.float32):
        N, mask, _ = R.forward(tex, uv, b, ng, u, v, active, w, 1.0, dtype)
        assert mask.tolist() == [True] + [False] * (n - 1), dict(zip(names, mask))
        assert np.array_equal(N[:, 1:], b[:, 1:].astype(dtype), equal_nan=True) and not np.array_equal(N[:, 0], b[:, 0])
        x = R.inputs(n, tex.shape)
        dN = R.tangent(tex, uv, b, ng, u, v, active, w, 1.0, x.dtex, x.duv, x.db, x.ddu, x.ddv, dtype)
        assert np.array_equal(dN[:, 1:], x.db[:, 1:].astype(dtype))
        gout = x.gout.copy()
        gout[:, 0] = 0                                              # (nothing from the good lane)
        g = R.adjoint(tex, uv, b, ng, u, v, active, w, 1.0, gout, dtype)
        assert np.array_equal(g.gn[:, 1:], gout[:, 1:].astype(dtype))
        assert not g.guv.any() and not g.gpu.any() and not g.gpv.any() and not g.gtex.any()
    _, _, s = R.forward(tex, uv, b, ng, u, v, active, w)
    # one ulp of freedom in the thresholds' inputs does not matter here: the good lane is far above, `parallel` far below
    assert s.ratio[0] > 1e-3 and s.ratio[names.index("parallel")] < 1e-13, s.ratio


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_conditions_on_the_oracles_records_of_the_gpu_tests_scenes(oracle, name, face_normals):
    """on the records the oracle computes for tests/test_gpu_bumpmap.py's scenes (view `steep`), for both textures, both
    wraps and both scales: every hit is perturbed, no sample lies within a factor of two of the pass-through threshold,
    |<n_geo, c / |c|>| >= 0.2 on every hit, the share of hits within MARGIN of a cell edge stays under
    row_helpers.UNSURE_CAP, and on `mirror_flip` sigma = -1 occurs"""
    sc = RS.scene(name, "steep")
    rec = R.oracle_records(sc, oracle, face_normals)
    assert rec["hit"].sum() >= 1000
    negative = 0
    for TW, TH in R.TEXTURES:
        tex = R.texture(TW, TH)
        for wrap in (R.CLAMP, R.REPEAT):
            for scale in R.SCALES:
                _, _, s = R.forward(tex, *R.record_args(rec), rec["hit"], wrap, scale)
                sh = R.shares(s, rec["hit"])
                print(name, "face" if face_normals else "smooth", (TW, TH), wrap, scale, sh)
                R.conditions(sh, UNSURE_CAP)
                assert not s.pert[~rec["hit"]].any()
                negative += sh["sigma_negative"]
    if name == "mirror_flip":
        assert negative > 0
    # the relief tilts the normal visibly: a map that did nothing would pass every comparison with b
    N, _, _ = R.forward(R.texture(*R.TEXTURES[0]), *R.record_args(rec), rec["hit"], R.REPEAT, R.SCALES[0])
    cosine = (N * rec["sh_n"]).sum(0)[rec["hit"]]
    print("median <N, b>", np.median(cosine))
    assert 0.3 < np.median(cosine) < 0.995, np.median(cosine)


def test_the_f32_table_is_the_record_of_the_error_script():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bumpmap", "f32_error.json")
    rec = json.load(open(path))["maxima"]
    assert set(rec) == set(R.F32) == {R.table_key(TW, TH, s) for TW, TH in R.TEXTURES for s in R.SCALES}
    for key, row in R.F32.items():
        assert set(rec[key]) == {"err_" + k for k in row} and set(row) == set(R.KEYS)
        for k, v in row.items():
            # cut off after three digits, never rounded down below the record
            assert rec[key]["err_" + k] <= v <= rec[key]["err_" + k] * 1.01 + 1e-12, (key, k, v, rec[key]["err_" + k])
            assert R.TOL[key][k] == 4 * v

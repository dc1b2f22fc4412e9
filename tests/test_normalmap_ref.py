"""The float64 restatement of the normal map (tests/normalmap_ref.py) against itself and against hand-placed lanes, on the
CPU: the tangent against Richardson-extrapolated central differences in each of tex, uv, sh_n and dp_du, the adjoint (a
reverse sweep written on its own) against the tangent by transposition, the flat map, the encode / decode round trip, the
pass-through lanes, and the shares on the oracle's records of the GPU test's scenes that make those scenes a test:
asserted here and, on the GPU's own records, in tests/test_gpu_normalmap.py before anything is compared.  Last, the
table normalmap_ref.F32 against the record of scripts/normalmap_f32_error.py."""
import json
import os

import numpy as np
import pytest

import normalmap_ref as R
import row_scenes as RS
from row_helpers import UNSURE_CAP

NAN, INF = float("nan"), float("inf")


def _lanes(n, seed=5):
    """well-conditioned lanes: b unit, dp_du with a part a orthogonal to b of length 0.5 .. 2 and a part along b of at most
    that length, uv over [-0.5, 1.5]^2 (outside [0, 1]: where the wrap decides)"""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(3, n))
    b /= np.linalg.norm(b, axis=0)
    u = rng.normal(size=(3, n))
    a = u - b * (b * u).sum(0)
    a *= rng.uniform(0.5, 2.0, n) / np.linalg.norm(a, axis=0)
    u = a + b * rng.uniform(-1, 1, n) * np.linalg.norm(a, axis=0)
    uv = rng.uniform(-0.5, 1.5, size=(2, n))
    return uv, b, u


def _away_from_edges(uv, TW, TH, margin):
    pos = R.positions(uv, TW, TH)
    f = (pos - 0.5) - np.floor(pos - 0.5)
    return (np.minimum(f, 1 - f) > margin).all(0)


@pytest.fixture(scope="module", params=["clamp", "repeat"])
def case(request):
    TW, TH = 7, 5
    wrap = R.WRAPS[request.param]
    uv, b, u = _lanes(400)
    keep = _away_from_edges(uv, TW, TH, 0.02)
    uv, b, u = uv[:, keep], b[:, keep], u[:, keep]
    tex = R.texture(TW, TH, seed=2).astype(np.float64)
    x = R.inputs(uv.shape[1], tex.shape)
    for k, v in vars(x).items():          # (float64: a step times a float32 array would be rounded to float32)
        setattr(x, k, v.astype(np.float64))
    return tex, uv, b, u, wrap, x


def _richardson(f, h):
    """the central difference of f at 0 with steps h and h / 2, extrapolated: error O(h^4)"""
    d = lambda s: (f(s) - f(-s)) / (2 * s)
    return (4 * d(h / 2) - d(h)) / 3


def test_tangent_against_richardson_extrapolated_central_differences(case):
    """each of tex, uv, sh_n, dp_du alone.  h = 1e-3: the extrapolated difference is off by h^4 f^(5) / 120-ish, about 1e-12
    times derivatives of order 10^2 here (1 / M and 1 / A are at most about 3), plus rounding 1e-16 / h = 1e-13; the bound
    1e-8 of the largest |dN| leaves both a wide margin and is far below any term of the tangent"""
    tex, uv, b, u, wrap, x = case
    N, mask, _ = R.forward(tex, uv, b, u, None, wrap)
    assert mask.all()
    zero = dict(dtex=None, duv=None, db=None, ddp=None)
    moves = {"dtex": lambda s: (tex + s * x.dtex, uv, b, u), "duv": lambda s: (tex, uv + s * x.duv, b, u),
             "db": lambda s: (tex, uv, b + s * x.db, u), "ddp": lambda s: (tex, uv, b, u + s * x.ddp)}
    for k, move in moves.items():
        dN = R.tangent(tex, uv, b, u, None, wrap, **dict(zero, **{k: getattr(x, k)}))
        fd = _richardson(lambda s: R.forward(*move(s), None, wrap)[0], 1e-3)
        err = np.abs(dN - fd).max()
        print(k, "largest |dN|", np.abs(dN).max(), "difference", err)
        assert np.abs(dN).max() > 1e-2 and err <= 1e-8 * max(1.0, np.abs(dN).max()), (k, err)


def test_the_adjoint_is_the_transpose_of_the_tangent(case):
    tex, uv, b, u, wrap, x = case
    dN = R.tangent(tex, uv, b, u, None, wrap, x.dtex, x.duv, x.db, x.ddp)
    g = R.adjoint(tex, uv, b, u, None, wrap, x.gout)
    lhs = (dN * x.gout).sum()
    rhs = (g.gtex * x.dtex).sum() + (g.guv * x.duv).sum() + (g.gn * x.db).sum() + (g.gp * x.ddp).sum()
    size = np.linalg.norm(dN) * np.linalg.norm(x.gout)
    print("<J u, v>", lhs, "<u, J^T v>", rhs, "size", size)
    assert size > 0 and abs(lhs - rhs) <= 1e-12 * size
    for k in ("gtex", "guv", "gn", "gp"):
        assert np.abs(getattr(g, k)).max() > 0, k


def test_the_result_is_unit_and_its_frame_orthonormal(case):
    tex, uv, b, u, wrap, _ = case
    N, _, s = R.forward(tex, uv, b, u, None, wrap)
    assert np.abs(np.linalg.norm(N, axis=0) - 1).max() <= 1e-14
    for p, q in ((s.s0, s.t0), (s.s0, b), (s.t0, b)):
        assert np.abs((p * q).sum(0)).max() <= 1e-14
    # N in the base frame IS m: the map names the normal in the tangent space of the surface
    assert np.abs(np.stack([(N * s.s0).sum(0), (N * s.t0).sum(0), (N * b).sum(0)]) - s.m).max() <= 1e-14


@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_flat_map_gives_the_base_normal_exactly(wrap, dtype):
    uv, b, u = _lanes(300, seed=7)
    b32, u32, uv32 = (v.astype(np.float32) for v in (b, u, uv))
    N, mask, _ = R.forward(R.flat(5, 3), uv32, b32, u32, None, R.WRAPS[wrap], dtype)
    assert mask.all() and np.array_equal(N, b32.astype(dtype))


def test_encode_decode_round_trip():
    rng = np.random.default_rng(1)
    m = rng.normal(size=(3, 6, 4))
    m[2] = np.abs(m[2]) + 0.1
    m /= np.linalg.norm(m, axis=0)
    assert np.abs(R.decode(R.encode(m)) - m).max() <= 1e-15
    assert np.array_equal(R.encode(np.array([0.0, 0.0, 1.0])), [0.5, 0.5, 1.0])
    assert np.array_equal(R.flat(4, 2), np.broadcast_to(np.array([0.5, 0.5, 1.0], np.float32)[:, None, None], (3, 2, 4)))


def pass_through_lanes(TW=4, TH=3):
    """(tex, uv, b, dp_du, active, names): a good lane first, then the hand-placed lanes that must pass through; texel
    (1, 1) of the texture is (0.5, 0.5, 0.5) and lane `grey` reads exactly it"""
    tex = R.texture(TW, TH, seed=4)
    tex[:, 1, 1] = 0.5
    names = ("good", "inactive", "grey", "parallel", "zero_dp_du", "nan_u", "inf_v", "nan_b", "inf_dp_du")
    n = len(names)
    uv = np.tile(np.array([[0.3], [0.7]], np.float32), (1, n))
    b = np.tile(np.array([[0.6], [0.0], [0.8]], np.float32), (1, n))
    u = np.tile(np.array([[1.0], [0.5], [-0.25]], np.float32), (1, n))
    active = np.ones(n, np.uint8)
    k = names.index
    active[k("inactive")] = 0
    uv[:, k("grey")] = ((1 + 0.5) / TW, (1 + 0.5) / TH)      # a texel centre: the lookup is that texel
    u[:, k("parallel")] = 2.5 * b[:, k("parallel")]
    u[:, k("zero_dp_du")] = 0
    uv[0, k("nan_u")] = NAN
    uv[1, k("inf_v")] = INF
    b[1, k("nan_b")] = NAN
    u[2, k("inf_dp_du")] = -INF
    return tex, uv, b, u, active, names


@pytest.mark.parametrize("wrap", ["clamp", "repeat"])
def test_pass_through_lanes_give_exact_copies_and_identity_gradients(wrap):
    tex, uv, b, u, active, names = pass_through_lanes()
    w = R.WRAPS[wrap]
    n = len(names)
    for dtype in (np.float64, np.float32):
        N, mask, _ = R.forward(tex, uv, b, u, active, w, dtype)
        assert mask.tolist() == [True] + [False] * (n - 1), dict(zip(names, mask))
        assert np.array_equal(N[:, 1:], b[:, 1:].astype(dtype), equal_nan=True) and not np.array_equal(N[:, 0], b[:, 0])
        x = R.inputs(n, tex.shape)
        dN = R.tangent(tex, uv, b, u, active, w, x.dtex, x.duv, x.db, x.ddp, dtype)
        assert np.array_equal(dN[:, 1:], x.db[:, 1:].astype(dtype))
        gout = x.gout.copy()
        gout[:, 0] = 0                                              # (nothing from the good lane)
        g = R.adjoint(tex, uv, b, u, active, w, gout, dtype)
        assert np.array_equal(g.gn[:, 1:], gout[:, 1:].astype(dtype)) and not g.guv.any() and not g.gp.any() and not g.gtex.any()
    # one ulp of freedom on either side of the thresholds' inputs does not matter here: no lane is near one
    _, _, s = R.forward(tex, uv, b, u, active, w)
    assert not R.near_threshold(s)[[0, names.index("good")]].any()


@pytest.mark.parametrize("name,face_normals", RS.CASES)
def test_the_shares_on_the_oracles_records_of_the_gpu_tests_scenes(oracle, name, face_normals):
    """on the records the oracle computes for tests/test_gpu_normalmap.py's scenes (view `steep`), for both textures and
    both wraps: the share of hit samples within MARGIN of a cell edge stays under row_helpers.UNSURE_CAP, no sample lies
    within a factor of two of a pass-through threshold, and every hit is perturbed"""
    sc = RS.scene(name, "steep")
    rec = R.oracle_records(sc, oracle, face_normals)
    assert rec["hit"].sum() >= 1000
    for TW, TH in R.TEXTURES:
        tex = R.texture(TW, TH)
        for wrap in (R.CLAMP, R.REPEAT):
            _, _, s = R.forward(tex, rec["uv"], rec["sh_n"], rec["dp_du"], rec["hit"], wrap)
            sh = R.shares(s, rec["hit"])
            print(name, "face" if face_normals else "smooth", (TW, TH), wrap, sh)
            assert sh["near_edge"] <= UNSURE_CAP, sh
            assert sh["near_threshold"] == 0 and sh["perturbed_of_hits"] == 1.0, sh
            assert not s.pert[~rec["hit"]].any()
    # the textures tilt the normal visibly: a map that did nothing would pass every comparison with b
    N, _, _ = R.forward(R.texture(*R.TEXTURES[0]), rec["uv"], rec["sh_n"], rec["dp_du"], rec["hit"], R.REPEAT)
    cosine = (N * rec["sh_n"]).sum(0)[rec["hit"]]
    assert 0.3 < np.median(cosine) < 0.98, np.median(cosine)


def test_the_f32_table_is_the_record_of_the_error_script():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "normalmap", "f32_error.json")
    rec = json.load(open(path))["maxima"]
    assert set(rec) == {"err_" + k for k in R.F32}
    for k, v in R.F32.items():
        # cut off after three digits, never rounded down below the record
        assert rec["err_" + k] <= v <= rec["err_" + k] * 1.01 + 1e-12, (k, v, rec["err_" + k])
        assert R.TOL[k] == 4 * v

"""The restatement of the large-steps operator (tests/largesteps_ref.py) held to its known answers on the CPU, so that the
GPU tests compare the kernels with something that has itself been checked."""
import numpy as np
import pytest
import scipy.sparse as sp

import largesteps_ref as R

GRIDS = [(2, 2), (2, 7), (7, 2), (5, 4), (33, 17)]


@pytest.mark.parametrize("W,H", GRIDS)
def test_matrix_is_symmetric_and_sums_to_one(W, H):
    A = R.matrix(W, H, 19.0)
    assert abs(A - A.T).max() == 0.0
    assert np.allclose(np.asarray(A.sum(axis=0)).ravel(), 1.0, atol=1e-12)        # 1^T A = 1^T
    assert np.allclose(A @ np.full(W * H, 3.5), 3.5, atol=1e-12)                  # a constant field is a fixed point
    g = np.random.default_rng(1).normal(size=(H, W))
    assert abs(R.solve_direct(W, H, 19.0, g).sum() - g.sum()) <= 1e-10 * np.abs(g).sum()


def test_degrees():
    assert R.degrees(2, 2).tolist() == [[2, 3], [3, 2]]
    d = R.degrees(5, 4)
    assert d.tolist() == [[2, 4, 4, 4, 3], [4, 6, 6, 6, 4], [4, 6, 6, 6, 4], [3, 4, 4, 4, 2]]
    d = R.degrees(33, 17)
    assert (d[1:-1, 1:-1] == 6).all() and (d[0, 1:-1] == 4).all() and (d[1:-1, -1] == 4).all()
    assert (d[0, 0], d[0, -1], d[-1, 0], d[-1, -1]) == (2, 3, 3, 2)
    assert R.degrees(2, 7).sum() == 2 * (7 * 1 + 2 * 6 + 6)     # twice the edges: 7 rows of 1, 2 columns of 6, 6 diagonals


def _faces(W, H):
    """the tessellation's triangles: cell (cx, cy) split along v10-v01"""
    f = []
    for cy in range(H - 1):
        for cx in range(W - 1):
            v00, v10, v01, v11 = cy * W + cx, cy * W + cx + 1, (cy + 1) * W + cx, (cy + 1) * W + cx + 1
            f += [(v00, v10, v01), (v11, v01, v10)]
    return np.array(f)


def _laplacian_from_faces(faces, n, lam):
    """I + lam L with L from the unique undirected edges of a face list (a generic mesh construction)"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    adj = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    adj = (adj + adj.T).tocsr()
    deg = np.asarray(adj.sum(axis=1)).ravel()
    return sp.identity(n) + lam * (sp.diags(deg) - adj)


@pytest.mark.parametrize("W,H", [(5, 4), (33, 17)])
def test_matrix_equals_the_mesh_laplacian_of_the_faces(W, H):
    assert abs(R.matrix(W, H, 19.0) - _laplacian_from_faces(_faces(W, H), W * H, 19.0)).max() == 0.0


@pytest.mark.parametrize("W,H", GRIDS)
def test_float32_apply_and_cg_agree_with_float64(W, H):
    lam = 19.0
    v = R.rhs("random", W, H, 3)
    err = np.abs(R.apply_f32(W, H, lam, v) - R.apply_f64(W, H, lam, v)).max()
    assert err <= 8 * 2.0 ** -24 * (1 + 12 * lam) * np.abs(v).max()
    x, it, res = R.cg_f32(W, H, lam, v)
    assert it < 256 and res <= 1e-6
    Rn = R.true_residual(W, H, lam, x, v)
    assert np.linalg.norm(x - R.solve_direct(W, H, lam, v)) <= Rn * (1 + 1e-6) + 1e-12
    assert Rn / np.linalg.norm(v) <= 2e-6


def test_cg_edge_cases():
    W, H = 5, 4
    x, it, res = R.cg_f32(W, H, 19.0, np.zeros((H, W)), guess=np.ones((H, W)))
    assert not x.any() and it == 0 and res == 0.0
    u = R.rhs("random", W, H)
    exact = R.solve_direct(W, H, 19.0, u).astype(np.float32)
    assert R.cg_f32(W, H, 19.0, u, guess=exact)[1] <= 1
    assert R.cg_f32(W, H, 19.0, u, max_iter=2)[1] == 2

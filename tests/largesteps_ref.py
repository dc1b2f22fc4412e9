"""The project's own restatement of the large-steps operator (include/hf.h), written from its formula:

    (A v)_ij = v_ij + lambda (deg_ij v_ij - sum of the neighbours),   A = I + lambda L

on a W x H vertex grid (row i, column j, index i W + j), where vertex (i, j) is adjacent to (i, j-1), (i, j+1),
(i-1, j), (i+1, j), (i+1, j-1) and (i-1, j+1) -- the edges of the tessellation that splits every cell along v10-v01 --
as far as they exist, and deg counts the ones that do.  Three things: A as a scipy.sparse matrix (float64; cached per
grid: treat it as read-only), a direct float64 solve, and conjugate gradients with float32 vectors and float64 dot
products in the operation order of the kernels (the order of a dot product's terms aside)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

# (di, dj) of the six neighbours, in the order the kernels add them up
NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0), (1, -1), (-1, 1))


@functools.lru_cache(maxsize=None)
def adjacency(W, H):
    """the 0/1 adjacency matrix of the grid's vertices, [W H, W H] CSR float64"""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rows, cols = [], []
    for di, dj in NEIGHBOURS:
        ok = (i + di >= 0) & (i + di < H) & (j + dj >= 0) & (j + dj < W)
        rows.append((i * W + j)[ok])
        cols.append(((i + di) * W + (j + dj))[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(W * H, W * H))


@functools.lru_cache(maxsize=None)
def degrees(W, H):
    """[H, W] number of neighbours that exist"""
    return np.asarray(adjacency(W, H).sum(axis=1)).reshape(H, W)


@functools.lru_cache(maxsize=None)
def matrix(W, H, lam):
    """A = I + lam (D - Adj), CSR float64"""
    adj = adjacency(W, H)
    deg = np.asarray(adj.sum(axis=1)).ravel()
    return (sp.identity(W * H, format="csr") + float(lam) * (sp.diags(deg) - adj)).tocsr()


def apply_f64(W, H, lam, v):
    return (matrix(W, H, lam) @ np.asarray(v, np.float64).ravel()).reshape(H, W)


@functools.lru_cache(maxsize=None)
def _lu(W, H, lam):
    return spla.splu(matrix(W, H, lam).tocsc())


def solve_direct(W, H, lam, u):
    """A^-1 u by sparse LU in float64, [H, W]"""
    return _lu(W, H, lam).solve(np.asarray(u, np.float64).ravel()).reshape(H, W)


def apply_f32(W, H, lam, v):
    """A v in float32, one rounding per operation, the neighbours in the order of NEIGHBOURS"""
    v = np.asarray(v, np.float32).reshape(H, W)
    pad = np.zeros((H + 2, W + 2), np.float32)
    pad[1:-1, 1:-1] = v
    s = None
    for di, dj in NEIGHBOURS:
        nb = pad[1 + di:1 + di + H, 1 + dj:1 + dj + W]
        s = nb.copy() if s is None else s + nb
    deg = degrees(W, H).astype(np.float32)
    return v + np.float32(lam) * (deg * v - s)


def dot64(a, b):
    return float(np.sum(a.astype(np.float64) * b.astype(np.float64)))


def cg_f32(W, H, lam, u, guess=None, max_iter=256, rel_tol=1e-6):
    """(v, iterations, |r| / |u|): conjugate gradients as hf_large_steps_solve runs them -- float32 vectors, float64 dot
    products, alpha and beta computed in float64 and rounded once, the residual tested before every iteration, and at
    the end the exact solve in the eigenspace of the constant field (A 1 = 1): (sum(u) - sum(x)) / (W H) added to x"""
    u = np.asarray(u, np.float32).reshape(H, W)
    uu = dot64(u, u)
    if uu == 0.0:
        return np.zeros((H, W), np.float32), 0, 0.0
    if guess is None:
        x, r = np.zeros((H, W), np.float32), u.copy()
    else:
        x = np.asarray(guess, np.float32).reshape(H, W).copy()
        r = u - apply_f32(W, H, lam, x)
    rr, rr_old, p = dot64(r, r), 0.0, None
    tol2 = float(np.float32(rel_tol)) ** 2
    for k in range(max_iter):
        if rr <= tol2 * uu and np.isfinite(rr):
            return _keep_sum(x, u), k, float(np.sqrt(rr / uu))
        if k == 0:
            p = r.copy()
        else:
            p = r + np.float32(rr / rr_old if rr_old != 0.0 else 0.0) * p
        q = apply_f32(W, H, lam, p)
        pq = dot64(p, q)
        alpha = np.float32(rr / pq if pq != 0.0 else 0.0)
        x = x + alpha * p
        r = r - alpha * q
        rr_old, rr = rr, dot64(r, r)
    return _keep_sum(x, u), max_iter, float(np.sqrt(rr / uu))


def _keep_sum(x, u):
    return x + np.float32((u.astype(np.float64).sum() - x.astype(np.float64).sum()) / x.size)


def true_residual(W, H, lam, v, u):
    """|A v - u|_2 in float64"""
    return float(np.linalg.norm(apply_f64(W, H, lam, v) - np.asarray(u, np.float64).reshape(H, W)))


def rhs(kind, W, H, seed=0):
    """the right-hand sides of the tests: 'random' (uniform in [-1, 1)) or 'spike' (one 1 off the centre)"""
    if kind == "random":
        return np.random.default_rng(seed).uniform(-1.0, 1.0, (H, W)).astype(np.float32)
    u = np.zeros((H, W), np.float32)
    u[H // 3, (2 * W) // 3] = 1.0
    return u

"""Float64 restatement of hf_film_splat_weighted, its adjoint and its tangent (include/hf.h): the yardstick of the film
kernels.  Separable as ImageBlock is: per axis a dense table  W[i, p] = w(p - (pos_i - 0.5))  over the pixels p of the
footprint  ceil(pos - 0.5 - r) .. floor(pos - 0.5 + r)  (clamped to the film by the table's extent), zero elsewhere, and
D[i, p] = w'(p - (pos_i - 0.5)):

    w(x) = max(0, e^(alpha x^2) - e^(alpha r^2)),  w'(x) = 2 alpha x e^(alpha x^2) where w(x) > 0 else 0,
    alpha = -1 / (2 stddev^2),  r = 4 stddev,  f = w(x) w(y),  df/dpos_x = -w'(x) w(y),  df/dpos_y = -w(x) w'(y).

numpy only; FilmFn wraps the three operations as a torch.autograd.Function (float64, CPU) so that a film built on top of
them -- the division by the weight plane -- is differentiated by torch in both modes."""
import numpy as np


def axis_tables(pos, size, stddev):
    """(W, D), each [n, size] float64: w and w' of every pixel of one axis for every sample"""
    pos = np.asarray(pos, np.float64)
    alpha, r = -1.0 / (2.0 * stddev * stddev), 4.0 * stddev
    f = pos - 0.5
    x = np.arange(size, dtype=np.float64)[None, :] - f[:, None]
    inside = (np.arange(size)[None, :] >= np.ceil(f - r)[:, None]) & (np.arange(size)[None, :] <= np.floor(f + r)[:, None])
    e = np.exp(alpha * x * x)
    w = np.where(inside, np.maximum(e - np.exp(alpha * r * r), 0.0), 0.0)
    d = np.where(w > 0.0, 2.0 * alpha * x * e, 0.0)
    return w, d


def edge_distance(pos, size, stddev):
    """min over samples and pixels of | |x| - r |: how close any sample is to the kink of w at the radius"""
    f = np.asarray(pos, np.float64) - 0.5
    x = np.arange(size, dtype=np.float64)[None, :] - f[:, None]
    return np.abs(np.abs(x) - 4.0 * stddev).min(axis=1)


def _tables(pos, width, height, stddev):
    wx, dx = axis_tables(pos[0], width, stddev)
    wy, dy = axis_tables(pos[1], height, stddev)
    return wx, dx, wy, dy


def _f64(x, shape=None):
    if x is None:
        return None
    x = np.asarray(x, np.float64)
    return x if shape is None else x.reshape(shape)


def forward(values, sample_weight, pos, width, height, stddev=0.5):
    """(image [K, H W], weight [H W]); sample_weight None = 1"""
    values = _f64(values); K, n = values.shape
    sw = np.ones(n) if sample_weight is None else _f64(sample_weight, n)
    wx, _, wy, _ = _tables(pos, width, height, stddev)
    image = np.einsum("ci,iy,ix->cyx", values, wy, wx).reshape(K, height * width)
    weight = np.einsum("i,iy,ix->yx", sw, wy, wx).reshape(height * width)
    return image, weight


def adjoint(values, sample_weight, pos, width, height, stddev, grad_image, grad_weight=None):
    """(grad_values [K, n], grad_sample_weight [n], grad_pos [2, n]) of <image, grad_image> + <weight, grad_weight>"""
    values = _f64(values); K, n = values.shape
    sw = np.ones(n) if sample_weight is None else _f64(sample_weight, n)
    gi = _f64(grad_image, (K, height, width))
    gw = np.zeros((height, width)) if grad_weight is None else _f64(grad_weight, (height, width))
    wx, dx, wy, dy = _tables(pos, width, height, stddev)
    gv = np.einsum("iy,ix,cyx->ci", wy, wx, gi)
    gsw = np.einsum("iy,ix,yx->i", wy, wx, gw)
    G = np.einsum("ci,cyx->iyx", values, gi) + sw[:, None, None] * gw[None]
    gpx = -np.einsum("iy,ix,iyx->i", wy, dx, G)
    gpy = -np.einsum("iy,ix,iyx->i", dy, wx, G)
    return gv, gsw, np.stack([gpx, gpy])


def tangent(values, sample_weight, pos, width, height, stddev, dvalues=None, dsample_weight=None, dpos=None):
    """(dimage [K, H W], dweight [H W]); every tangent may be None (zero)"""
    values = _f64(values); K, n = values.shape
    sw = np.ones(n) if sample_weight is None else _f64(sample_weight, n)
    dv = np.zeros((K, n)) if dvalues is None else _f64(dvalues, (K, n))
    dsw = np.zeros(n) if dsample_weight is None else _f64(dsample_weight, n)
    dp = np.zeros((2, n)) if dpos is None else _f64(dpos, (2, n))
    wx, dx, wy, dy = _tables(pos, width, height, stddev)
    f = wy[:, :, None] * wx[:, None, :]
    df = -(wy[:, :, None] * dx[:, None, :]) * dp[0][:, None, None] - (dy[:, :, None] * wx[:, None, :]) * dp[1][:, None, None]
    dimage = (np.einsum("ci,iyx->cyx", dv, f) + np.einsum("ci,iyx->cyx", values, df)).reshape(K, height * width)
    dweight = (np.einsum("i,iyx->yx", dsw, f) + np.einsum("i,iyx->yx", sw, df)).reshape(height * width)
    return dimage, dweight


def film_fn():
    """the torch.autograd.Function (built on first use: importing this module needs numpy only)"""
    import torch

    class FilmFn(torch.autograd.Function):
        """(image, weight) = forward(values, weight, pos): float64 CPU tensors, differentiable in all three, both modes"""

        @staticmethod
        def forward(ctx, values, sample_weight, pos, width, height, stddev):
            ctx.args = (width, height, stddev)
            ctx.save_for_backward(values, sample_weight, pos)
            ctx.save_for_forward(values, sample_weight, pos)
            image, weight = forward(values.detach().numpy(), sample_weight.detach().numpy(), pos.detach().numpy(), *ctx.args)
            return torch.from_numpy(image), torch.from_numpy(weight)

        @staticmethod
        def jvp(ctx, dvalues, dsample_weight, dpos, *_):
            v, sw, pos = (x.detach().numpy() for x in ctx.saved_tensors)
            num = lambda t: None if t is None else t.detach().numpy()
            dimage, dweight = tangent(v, sw, pos, *ctx.args, num(dvalues), num(dsample_weight), num(dpos))
            return torch.from_numpy(dimage), torch.from_numpy(dweight)

        @staticmethod
        def backward(ctx, grad_image, grad_weight):
            v, sw, pos = (x.detach().numpy() for x in ctx.saved_tensors)
            gv, gsw, gpos = adjoint(v, sw, pos, *ctx.args, grad_image.numpy(), grad_weight.numpy())
            return torch.from_numpy(gv), torch.from_numpy(gsw), torch.from_numpy(gpos), None, None, None

    return FilmFn


def film(values, sample_weight, pos, width, height, stddev=0.5):
    """the normalised film [K, H W] of float64 CPU tensors: accumulated image / accumulated weight where the weight is
    positive, else 0; differentiable by torch in values, sample_weight and pos"""
    import torch
    image, weight = film_fn().apply(values, sample_weight, pos, width, height, stddev)
    covered = weight > 0
    return torch.where(covered[None], image / torch.where(covered, weight, torch.ones_like(weight))[None],
                       torch.zeros_like(image))

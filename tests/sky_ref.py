"""Float64 restatement of the sky-lighting row of include/hf.h (hf_sky_rays, hf_sky_lighting, _adjoint, _tangent):
the sample stream, the directions, the spawned shadow rays, the value, its adjoint and its tangent.  Visibility is an
input (a [K, n] bit array): nothing here traces.  Uses the oracle's sample_tea_32 and nothing of the product."""
import numpy as np

RAY_EPSILON = 1500.0 * 2.0 ** -24      # math.h:18-22


def tea32(v0, v1, rounds=4):
    """sample_tea_32 (random.h:76-91) over arrays; tests/test_sky_abi.py holds it against the oracle's"""
    M = np.uint64(0xFFFFFFFF)
    v0 = np.asarray(v0, np.uint64) & M; v1 = np.asarray(v1, np.uint64) & M
    s = np.uint64(0)
    for _ in range(rounds):
        s = (s + np.uint64(0x9E3779B9)) & M
        v0 = (v0 + ((((v1 << np.uint64(4)) & M) + np.uint64(0xA341316C)) ^ ((v1 + s) & M) ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & M))) & M
        v1 = (v1 + ((((v0 << np.uint64(4)) & M) + np.uint64(0xAD90777D)) ^ ((v0 + s) & M) ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & M))) & M
    return v0, v1


def samples(ids, k, seed):
    """the two 23-bit floats of direction k of the samples with stream ids `ids`: key = sample_tea_32(seed, k)[0] (the
    oracle's), (r0, r1) = sample_tea_32(key, id)"""
    from oracle import hf_oracle
    key, _ = hf_oracle.sample_tea_32(int(seed) & 0xFFFFFFFF, int(k))
    ids = np.asarray(ids, np.uint64)
    r0, r1 = tea32(np.full(ids.shape, key, np.uint64), ids)
    return (r0 >> np.uint64(9)).astype(np.float64) * 2.0 ** -23, (r1 >> np.uint64(9)).astype(np.float64) * 2.0 ** -23


def directions(ids, K, seed):
    """[K, 3, n]: square_to_uniform_sphere (warp.h:250-255) of every sample's K draws; world space"""
    out = np.empty((K, 3, len(ids)))
    for k in range(K):
        sx, sy = samples(ids, k, seed)
        z = 1.0 - 2.0 * sy
        r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        out[k] = np.stack([r * np.cos(2.0 * np.pi * sx), r * np.sin(2.0 * np.pi * sx), z])
    return out


def eligible(sh_n, d, t):
    """the masks of hf_direct_lighting: a hit seen from the front; and |<sh_n, -d>|, the margin of that decision"""
    c = -(np.asarray(sh_n, np.float64) * np.asarray(d, np.float64)).sum(0)
    return np.isfinite(np.asarray(t, np.float64)) & (c > 0), np.abs(c)


def traced(sh_n, d, t, w):
    """[K, n]: direction k of an eligible sample is traced when <sh_n, w_k> > 0; and the margins |<sh_n, w_k>|"""
    el, _ = eligible(sh_n, d, t)
    co = np.einsum("cn,kcn->kn", np.asarray(sh_n, np.float64), w)
    return el[None] & (co > 0), np.abs(co)


def spawn_origin(p, nrm, wk):
    """SurfaceInteraction::spawn_ray(w_k).o (interaction.h:134-136, 161-165): p + n s (1 + max|p_c|) RayEpsilon"""
    p = np.asarray(p, np.float64); nrm = np.asarray(nrm, np.float64)
    mag = (1.0 + np.abs(p).max(0)) * RAY_EPSILON
    mag = np.where((nrm * wk).sum(0) < 0, -mag, mag)
    return p + mag[None] * nrm


def _sums(sh_n, d, t, bits, w):
    """per sample: sum_k bit w_k [3, n] and sum_k bit <sh_n, w_k> [n], bits of samples that are not eligible ignored"""
    el, _ = eligible(sh_n, d, t)
    b = np.asarray(bits, bool) & el[None]
    sw = (b[:, None, :] * w).sum(0)
    return sw, (np.asarray(sh_n, np.float64) * sw).sum(0)


def forward(sh_n, d, t, weight, bits, w, radiance, albedo, spp):
    """(image [n / spp], per-sample values [n])"""
    K = w.shape[0]
    _, sc = _sums(sh_n, d, t, bits, w)
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    value = wgt * (4.0 * albedo * radiance / K) * sc
    return value.reshape(-1, spp).mean(1), value


def adjoint(sh_n, d, t, weight, bits, w, radiance, albedo, spp, grad_image):
    """(grad_sh_n [3, n], grad_weight [n])"""
    K = w.shape[0]
    sw, sc = _sums(sh_n, d, t, bits, w)
    g = np.repeat(np.asarray(grad_image, np.float64), spp) / spp
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    c = 4.0 * albedo * radiance / K
    return (g * wgt * c)[None] * sw, g * c * sc


def tangent(sh_n, d, t, weight, bits, w, radiance, albedo, spp, dsh_n=None, dweight=None):
    """dimage [n / spp] for tangents dsh_n [3, n] and dweight [n] (None: zero)"""
    K = w.shape[0]
    sw, sc = _sums(sh_n, d, t, bits, w)
    wgt = 1.0 if weight is None else np.asarray(weight, np.float64)
    dv = np.zeros(sc.shape)
    if dsh_n is not None:
        dv = dv + wgt * (np.asarray(dsh_n, np.float64) * sw).sum(0)
    if dweight is not None:
        dv = dv + np.asarray(dweight, np.float64) * sc
    return ((4.0 * albedo * radiance / K) * dv).reshape(-1, spp).mean(1)


def unpack(words, K):
    """[K, n] bool from n uint32 visibility words"""
    words = np.asarray(words).view(np.uint32)
    return ((words[None, :] >> np.arange(K, dtype=np.uint32)[:, None]) & 1).astype(bool)

"""numpy float32 restatement of mirt_hit_features and mirt_denoise, written from the comments in include/mirt.h: every operation
rounds to float32 once, in the order the header gives.  expf is the oracle's (test_gpu_parity.py pins it bit for bit to the
device's), normalize the one test_gpu_queries.py restates from vec3.cuh."""
import numpy as np

import oracle_lib
from test_gpu_queries import _normalize

f32 = np.float32
K5 = (f32(0.375), f32(0.25), f32(0.0625))                       # the B3 spline 1/16 1/4 3/8 1/4 1/16, by |offset|
K3 = ((f32(0.0625), f32(0.125), f32(0.0625)), (f32(0.125), f32(0.25), f32(0.125)), (f32(0.0625), f32(0.125), f32(0.0625)))


def expf(x):
    x = np.ascontiguousarray(x, dtype=f32)
    out = np.empty_like(x)
    oracle_lib.lib().orc_math_probe(1, x.size, x.ctypes.data, out.ctypes.data)
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _finite3(c):
    return np.all(np.isfinite(c[..., :3]), axis=-1)


def features(rays, hits):
    """rays float32 [n, 8], hits [n, 6] 4-byte words -> float32 [n, 8]."""
    rays = np.ascontiguousarray(rays, dtype=f32)
    words = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 6)
    t = words[:, 0].copy().view(f32)
    nrm = words[:, 3:6].copy().view(f32)
    out = np.zeros((len(rays), 8), f32)
    with np.errstate(all="ignore"):
        d = _normalize(rays[:, 4:7].copy())
        out[:, 0:3] = rays[:, 0:3] + t[:, None] * d
    out[:, 3] = 1.0
    out[:, 4:7] = nrm
    out[words[:, 1] == 0] = 0
    return out


def prepare(S, Q, k):
    """S, Q float32 [N, 4], k integer [N] -> (c float32 [N, 4], v float32 [N])."""
    S, Q = np.asarray(S, f32).reshape(-1, 4), np.asarray(Q, f32).reshape(-1, 4)
    k = np.asarray(k).astype(np.int64).reshape(-1)
    with np.errstate(all="ignore"):
        nf = k.astype(f32)[:, None]
        c = np.where(k[:, None] != 0, S / nf, f32(0))
        m = S[:, :3] / nf
        q = Q[:, :3] / nf
        t = q - m * m
        t = np.where(t > 0, t, f32(0))
        e = t / (nf - f32(1))
        v = np.fmax(e[:, 0], np.fmax(e[:, 1], e[:, 2]))
        v = np.where(k >= 2, v, f32(0))
    return c.astype(f32), v.astype(f32)


def iteration(c, v, F, s, sigma_c, sigma_n, sigma_p, stats):
    """One a-trous step at distance s: c [H, W, 4], v [H, W], F [H, W, 8] -> (c', v')."""
    H, W = v.shape
    sigma_c, sigma_n, sigma_p = f32(sigma_c), f32(sigma_n), f32(sigma_p)
    Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        g = None
        for j, dy in enumerate((-1, 0, 1)):
            for i, dx in enumerate((-1, 0, 1)):
                term = K3[j][i] * v[np.clip(Y + dy, 0, H - 1), np.clip(X + dx, 0, W - 1)]
                g = term if g is None else g + term
        den = sigma_c * np.sqrt(g) + f32(1e-10)
        centre_ok = _finite3(c)
        hit_p = F[..., 3] != 0
        Pp, Np = F[..., 0:3], F[..., 4:7]
        sw = np.zeros((H, W), f32)
        sv = np.zeros((H, W), f32)
        sc = np.zeros((H, W, 4), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = Y + s * dy, X + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq, vq, Fq = c[qy, qx], v[qy, qx], F[qy, qx]
                valid = inside & _finite3(cq)
                if dx == 0 and dy == 0:
                    a = np.zeros((H, W), f32)
                else:
                    hit_q = Fq[..., 3] != 0
                    valid &= hit_p == hit_q
                    both = hit_p & hit_q
                    a_n = np.fmax(f32(0), f32(1) - _dot(Np, Fq[..., 4:7])) / sigma_n
                    D = Fq[..., 0:3] - Pp
                    l = np.sqrt(_dot(D, D))
                    a_p = np.where(l == 0, f32(0), np.abs(_dot(Np, D)) / (sigma_p * l))
                    a_n, a_p = np.where(both, a_n, f32(0)), np.where(both, a_p, f32(0))
                    d3 = np.abs(c[..., :3] - cq[..., :3])
                    a_c = np.fmax(np.fmax(d3[..., 0], d3[..., 1]), d3[..., 2]) / den
                    t = (a_n + a_p) + a_c
                    valid &= ~np.isnan(t)
                    a = np.fmin(t, f32(87))
                    stats["kept"] += int(np.count_nonzero(valid & centre_ok))
                    stats["skipped"] += int(np.count_nonzero(inside & ~valid & centre_ok))
                w = (K5[abs(dx)] * K5[abs(dy)]) * expf(-a.astype(f32)).reshape(H, W)
                sw = np.where(valid, sw + w, sw)
                sc = np.where(valid[..., None], sc + w[..., None] * cq, sc)
                sv = np.where(valid, sv + (w * w) * vq, sv)
        c2 = np.where(centre_ok[..., None], sc / sw[..., None], c)
        v2 = np.where(centre_ok, sv / (sw * sw), v)
    assert c2.dtype == f32 and v2.dtype == f32
    return c2, v2


def denoise(S, Q, k, F, width, height, iterations, sigma_c, sigma_n, sigma_p):
    """mirt_denoise: (out float32 [N, 4], stats) -- stats counts the off-centre taps inside the frame of pixels with a finite
    centre that were kept and that a rule skipped, over all iterations."""
    c, v = prepare(S, Q, k)
    c, v = c.reshape(height, width, 4), v.reshape(height, width)
    F = np.asarray(F, f32).reshape(height, width, 8)
    stats = dict(kept=0, skipped=0)
    for i in range(iterations):
        c, v = iteration(c, v, F, 1 << i, sigma_c, sigma_n, sigma_p, stats)
    return c.reshape(-1, 4), stats


def same_bits(a, b):
    """Equal bit patterns, a NaN matching any NaN at the same place (the sign and payload of a NaN an operation produces are the
    processor's choice, not IEEE's)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])

"""numpy float32 restatement of mirt_direct_light, written from the comment in include/mirt_light.h: one operation per line, every
one rounding to float32 once, in the order the header gives.  What the restatement does not decide is which shadow rays are
blocked: the caller brings `occluded[n, L]` (a brute-force test over the scene on the CPU, mirt_trace_rays' any-hit answers on the
GPU) and the expf to use (orc_math_probe on the CPU, mirt_probe_math which = 1 on the GPU, as denoise_ref.py does)."""
import numpy as np

f32 = np.float32
EPSILON = f32(0.001)


def _dot(a, b):
    s = a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    s = s + a[..., 2] * b[..., 2]
    return s


def _length(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):
    """vec3::normalize (vec3.cuh:72-82)."""
    mag = _length(a)
    inv = f32(1.0) / mag
    out = a * inv[..., None]
    out[np.abs(mag) < f32(1e-6)] = 0
    return out


def set_expose(c, expose, expf):
    """setExpose (helper.cu:40-45): the subtraction is in double."""
    expose = f32(expose)
    if expose == f32(np.inf):
        return c
    x = -expose
    x = x * c
    e = expf(x).reshape(c.shape)
    return (1.0 - e.astype(np.float64)).astype(f32)


def shadow_rays(F, suns, bulbs):
    """The MirtRay rows [n, L, 8] the header names, for every row and every light whether it faces the light or not, and
    lam [n, L], tl [n, L] (inf for a sun)."""
    F = np.asarray(F, f32)
    n, L = len(F), len(suns) + len(bulbs)
    P, ng = F[:, 0:3], F[:, 4:7]
    rays = np.zeros((n, L, 8), f32)
    lam = np.zeros((n, L), f32)
    tl = np.full((n, L), np.inf, f32)
    with np.errstate(all="ignore"):
        N = _normalize(ng.copy())
        scaled = ng * EPSILON
        o = P + scaled
        for j in range(len(suns)):
            direction = np.asarray(suns["v"][j], f32)
            Lj = _normalize(direction[None, :].copy())
            lam[:, j] = _dot(N, Lj)
            rays[:, j, 0:3] = o
            rays[:, j, 3] = np.inf
            rays[:, j, 4:7] = direction
        for k in range(len(bulbs)):
            li = len(suns) + k
            bd = np.asarray(bulbs["v"][k], f32)[None, :] - P
            tl[:, li] = _length(bd)
            Lk = _normalize(bd.copy())
            lam[:, li] = _dot(N, Lk)
            rays[:, li, 0:3] = o
            rays[:, li, 3] = tl[:, li]
            rays[:, li, 4:7] = bd
    return rays, lam, tl


def direct_light(F, suns, bulbs, expose, raw, occluded, expf):
    """F float32 [n, 8] feature rows, suns / bulbs LIGHT records (v, color), occluded bool [n, L] -> (out float32 [n, 4],
    mask uint64 [n])."""
    F = np.asarray(F, f32)
    n, L = len(F), len(suns) + len(bulbs)
    occluded = np.asarray(occluded, bool).reshape(n, L)
    hit = F[:, 3] != 0
    _, lam, tl = shadow_rays(F, suns, bulbs)
    acc = np.zeros((n, 3), f32)
    mask = np.zeros(n, np.uint64)
    with np.errstate(all="ignore"):
        for li in range(L):
            is_sun = li < len(suns)
            colour = np.asarray((suns if is_sun else bulbs)["color"][li if is_sun else li - len(suns)], f32)
            facing = lam[:, li] > 0
            lit = hit & facing & ~occluded[:, li]
            c = colour[None, :] * lam[:, li, None]
            e = c if raw else set_expose(c, expose, expf)
            if not is_sun:
                sq = tl[:, li] * tl[:, li]
                i2 = f32(1.0) / sq
                e = e * i2[:, None]
            summed = acc + e
            acc = np.where(lit[:, None], summed, acc)
            mask = np.where(lit, mask | np.uint64(1 << li), mask)
    out = np.zeros((n, 4), f32)
    out[:, 0:3] = acc
    out[:, 3] = 1.0
    out[~hit] = 0
    assert out.dtype == f32 and acc.dtype == f32
    return out, mask

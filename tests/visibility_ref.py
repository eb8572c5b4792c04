"""numpy float32 restatement of mirt_hemisphere_visibility, written from the comment in include/mirt_visibility.h: one operation
per line, every one rounding to float32 once, in the order the header gives.  What the restatement does not decide is which rays
are blocked: the caller brings `occluded[n, K]` (a brute-force test over the scene on the CPU, mirt_trace_rays' any-hit answers on
the GPU)."""
import numpy as np

from light_ref import EPSILON, _dot, _normalize      # noqa: F401  (_dot: the header's dot, for the callers' checks)

f32 = np.float32
ONE = f32(1.0)


def basis(N):
    """(T, B) [n, 3] of unit normals N [n, 3] (Duff et al. 2017), the header's operations."""
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    s = np.copysign(ONE, nz)
    sum_ = s + nz
    a = f32(-1.0) / sum_
    xy = nx * ny
    b = xy * a
    sx = s * nx
    sxx = sx * nx
    sxxa = sxx * a
    tx = ONE + sxxa
    ty = s * b
    ms = -s
    tz = ms * nx
    yy = ny * ny
    yya = yy * a
    by = s + yya
    bz = -ny
    return np.stack([tx, ty, tz], axis=1), np.stack([b, by, bz], axis=1)


def _directions(F, dirs, rot):
    """o [n, 3] and d [n, K, 3] of the header."""
    F = np.asarray(F, f32)
    dirs = np.asarray(dirs, f32).reshape(-1, 4)
    n, K = len(F), len(dirs)
    P, ng = F[:, 0:3], F[:, 4:7]
    with np.errstate(all="ignore"):
        N = _normalize(ng.copy())
        scaled = ng * EPSILON
        o = P + scaled
        T, B = basis(N)
        d = np.zeros((n, K, 3), f32)
        for k in range(K):
            lx, ly, lz = dirs[k, 0], dirs[k, 1], dirs[k, 2]
            if rot is None:
                x = np.full(n, lx, f32)
                y = np.full(n, ly, f32)
            else:
                c, r = np.asarray(rot, f32)[:, 0], np.asarray(rot, f32)[:, 1]
                clx = c * lx
                rly = r * ly
                x = clx - rly
                rlx = r * lx
                cly = c * ly
                y = rlx + cly
            tx = T * x[:, None]
            by = B * y[:, None]
            plane = tx + by
            nz = N * lz
            d[:, k] = plane + nz
    assert o.dtype == f32 and d.dtype == f32
    return o, d


def hemisphere_rays(F, dirs, rot, radius):
    """The MirtRay rows [n, K, 8] the header names, for every row whether it is a hit or not."""
    o, d = _directions(F, dirs, rot)
    n, K = d.shape[0], d.shape[1]
    rays = np.zeros((n, K, 8), f32)
    rays[:, :, 0:3] = o[:, None, :]
    rays[:, :, 3] = f32(radius)
    rays[:, :, 4:7] = d
    return rays


def butterfly(e):
    """The header's sum over axis 1 of e [n, G, C], G a power of two: e_k = e_k + e_(k xor off) for off = G/2, ..., 1; e_0."""
    e = np.array(e, f32)
    G = e.shape[1]
    assert G & (G - 1) == 0
    idx = np.arange(G)
    off = G >> 1
    with np.errstate(all="ignore"):
        while off > 0:
            e = e + e[:, idx ^ off]
            off >>= 1
    assert e.dtype == f32
    return e[:, 0]


def hemisphere_visibility(F, dirs, rot, radius, occluded):
    """F float32 [n, 8] feature rows, dirs [K, 4], rot None or [n, 2], occluded bool [n, K] -> (out float32 [n, 4], mask uint64 [n])."""
    F = np.asarray(F, f32)
    dirs = np.asarray(dirs, f32).reshape(-1, 4)
    n, K = len(F), len(dirs)
    occluded = np.asarray(occluded, bool).reshape(n, K)
    hit = F[:, 3] != 0
    _, d = _directions(F, dirs, rot)
    visible = hit[:, None] & ~occluded
    G = 1
    while G < K:
        G *= 2
    e = np.zeros((n, G, 4), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            w = dirs[k, 3]
            u = _normalize(d[:, k].copy())
            term = np.zeros((n, 4), f32)
            term[:, 0:3] = u * w
            term[:, 3] = w
            e[:, k] = np.where(visible[:, k, None], term, f32(0.0))
    out = butterfly(e)
    mask = (visible.astype(np.uint64) << np.arange(K, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    assert out.dtype == f32
    return out, mask

"""numpy float32 restatement of mirt_indirect_light, written from the comment in include/mirt_indirect.h: one operation per line,
every one rounding to float32 once, in the order the header gives.  Built from the other two restatements, as the header is built
from the other two headers: visibility_ref makes the gather rays and the butterfly, light_ref.direct_light(raw=True) the light at a
hit point.  What the restatement does not decide is what a ray meets: the caller brings `closest(rays) -> (t, kind, id, n)` for the
gather rays (MirtHit's fields, kind 0 for a miss) and `occluded(rays) -> bool` for the shadow rays (a brute-force test over the
scene on the CPU, mirt_trace_rays' answers on the GPU).  Rays are MirtRay rows, float32 [m, 8]."""
import numpy as np

import light_ref
import visibility_ref as vr
from light_ref import _normalize

f32 = np.float32
ONE = f32(1.0)
KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE = 1, 2, 3


def rho(kind, ident, sphere_mats, triangle_mats, plane_mats):
    """The header's diffuse weight ((1 - shininess) * (1 - trans)) * colour of primitive (kind, id), float32 [m, 3]; the material
    tables are float32 [*, 11] in layouts.MAT's order (colour, shininess, trans, ior, roughness).  Rows of kind 0 give zeros."""
    kind = np.asarray(kind).astype(np.int64)
    ident = np.asarray(ident).astype(np.int64)
    out = np.zeros((len(kind), 3), f32)
    for code, table in ((KIND_SPHERE, sphere_mats), (KIND_TRIANGLE, triangle_mats), (KIND_PLANE, plane_mats)):
        sel = kind == code
        if not np.any(sel):
            continue
        mats = np.asarray(table, f32).reshape(-1, 11)[ident[sel]]
        colour, shininess, trans = mats[:, 0:3], mats[:, 3:6], mats[:, 6:9]
        with np.errstate(all="ignore"):
            a = ONE - shininess
            b = ONE - trans
            ab = a * b
            out[sel] = ab * colour
    assert out.dtype == f32
    return out


def hit_points(rays, t):
    """mirt_hit_features' point for rays [m, 8] and distances t [m]: o + t * normalize(d), the product rounded, then the sum."""
    rays = np.asarray(rays, f32)
    with np.errstate(all="ignore"):
        u = _normalize(rays[:, 4:7].copy())
        step = u * np.asarray(t, f32)[:, None]
        P2 = rays[:, 0:3] + step
    assert P2.dtype == f32
    return P2


def gather(F, dirs, hit, weight, D):
    """The header's terms and their sum: F float32 [n, 8] feature rows, dirs [K, 4], and per (row, direction) hit bool [n, K],
    weight = rho float32 [n, K, 3] and D float32 [n, K, 3] -> (out float32 [n, 4], mask uint64 [n])."""
    F = np.asarray(F, f32)
    dirs = np.asarray(dirs, f32).reshape(-1, 4)
    n, K = len(F), len(dirs)
    row_hit = F[:, 3] != 0
    hit = np.asarray(hit, bool).reshape(n, K) & row_hit[:, None]
    weight = np.asarray(weight, f32).reshape(n, K, 3)
    D = np.asarray(D, f32).reshape(n, K, 3)
    G = 1
    while G < K:
        G *= 2
    e = np.zeros((n, G, 4), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            w = dirs[k, 3]
            L = weight[:, k] * D[:, k]
            term = np.zeros((n, 4), f32)
            term[:, 0:3] = L * w
            miss = np.zeros((n, 4), f32)
            miss[:, 3] = w
            e[:, k] = np.where(hit[:, k, None], term, miss)
        e[~row_hit] = 0
    out = vr.butterfly(e)
    mask = (hit.astype(np.uint64) << np.arange(K, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    assert out.dtype == f32
    return out, mask


def indirect_light(F, dirs, rot, radius, suns, bulbs, sphere_mats, triangle_mats, plane_mats, closest, occluded):
    """F float32 [n, 8] feature rows, dirs [K, 4], rot None or [n, 2], suns / bulbs LIGHT records (v, color), the three material
    tables, and the two callbacks -> (out float32 [n, 4], mask uint64 [n])."""
    F = np.asarray(F, f32)
    dirs = np.asarray(dirs, f32).reshape(-1, 4)
    n, K = len(F), len(dirs)
    nl = len(suns) + len(bulbs)
    rays = vr.hemisphere_rays(F, dirs, rot, radius).reshape(n * K, 8)
    t, kind, ident, n2 = closest(rays)
    kind = np.asarray(kind).reshape(-1)
    hit = kind != 0
    # the row (P2, 1) (n2, _) of every gather ray that hit; a row of zeros, which direct_light answers with zeros, for the others
    rows = np.zeros((n * K, 8), f32)
    rows[:, 0:3] = hit_points(rays, t)
    rows[:, 3] = 1
    rows[:, 4:7] = np.asarray(n2, f32).reshape(-1, 3)
    rows[~hit] = 0
    if nl:
        shadow, _, _ = light_ref.shadow_rays(rows, suns, bulbs)
        occ = np.asarray(occluded(shadow.reshape(-1, 8)), bool).reshape(n * K, nl)
    else:
        occ = np.zeros((n * K, 0), bool)
    D, _ = light_ref.direct_light(rows, suns, bulbs, np.inf, True, occ, None)
    weight = rho(kind, ident, sphere_mats, triangle_mats, plane_mats)
    return gather(F, dirs, hit.reshape(n, K), weight.reshape(n, K, 3), D[:, 0:3].reshape(n, K, 3))

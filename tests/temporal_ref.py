"""numpy float32 restatement of mirt_prev_features and mirt_temporal_accumulate, written from the comments in include/mirt.h: every
operation rounds to float32 once, in the order the header gives.  normalize is the one test_gpu_queries.py restates from
vec3.cuh (the one denoise_ref.py uses)."""
import numpy as np

from test_gpu_queries import _normalize

f32 = np.float32
HIT_NONE, HIT_SPHERE, HIT_TRIANGLE, HIT_PLANE = 0, 1, 2, 3


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _length(a):
    return np.sqrt(_dot(a, a))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _finite3(c):
    return np.all(np.isfinite(c[..., :3]), axis=-1)


def triangle_records(verts):
    """The scene's 48-byte triangle records from vertices [n, 9] (object.cuh:177-191, as mirt_scene_update_triangles computes
    them): (p0, nor, e1, e2), each [n, 3]."""
    v = np.asarray(verts, f32).reshape(-1, 9)
    p0, p1, p2 = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    with np.errstate(all="ignore"):
        d1, d2 = p1 - p0, p2 - p0
        nor = _normalize(_cross(d1, d2))
        a1, a2 = _cross(d2, nor), _cross(d1, nor)
        k1, k2 = f32(1) / _dot(a1, d1), f32(1) / _dot(a2, d2)
        return p0, nor, a1 * k1[:, None], a2 * k2[:, None]


def prev_features(rays, hits, spheres, tri_verts, prev_xyzr, prev_verts):
    """rays float32 [n, 8], hits [n, 6] 4-byte words, spheres [Ns, 4] and tri_verts [Nt, 9]: the scene as it is; prev_xyzr [Ns, 4]
    and prev_verts [Nt, 9] (or None): the scene as it was -> float32 [n, 8]."""
    rays = np.ascontiguousarray(rays, dtype=f32).reshape(-1, 8)
    words = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 6)
    n = len(rays)
    t = words[:, 0].copy().view(f32)
    nrm = words[:, 3:6].copy().view(f32)
    kind, ident = words[:, 1].astype(np.int64), words[:, 2].astype(np.int64)
    out = np.zeros((n, 8), f32)
    with np.errstate(all="ignore"):
        d = _normalize(rays[:, 4:7].copy())
        P = rays[:, 0:3] + t[:, None] * d
        out[:, 0:3] = P
        out[:, 3] = 1.0
        out[:, 4:7] = nrm
        if prev_xyzr is not None:
            spheres, prev_xyzr = np.asarray(spheres, f32).reshape(-1, 4), np.asarray(prev_xyzr, f32).reshape(-1, 4)
            sel = kind == HIT_SPHERE
            bad = sel & (ident >= len(spheres))
            ok = np.nonzero(sel & ~bad)[0]
            s, sp = spheres[ident[ok]], prev_xyzr[ident[ok]]
            u = (P[ok] - s[:, 0:3]) / s[:, 3:4]
            out[ok, 0:3] = sp[:, 0:3] + u * sp[:, 3:4]
            out[bad] = 0
        if prev_verts is not None:
            prev_verts = np.asarray(prev_verts, f32).reshape(-1, 9)
            p0, nor, e1, e2 = triangle_records(tri_verts)
            sel = kind == HIT_TRIANGLE
            bad = sel & (ident >= len(p0))
            ok = np.nonzero(sel & ~bad)[0]
            i = ident[ok]
            v = P[ok] - p0[i]
            b1, b2 = _dot(e1[i], v), _dot(e2[i], v)
            q0, q1, q2 = prev_verts[i, 0:3], prev_verts[i, 3:6], prev_verts[i, 6:9]
            d1, d2 = q1 - q0, q2 - q0
            out[ok, 0:3] = (q0 + b1[:, None] * d1) + b2[:, None] * d2
            m = _normalize(_cross(d1, d2))
            flip = _dot(nrm[ok], nor[i]) < 0
            out[ok, 4:7] = np.where(flip[:, None], -m, m)
            out[bad] = 0
    out[kind == HIT_NONE] = 0
    return out


def _split_axis(x, size):
    """(finite, first tap's coordinate, second tap's weight) of a position after the snap."""
    r = np.rint(x)
    x = np.where(np.abs(x - r) <= f32(1.0 / 1024.0), r, x)
    fl = np.floor(x)
    finite = np.isfinite(x)
    first = np.where(finite, np.clip(fl, -2.0 ** 31, 2.0 ** 31), 0).astype(np.int64)      # (far outside stays outside)
    return finite, first, (x - fl).astype(f32)


def temporal_accumulate(S, Q, k, G, hS, hQ, hk, hF, camera, width, height, max_history, sigma_n, sigma_p):
    """camera: (eye, forward, right, up), each three numbers.  Returns (out S [N, 4] float32, out Q, out k uint32 [N], stats) --
    stats counts the taps inside the frame with a non-zero weight that were valid and that step 4 rejected, the pixels that took
    history, the pixels whose history was one tap as it is, the pixels whose history was capped, and -- `outside`: left, right,
    top, bottom -- the taps with a non-zero weight that were dropped for lying beyond that border of the frame."""
    N = width * height
    S, Q = np.asarray(S, f32).reshape(N, 4), np.asarray(Q, f32).reshape(N, 4)
    hS, hQ = np.asarray(hS, f32).reshape(N, 4), np.asarray(hQ, f32).reshape(N, 4)
    k, hk = np.asarray(k).astype(np.uint32).reshape(N), np.asarray(hk).astype(np.uint32).reshape(N)
    G, hF = np.asarray(G, f32).reshape(N, 8), np.asarray(hF, f32).reshape(N, 8)
    eye, fw, rt, up = (np.asarray(v, f32).reshape(1, 3) for v in camera)
    sigma_n, sigma_p = f32(sigma_n), f32(sigma_p)
    W, H = width, height
    max_dim = f32(max(W, H))
    stats = dict(valid=0, rejected=0, merged=0, exact=0, capped=0, outside=[0, 0, 0, 0])
    with np.errstate(all="ignore"):
        P, nP = G[:, 0:3], G[:, 4:7]
        v = P - eye
        f = _dot(v, fw) / _dot(fw, fw)
        go = (G[:, 3] != 0) & np.isfinite(f) & (f > 0)
        sx = _dot(v, rt) / _dot(rt, rt) / f
        sy = _dot(v, up) / _dot(up, up) / f
        fx = (sx * max_dim + f32(W)) / f32(2)
        fy = (f32(H) - sy * max_dim) / f32(2)
        in_x, x0, tx = _split_axis(fx, W)
        in_y, y0, ty = _split_axis(fy, H)
        go &= in_x & in_y
        foot = _length(v) * f32(2) / max_dim
        wx, wy = (f32(1) - tx, tx), (f32(1) - ty, ty)
        taps = []
        sw = np.zeros(N, f32)
        kmin = np.full(N, 0xffffffff, np.uint32)
        exact = np.full(N, -1)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                w = (wx[i] * wy[j]).astype(f32)
                live = go & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (w != 0)
                for side, beyond in enumerate((qx < 0, qx >= W, qy < 0, qy >= H)):
                    stats["outside"][side] += int(np.count_nonzero(go & (w != 0) & beyond))
                q = np.where(live, qy * W + qx, 0)
                kq, Sq, Qq, Fq = hk[q], hS[q], hQ[q], hF[q]
                c = f32(1) - _dot(nP, Fq[:, 4:7])
                a_n = np.where(c < 0, f32(0), c) / sigma_n
                D = Fq[:, 0:3] - P
                a_p = np.abs(_dot(nP, D)) / (sigma_p * np.fmax(_length(D), foot))
                geometry = (a_n + a_p) <= f32(1)
                valid = live & (kq > 0) & _finite3(Sq) & _finite3(Qq) & (Fq[:, 3] != 0) & geometry
                stats["valid"] += int(np.count_nonzero(valid))
                stats["rejected"] += int(np.count_nonzero(live & (kq > 0) & _finite3(Sq) & _finite3(Qq) & (Fq[:, 3] != 0) & ~geometry))
                sw = np.where(valid, sw + w, sw)
                kmin = np.where(valid & (kq < kmin), kq, kmin)
                exact = np.where(valid & (w == 1), len(taps), exact)
                taps.append((valid, w, kq, Sq, Qq))
        have = sw != 0
        m, s = np.zeros((N, 4), f32), np.zeros((N, 4), f32)
        Sh, Qh, kh = np.zeros((N, 4), f32), np.zeros((N, 4), f32), np.zeros(N, np.uint32)
        for t, (valid, w, kq, Sq, Qq) in enumerate(taps):
            wn = (w / sw)[:, None]
            kf = kq.astype(f32)[:, None]
            m = np.where(valid[:, None], m + wn * (Sq / kf), m)
            s = np.where(valid[:, None], s + wn * (Qq / kf), s)
            one = exact == t
            Sh, Qh, kh = np.where(one[:, None], Sq, Sh), np.where(one[:, None], Qq, Qh), np.where(one, kq, kh)
        blend = have & (exact < 0)
        kf = kmin.astype(f32)[:, None]
        Sh, Qh, kh = np.where(blend[:, None], m * kf, Sh), np.where(blend[:, None], s * kf, Qh), np.where(blend, kmin, kh)
        over = have & (kh > np.uint32(max_history))
        c = (f32(max_history) / kh.astype(f32))[:, None]
        Sh, Qh, kh = np.where(over[:, None], Sh * c, Sh), np.where(over[:, None], Qh * c, Qh), np.where(over, np.uint32(max_history), kh)
        oS = np.where(have[:, None], S + Sh, S)
        oQ = np.where(have[:, None], Q + Qh, Q)
        ok = np.where(have, k + kh, k).astype(np.uint32)
    stats.update(merged=int(np.count_nonzero(have)), exact=int(np.count_nonzero(have & (exact >= 0))), capped=int(np.count_nonzero(over)))
    assert oS.dtype == f32 and oQ.dtype == f32
    return oS, oQ, ok, stats


def same_bits(a, b):
    """Equal bit patterns, a NaN matching any NaN at the same place."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])

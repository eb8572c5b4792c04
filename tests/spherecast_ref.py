"""include_ext/mirt_spherecast.h restated in numpy float32, one operation per line: every candidate's parameter t for every row (a
brute force over the scene's arrays), the (t, kind, id) choice, and the winner's record.  Then the header's pruning rule as a walk
over a tree given as arrays (oracle_lib.OracleScene.nodes() / refs()), which must give the brute force's answer whatever the tree.

Scenes are pyscene.PyScene.arrays() dictionaries (spheres, triangles, planes in file order).  Rows are float32 [n, 8]:
(ox, oy, oz, tmax) (dx, dy, dz, r).  The vector operations and the closest point of a triangle are closest_ref's: the header adopts
mirt_closest.h's."""
import numpy as np

import closest_ref as cr
from closest_ref import KIND_PLANE, KIND_SPHERE, KIND_TRIANGLE, _dot, _length, _normalize, _scale

f32 = np.float32
u32 = np.uint32
SLACK = f32(2.0 ** -18)      # sigma = SLACK * ((max |o| + C) + r)
TAU = f32(2.0 ** -20)        # bound = best + best * TAU
NAN = f32(np.nan)
INF = f32(np.inf)
ZERO = f32(0.0)


# ---- the row rule ---------------------------------------------------------------------------------------------------------------------
def directions(rows):
    """d^ = normalize(d) of every row."""
    return _normalize(np.ascontiguousarray(rows[:, 4:7], f32))


def live_rows(rows):
    with np.errstate(all="ignore"):
        d = directions(rows)
        dsum = np.abs(d[:, 0]) + np.abs(d[:, 1])
        dsum = dsum + np.abs(d[:, 2])
        tmax, r = rows[:, 3], rows[:, 7]
        return (tmax > 0) & (r >= 0) & np.isfinite(r) & np.all(np.isfinite(rows[:, 0:3]), axis=1) & (dsum > 0)


def centre(o, d, t):
    """C(t) = o + d^ * t: the product rounded, then the sum."""
    return o + _scale(d, t)


# ---- the helpers: the centre ray (o, d^) against the ball (p, R), closest-approach form -------------------------------------------------
def _approach(p, R, o, d):
    m = p - o
    a = _dot(m, d)
    da = _scale(d, a)
    w = m - da
    ww = _dot(w, w)
    RR = R * R
    h2 = RR - ww
    return a, h2


def entry(p, R, o, d):
    a, h2 = _approach(p, R, o, d)
    s = np.sqrt(h2)
    t = a - s
    return np.where(h2 >= 0, t, NAN)


def exit_(p, R, o, d):
    a, h2 = _approach(p, R, o, d)
    h2 = np.where(h2 < 0, ZERO, h2)
    s = np.sqrt(h2)
    return a + s


# ---- the three kinds of candidates: t (NaN or +inf: none), each broadcast over o, d [..., 3] and r [...] ----------------------------------
def sphere_t(o, d, r, c, rs):
    v = o - c
    l = _length(v)
    g = l - rs
    t_in = entry(c, rs + r, o, d)
    t_out = exit_(c, rs - r, o, d)
    t = np.where(g > 0, t_in, t_out)
    return np.where(np.abs(g) <= r, ZERO, t)


def plane_rule(o, d, r, N, point):
    """The plane rule for a unit normal N (a plane's normalize(nor); a triangle's nor)."""
    v = o - point
    s = _dot(N, v)
    dn = _dot(N, d)
    t_above = r - s
    t_above = t_above / dn
    t_below = (-r) - s
    t_below = t_below / dn
    t = np.where((s > 0) & (dn < 0), t_above, np.where((s < 0) & (dn > 0), t_below, NAN))
    return np.where(np.abs(s) <= r, ZERO, t)


def plane_t(o, d, r, nor, point):
    return plane_rule(o, d, r, _normalize(nor), point)


def in_face_region(q, a, b, c):
    """mirt_closest.h's region walk for q falls through to its last case: none of the six vertex and edge regions matches."""
    ab = b - a
    ac = c - a
    ap = q - a
    d1 = _dot(ab, ap)
    d2 = _dot(ac, ap)
    in_a = (d1 <= 0) & (d2 <= 0)
    bp = q - b
    d3 = _dot(ab, bp)
    d4 = _dot(ac, bp)
    in_b = (d3 >= 0) & (d4 <= d3)
    vc1 = d1 * d4
    vc2 = d3 * d2
    vc = vc1 - vc2
    in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    cp = q - c
    d5 = _dot(ab, cp)
    d6 = _dot(ac, cp)
    in_c = (d6 >= 0) & (d5 <= d6)
    vb1 = d5 * d2
    vb2 = d1 * d6
    vb = vb1 - vb2
    in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    va1 = d3 * d6
    va2 = d5 * d4
    va = va1 - va2
    e = d4 - d3
    f = d5 - d6
    in_bc = (va <= 0) & (e >= 0) & (f >= 0)
    return ~(in_a | in_b | in_ab | in_c | in_ac | in_bc)


def edge_t(o, d, r, p, q):
    e = q - p
    ee = _dot(e, e)
    m = o - p
    u = _dot(m, e) / ee
    k = _dot(d, e) / ee
    mp = m - _scale(e, u)
    dp = d - _scale(e, k)
    A = _dot(dp, dp)
    t0 = (-_dot(mp, dp)) / A
    wv = mp + _scale(dp, t0)
    rr = r * r
    h2 = rr - _dot(wv, wv)
    s = h2 / A
    s = np.sqrt(s)
    t = t0 - s
    tk = t * k
    at = u + tk
    valid = (ee != 0) & (A != 0) & (h2 >= 0) & (at >= 0) & (at <= 1)
    return np.where(valid, t, NAN)


def triangle_t(o, d, r, a, b, c, nor):
    P0 = cr.triangle_point(o, a, b, c)
    l0 = _length(o - P0)
    tf = plane_rule(o, d, r, nor, a)
    Cf = centre(o, d, tf)
    has_plane = _dot(nor, nor) > 0                         # (a record normal of (0, 0, 0) names no plane: no face piece)
    pieces = [np.where(has_plane & in_face_region(Cf, a, b, c), tf, NAN), entry(a, r, o, d), entry(b, r, o, d), entry(c, r, o, d),
              edge_t(o, d, r, a, b), edge_t(o, d, r, a, c), edge_t(o, d, r, b, c)]
    t = np.broadcast_to(INF, l0.shape).copy()
    for piece in pieces:                                   # (the smallest piece with t >= 0; a NaN never counts; +inf: none)
        t = np.where((piece >= 0) & (piece < t), piece, t)
    t = np.where(l0 <= r, ZERO, t)
    assert t.dtype == f32
    return t


def candidates(arrays, rows):
    """t of every candidate for every row: (spheres [n, Ns], triangles [n, Nt], planes [n, Np]), float32 (NaN or +inf: none)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    o = rows[:, None, 0:3]
    r = rows[:, None, 7]
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    with np.errstate(all="ignore"):
        d = directions(rows)[:, None, :]
        ts = sphere_t(o, d, r, S["c"][None], S["r"][None]) if len(S) else np.zeros((n, 0), f32)
        tt = triangle_t(o, d, r, T["p0"][None], T["p1"][None], T["p2"][None], T["nor"][None]) if len(T) else np.zeros((n, 0), f32)
        tp = plane_t(o, d, r, Pl["nor"][None], Pl["point"][None]) if len(Pl) else np.zeros((n, 0), f32)
    for t in (ts, tt, tp):
        assert t.dtype == f32 and t.shape[0] == n
    return ts, tt, tp


def admitted(t, rows):
    """0 <= t < tmax (a NaN never)."""
    with np.errstate(all="ignore"):
        return (t >= 0) & (t < rows[:, 3:4])


# ---- the winner's record ----------------------------------------------------------------------------------------------------------------
def records(arrays, rows, t, kind, pid):
    """MirtHit words [n, 6] (uint32) and feature rows [n, 8] (float32) of the named candidates at their t (kind 0: a miss)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    hits = np.zeros((n, 6), u32)
    feat = np.zeros((n, 8), f32)
    hits[:, 0] = f32(-1.0).view(u32)
    o = np.ascontiguousarray(rows[:, 0:3])
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    with np.errstate(all="ignore"):
        d = directions(rows)
        for k in (KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE):
            sel = np.flatnonzero(kind == k)
            if not len(sel):
                continue
            j = pid[sel]
            tw = np.ascontiguousarray(t[sel], f32)
            Cw = centre(o[sel], d[sel], tw)
            if k == KIND_SPHERE:
                v = Cw - S["c"][j]
                u = _normalize(v)
                P = S["c"][j] + _scale(u, S["r"][j])
            elif k == KIND_TRIANGLE:
                P = cr.triangle_point(Cw, T["p0"][j], T["p1"][j], T["p2"][j])
            else:
                N = _normalize(Pl["nor"][j])
                s = _dot(N, Cw - Pl["point"][j])
                P = Cw - _scale(N, s)
            nn = _normalize(Cw - P)
            assert P.dtype == f32 and nn.dtype == f32
            hits[sel, 0] = tw.view(u32)
            hits[sel, 1] = k
            hits[sel, 2] = j
            hits[sel, 3:6] = np.ascontiguousarray(nn, f32).view(u32)
            feat[sel, 0:3] = P
            feat[sel, 3] = 1
            feat[sel, 4:7] = nn
    return hits, feat


def brute_force(arrays, rows, cands=None):
    """(hits uint32 [n, 6], features float32 [n, 8]): the admitted candidate with the smallest (t, kind, id) of every row."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = live_rows(rows)
    best = np.full(n, np.inf, f32)
    kind = np.zeros(n, np.int64)
    pid = np.zeros(n, np.int64)
    for k, t in zip((KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE), cands or candidates(arrays, rows)):      # (ascending kind: a tie keeps the earlier)
        if not t.shape[1]:
            continue
        t = np.where(admitted(t, rows), t, INF)
        j = np.argmin(t, axis=1)                           # (the first of equal minima: the lowest id)
        tj = t[np.arange(n), j]
        take = live & (tj < best)
        best = np.where(take, tj, best)
        kind = np.where(take, k, kind)
        pid = np.where(take, j, pid)
    return records(arrays, rows, best, kind, pid)


def any_hit_is_valid(arrays, rows, hits, feat, cands=None):
    """MIRT_CAST_ANY_HIT's contract: kind != 0 exactly where the closest-hit answer's is, and every record is the restatement's
    record of the admitted candidate it names.  Returns the indices of the rows that break it."""
    rows = np.ascontiguousarray(rows, f32)
    cands = cands or candidates(arrays, rows)
    want_hits, _ = brute_force(arrays, rows, cands)
    kind, pid = hits[:, 1].astype(np.int64), hits[:, 2].astype(np.int64)
    bad = (kind != 0) != (want_hits[:, 1] != 0)
    t = np.full(len(rows), -1.0, f32)
    for k, tk in zip((KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE), cands):
        sel = np.flatnonzero(kind == k)
        if not len(sel):
            continue
        inside = pid[sel] < tk.shape[1]
        bad[sel[~inside]] = True
        sel = sel[inside]
        t[sel] = tk[sel, pid[sel]]
        bad[sel] |= ~admitted(tk, rows)[sel, pid[sel]]
    kind = np.where(bad, 0, kind)
    own_hits, own_feat = records(arrays, rows, t, kind, pid)
    bad |= np.any(own_hits != hits, axis=1) | np.any(own_feat.view(u32) != feat.view(u32), axis=1)
    return np.flatnonzero(bad)


# ---- the pruning rule as a walk -------------------------------------------------------------------------------------------------------
def slab_intervals(nodes, o, d, grow):
    """(enter, leave) [n, nodes] of the centre ray against every node's box grown by `grow` [n], the kernel's operations: per axis
    t0 = ((min - grow) - o) * inv, t1 = ((max + grow) - o) * inv, inv = 1 / d^; the latest of the three nearer and the earliest of
    the three farther ones, fmin / fmax dropping a NaN (0 * inf: the centre on a face of a slab it runs along)."""
    inv = f32(1.0) / d
    near, far = [], []
    for lo, hi, k in (("xmin", "xmax", 0), ("ymin", "ymax", 1), ("zmin", "zmax", 2)):
        a = nodes[lo][None, :] - grow[:, None]
        b = nodes[hi][None, :] + grow[:, None]
        t0 = (a - o[:, k:k + 1]) * inv[:, k:k + 1]
        t1 = (b - o[:, k:k + 1]) * inv[:, k:k + 1]
        near.append(np.fmin(t0, t1))
        far.append(np.fmax(t0, t1))
    enter = np.fmax(np.fmax(np.fmax(near[0], near[1]), near[2]), ZERO)
    leave = np.fmin(np.fmin(far[0], far[1]), far[2])
    assert enter.dtype == f32 and leave.dtype == f32
    return enter, leave


def pruned_walk(arrays, rows, nodes, refs, slack=SLACK, tau=TAU, near_first=True, any_hit=False):
    """The header's rule over the tree `nodes` (oracle_lib.NODE: internal nodes first, node 0 the root, leaves with count 1 whose
    prim_offset indexes `refs`, the sorted (type, id) pairs): the planes, then a stack walk that leaves a subtree out only when
    the centre ray misses its box grown by r + sigma within [0, best + best * tau], sigma = slack * ((max |o| + C) + r), C the
    largest coordinate magnitude of the root's box.  Returns (hits, features, leaves visited per row)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = live_rows(rows)
    cands = candidates(arrays, rows)
    ts, tt, tp = cands
    ok_s, ok_t, ok_p = (admitted(t, rows) for t in cands)
    o = np.ascontiguousarray(rows[:, 0:3])
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        d = directions(rows)
        omax = np.fmax(np.fmax(np.abs(o[:, 0]), np.abs(o[:, 1])), np.abs(o[:, 2]))
        sigma = ((omax + C) + rows[:, 7]) * f32(slack)
        grow = rows[:, 7] + sigma
        assert sigma.dtype == f32 and grow.dtype == f32
        if len(nodes):
            enter, leave = slab_intervals(nodes, o, d, grow)
            enter, leave = enter.tolist(), leave.tolist()
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))
    rtype, rid = refs["type"].tolist(), refs["id"].tolist()
    best = np.full(n, np.inf, f32)
    kind = np.zeros(n, np.int64)
    pid = np.zeros(n, np.int64)
    visited = np.zeros(n, np.int64)
    tau = f32(tau)

    def bound_of(b):
        with np.errstate(all="ignore"):
            return float(f32(b + f32(b * tau)))

    for i in np.flatnonzero(live):
        b, bk, bj = rows[i, 3], 0, 0
        for j in range(tp.shape[1]):
            if ok_p[i, j] and tp[i, j] < b:
                b, bk, bj = tp[i, j], KIND_PLANE, j
        if len(nodes) and not (any_hit and bk):
            row_enter, row_leave = enter[i], leave[i]
            bound = bound_of(b)
            stack, cur = [], 0
            while True:
                if count[cur] > 0:
                    visited[i] += 1
                    tri = rtype[off[cur]]
                    k = KIND_TRIANGLE if tri else KIND_SPHERE
                    j = rid[off[cur]]
                    t = tt[i, j] if tri else ts[i, j]
                    ok = ok_t[i, j] if tri else ok_s[i, j]
                    if ok and (t < b or (t == b and bk != 0 and (k, j) < (bk, bj))):
                        b, bk, bj = t, k, j
                        bound = bound_of(b)
                        if any_hit:
                            break
                    pop = True
                else:
                    l, r = left[cur], right[cur]
                    hl = not (row_enter[l] > (row_leave[l] if row_leave[l] < bound else bound))      # (fmin: a NaN is dropped)
                    hr = not (row_enter[r] > (row_leave[r] if row_leave[r] < bound else bound))
                    first, second = (r, l) if (near_first and row_enter[r] < row_enter[l]) else (l, r)
                    if hl and hr:
                        stack.append(second)
                        cur = first
                    else:
                        cur = l if hl else r
                    pop = not (hl or hr)
                if pop:
                    if not stack:
                        break
                    cur = stack.pop()
        if bk:
            best[i], kind[i], pid[i] = b, bk, bj
    hits, feat = records(arrays, rows, best, kind, pid)
    return hits, feat, visited

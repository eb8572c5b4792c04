"""include/mirt_closest.h restated in numpy float32, one operation per line: every candidate's distance for every row (a brute
force over the scene's arrays), the (dist, kind, id) choice, and the winner's record.  Then the header's pruning rule as a walk over
a tree given as arrays (oracle_lib.OracleScene.nodes() / refs()), which must give the brute force's answer whatever the tree.

Scenes are pyscene.PyScene.arrays() dictionaries (spheres, triangles, planes in file order).  Rows are float32 [n, 4]: (q, R)."""
import numpy as np

f32 = np.float32
u32 = np.uint32
SLACK = f32(2.0 ** -18)
KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE = 1, 2, 3


# ---- the header's vector operations on arrays [..., 3] ------------------------------------------------------------------------
def _dot(a, b):
    x = a[..., 0] * b[..., 0]
    y = a[..., 1] * b[..., 1]
    z = a[..., 2] * b[..., 2]
    s = x + y
    return s + z


def _length(v):
    return np.sqrt(_dot(v, v))


def _scale(v, s):
    return v * s[..., None]


def _normalize(v):
    mag = _length(v)
    inv = f32(1.0) / mag
    out = _scale(v, inv)
    return np.where((np.abs(mag) < f32(1e-6))[..., None], f32(0.0), out)


def _assert_f32(*arrays):
    for a in arrays:
        assert a.dtype == f32, a.dtype


# ---- the three kinds of candidates: (dist, P, n), each broadcast over q [..., 3] -----------------------------------------------
def plane_candidate(q, nor, point):
    N = _normalize(nor)
    d = q - point
    s = _dot(N, d)
    dist = np.abs(s)
    Ns = _scale(N, s)
    P = q - Ns
    n = np.where((s < 0)[..., None], -N, N)
    _assert_f32(dist, P, n)
    return dist, P, n


def sphere_distance(q, c, r):
    v = q - c
    l = _length(v)
    t = l - r
    return np.abs(t)


def sphere_candidate(q, c, r):
    v = q - c
    l = _length(v)
    t = l - r
    dist = np.abs(t)
    u = _normalize(v)
    ur = _scale(u, r)
    P = c + ur
    n = np.where((l < r)[..., None], -u, u)
    _assert_f32(dist, P, n)
    return dist, P, n


def triangle_point(q, a, b, c):
    """The closest point by Voronoi region, the first region that matches winning: every region's point is computed for every
    row and the first match picked."""
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
    t_ab = d1 - d3
    t_ab = d1 / t_ab
    P_ab = a + _scale(ab, t_ab)
    cp = q - c
    d5 = _dot(ab, cp)
    d6 = _dot(ac, cp)
    in_c = (d6 >= 0) & (d5 <= d6)
    vb1 = d5 * d2
    vb2 = d1 * d6
    vb = vb1 - vb2
    in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    t_ac = d2 - d6
    t_ac = d2 / t_ac
    P_ac = a + _scale(ac, t_ac)
    va1 = d3 * d6
    va2 = d5 * d4
    va = va1 - va2
    e = d4 - d3
    f = d5 - d6
    in_bc = (va <= 0) & (e >= 0) & (f >= 0)
    t_bc = e + f
    t_bc = e / t_bc
    bc = c - b
    P_bc = b + _scale(bc, t_bc)
    den = va + vb
    den = den + vc
    den = f32(1.0) / den
    v = vb * den
    w = vc * den
    P_in = a + _scale(ab, v)
    P_in = P_in + _scale(ac, w)
    shape = np.broadcast(P_in, q).shape
    P = np.broadcast_to(P_in, shape).copy()
    for cond, val in ((in_bc, P_bc), (in_ac, P_ac), (in_c, c), (in_ab, P_ab), (in_b, b), (in_a, a)):      # (last assigned = first in the header)
        P = np.where(cond[..., None], np.broadcast_to(val, shape), P)
    _assert_f32(P)
    return P


def triangle_candidate(q, a, b, c, nor):
    P = triangle_point(q, a, b, c)
    w = q - P
    dist = _length(w)
    n = np.where((_dot(w, nor) < 0)[..., None], -nor, nor)
    _assert_f32(dist, P, n)
    return dist, P, np.broadcast_to(n, P.shape)


# ---- all candidates of a scene --------------------------------------------------------------------------------------------------
def live_rows(rows):
    with np.errstate(all="ignore"):
        return (rows[:, 3] > 0) & np.all(np.isfinite(rows[:, 0:3]), axis=1)


def distances(arrays, rows):
    """dist of every candidate for every row: (spheres [n, Ns], triangles [n, Nt], planes [n, Np]), float32."""
    rows = np.ascontiguousarray(rows, f32)
    q = rows[:, None, 0:3]
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    with np.errstate(all="ignore"):
        ds = sphere_distance(q, S["c"][None], S["r"][None]) if len(S) else np.zeros((len(rows), 0), f32)
        dt = triangle_candidate(q, T["p0"][None], T["p1"][None], T["p2"][None], T["nor"][None])[0] if len(T) else np.zeros((len(rows), 0), f32)
        dp = plane_candidate(q, Pl["nor"][None], Pl["point"][None])[0] if len(Pl) else np.zeros((len(rows), 0), f32)
    return ds, dt, dp


def _records(arrays, rows, dist, kind, pid):
    """MirtHit words [n, 6] (uint32) and feature rows [n, 8] (float32) of the winners (kind 0: a miss)."""
    n = len(rows)
    hits = np.zeros((n, 6), u32)
    feat = np.zeros((n, 8), f32)
    hits[:, 0] = f32(-1.0).view(u32)
    q = np.ascontiguousarray(rows[:, 0:3], f32)
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    with np.errstate(all="ignore"):
        for k in (KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE):
            sel = np.flatnonzero(kind == k)
            if not len(sel):
                continue
            j = pid[sel]
            if k == KIND_SPHERE:
                d, P, nn = sphere_candidate(q[sel], S["c"][j], S["r"][j])
            elif k == KIND_TRIANGLE:
                d, P, nn = triangle_candidate(q[sel], T["p0"][j], T["p1"][j], T["p2"][j], T["nor"][j])
            else:
                d, P, nn = plane_candidate(q[sel], Pl["nor"][j], Pl["point"][j])
            assert np.array_equal(d.view(u32), dist[sel].view(u32))
            hits[sel, 0] = d.view(u32)
            hits[sel, 1] = k
            hits[sel, 2] = j
            hits[sel, 3:6] = np.ascontiguousarray(nn, f32).view(u32)
            feat[sel, 0:3] = P
            feat[sel, 3] = 1
            feat[sel, 4:7] = nn
    return hits, feat


def brute_force(arrays, rows):
    """(hits uint32 [n, 6], features float32 [n, 8]): the admitted candidate with the smallest (dist, kind, id) of every row."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = live_rows(rows)
    R = rows[:, 3]
    best = np.full(n, np.inf, f32)
    kind = np.zeros(n, np.int64)
    pid = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for k, d in zip((KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE), distances(arrays, rows)):      # (ascending kind: a tie keeps the earlier)
            if not d.shape[1]:
                continue
            d = np.where(d < R[:, None], d, f32(np.inf))      # (admitted: dist < R; NaN never)
            j = np.argmin(d, axis=1)                           # (the first of equal minima: the lowest id)
            dj = d[np.arange(n), j]
            take = live & (dj < best)
            best = np.where(take, dj, best)
            kind = np.where(take, k, kind)
            pid = np.where(take, j, pid)
    return _records(arrays, rows, best, kind, pid)


# ---- the pruning rule as a walk -----------------------------------------------------------------------------------------------------
def box_distance2(nodes, q):
    """Squared point-box distance [n, nodes], the kernel's operations: per axis max(max(min - q, q - max), 0), then the squared sum."""
    e = []
    for lo, hi, k in (("xmin", "xmax", 0), ("ymin", "ymax", 1), ("zmin", "zmax", 2)):
        a = nodes[lo][None, :] - q[:, k:k + 1]
        b = q[:, k:k + 1] - nodes[hi][None, :]
        e.append(np.fmax(np.fmax(a, b), f32(0.0)))
    s = e[0] * e[0] + e[1] * e[1]
    return s + e[2] * e[2]


def pruned_walk(arrays, rows, nodes, refs, slack=SLACK, near_first=True):
    """The header's rule over the tree `nodes` (oracle_lib.NODE: internal nodes first, node 0 the root, leaves with count 1 whose
    prim_offset indexes `refs`, the sorted (type, id) pairs): the planes, then a stack walk that leaves a subtree out only when
    its squared box distance exceeds (best + sigma)^2, sigma = slack * (max |q| + C), C the largest coordinate magnitude of the
    root's box.  Returns (hits, features, leaves visited per row)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = live_rows(rows)
    ds, dt, dp = distances(arrays, rows)
    q = np.ascontiguousarray(rows[:, 0:3], f32)
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        lb2 = box_distance2(nodes, q).tolist() if len(nodes) else None
        qmax = np.fmax(np.fmax(np.abs(q[:, 0]), np.abs(q[:, 1])), np.abs(q[:, 2]))
        sigma = (qmax + C) * f32(slack)
    assert sigma.dtype == f32
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))
    rtype, rid = refs["type"].tolist(), refs["id"].tolist()
    best = np.full(n, np.inf, f32)
    kind = np.zeros(n, np.int64)
    pid = np.zeros(n, np.int64)
    visited = np.zeros(n, np.int64)
    for i in np.flatnonzero(live):
        b, bk, bj = rows[i, 3], 0, 0
        for j in range(dp.shape[1]):
            if dp[i, j] < b:
                b, bk, bj = dp[i, j], KIND_PLANE, j
        if len(nodes):
            row_lb2 = lb2[i]
            dsi, dti = ds[i], dt[i]
            with np.errstate(all="ignore"):
                reach = f32(b + sigma[i])
                bound2 = float(f32(reach * reach))
            stack, cur = [], 0
            while True:
                if count[cur] > 0:
                    visited[i] += 1
                    k = KIND_TRIANGLE if rtype[off[cur]] else KIND_SPHERE
                    j = rid[off[cur]]
                    d = dti[j] if rtype[off[cur]] else dsi[j]
                    if d < b or (d == b and bk != 0 and (k, j) < (bk, bj)):
                        b, bk, bj = d, k, j
                        with np.errstate(all="ignore"):
                            reach = f32(b + sigma[i])
                            bound2 = float(f32(reach * reach))
                    pop = True
                else:
                    l, r = left[cur], right[cur]
                    l2, r2 = row_lb2[l], row_lb2[r]
                    hl, hr = not (l2 > bound2), not (r2 > bound2)
                    first, second = (r, l) if (near_first and r2 < l2) else (l, r)
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
    hits, feat = _records(arrays, rows, best, kind, pid)
    return hits, feat, visited

"""include_ext/mirt_overlap.h restated in numpy float32, one operation per line: every candidate's overlap test for every row (a
brute force over the scene's arrays), the admitted set -- the test passed and mirt_closest.h's dist at the box's centre not a NaN
(tests/closest_ref.py's candidate functions) --, its (dist, kind, id) order, the first k as records and feature rows, and the
count.  Then the header's pruning rule as a walk over a tree given as arrays (oracle_lib.OracleScene.nodes() / refs()), which must
give the brute force's answer whatever the tree, and the any-overlap walk, which ends at the first admitted candidate.

Scenes are pyscene.PyScene.arrays() dictionaries (spheres, triangles, planes in file order).  Rows are float32 [n, 8]:
(lo, _) (hi, _)."""
import bisect

import numpy as np

import closest_ref as cr
import contacts_ref as kr

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
SLACK = f32(2.0 ** -18)
MAX_K = 8
KEY_NONE = kr.KEY_NONE
MISS = kr.MISS
HALF = f32(0.5)
ZERO = f32(0.0)


# ---- the row ----------------------------------------------------------------------------------------------------------------------
def live_rows(rows):
    lo, hi = rows[:, 0:3], rows[:, 4:7]
    with np.errstate(all="ignore"):
        return np.all(np.isfinite(lo), axis=1) & np.all(np.isfinite(hi), axis=1) & np.all(lo <= hi, axis=1)


def box_quantities(rows):
    """(lo, hi, m, h), float32 [n, 3] each: m = (lo + hi) * 0.5, h = (hi - lo) * 0.5."""
    rows = np.ascontiguousarray(rows, f32)
    lo = np.ascontiguousarray(rows[:, 0:3])
    hi = np.ascontiguousarray(rows[:, 4:7])
    with np.errstate(all="ignore"):
        s = lo + hi
        m = s * HALF
        d = hi - lo
        h = d * HALF
    cr._assert_f32(m, h)
    return lo, hi, m, h


def centre_rows(rows):
    """Rows (m, inf) for closest_ref: the point every candidate's dist, P and n are taken at."""
    _, _, m, _ = box_quantities(rows)
    return np.ascontiguousarray(np.concatenate([m, np.full((len(m), 1), np.inf, f32)], axis=1), f32)


# ---- the three overlap tests, each broadcast over [..., 3] ---------------------------------------------------------------------------
def _abs_dot(h, v):
    """(h.x |v.x| + h.y |v.y|) + h.z |v.z|"""
    x = h[..., 0] * np.abs(v[..., 0])
    y = h[..., 1] * np.abs(v[..., 1])
    z = h[..., 2] * np.abs(v[..., 2])
    s = x + y
    return s + z


def sphere_passes(lo, hi, c, rs):
    a = lo - c
    b = c - hi
    dn = np.fmax(np.fmax(a, b), ZERO)
    e = c - lo
    g = hi - c
    df = np.fmax(np.abs(e), np.abs(g))
    dmin2 = cr._dot(dn, dn)
    dmax2 = cr._dot(df, df)
    rr = rs * rs
    cr._assert_f32(dmin2, dmax2, rr)
    return (dmin2 <= rr) & (dmax2 >= rr)


def plane_passes(m, h, nor, point):
    N = cr._normalize(nor)
    d = m - point
    s = cr._dot(N, d)
    e = _abs_dot(h, N)
    cr._assert_f32(s, e)
    return np.abs(s) <= e


def _min3(x, y, z):
    return np.fmin(np.fmin(x, y), z)


def _max3(x, y, z):
    return np.fmax(np.fmax(x, y), z)


def triangle_axes(m, h, a, b, c):
    """The thirteen axes in the header's order: a list of (name, lower, upper, passes) with passes = lower & upper; lower and
    upper are returned as the pairs of compared values (value, bound) so that a caller can see how near an axis is to its bound."""
    v0 = a - m
    v1 = b - m
    v2 = c - m
    f0 = v1 - v0
    f1 = v2 - v1
    f2 = v0 - v2
    cr._assert_f32(v0, f0)
    out = []
    for k in range(3):
        mn = _min3(v0[..., k], v1[..., k], v2[..., k])
        mx = _max3(v0[..., k], v1[..., k], v2[..., k])
        out.append(("box %d" % k, mn, mx, h[..., k]))
    x1 = f0[..., 1] * f1[..., 2]
    x2 = f0[..., 2] * f1[..., 1]
    y1 = f0[..., 2] * f1[..., 0]
    y2 = f0[..., 0] * f1[..., 2]
    z1 = f0[..., 0] * f1[..., 1]
    z2 = f0[..., 1] * f1[..., 0]
    nn = np.stack([x1 - x2, y1 - y2, z1 - z2], axis=-1)
    d = cr._dot(nn, v0)
    r = _abs_dot(np.broadcast_to(h, nn.shape), nn)
    out.append(("face", d, d, r))
    for e, f in enumerate((f0, f1, f2)):
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            p = []
            for v in (v0, v1, v2):
                s = v[..., k2] * f[..., k1]
                t = v[..., k1] * f[..., k2]
                p.append(s - t)
            ra = h[..., k1] * np.abs(f[..., k2])
            rb = h[..., k2] * np.abs(f[..., k1])
            rr = ra + rb
            out.append(("edge %d axis %d" % (e, k), _min3(*p), _max3(*p), rr))
    for _, mn, mx, r in out:
        cr._assert_f32(mn, mx, r)
    return out


def triangle_passes(m, h, a, b, c):
    ok = None
    for _, mn, mx, r in triangle_axes(m, h, a, b, c):
        p = (mn <= r) & (mx >= -r)      # (the face axis: mn = mx = d, which is fabsf(d) <= r)
        ok = p if ok is None else ok & p
    return ok


def passes(arrays, rows):
    """The overlap test of every candidate for every row: (spheres [n, Ns], triangles [n, Nt], planes [n, Np]), bool."""
    lo, hi, m, h = box_quantities(rows)
    n = len(lo)
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    lo, hi, m, h = lo[:, None], hi[:, None], m[:, None], h[:, None]
    with np.errstate(all="ignore"):
        ps = sphere_passes(lo, hi, S["c"][None], S["r"][None]) if len(S) else np.zeros((n, 0), bool)
        pt = triangle_passes(m, h, T["p0"][None], T["p1"][None], T["p2"][None]) if len(T) else np.zeros((n, 0), bool)
        pp = plane_passes(m, h, Pl["nor"][None], Pl["point"][None]) if len(Pl) else np.zeros((n, 0), bool)
    return ps, pt, pp


# ---- the admitted set, its order, the records ---------------------------------------------------------------------------------------
def keys(arrays, rows):
    """(key uint64 [n, candidates]: dist's bits << 32 | kind << 30 | id for an admitted candidate and KEY_NONE for one that is not;
    the columns are the spheres, the triangles, the planes, each in file order.  kind, id [candidates]: what each column is."""
    rows = np.ascontiguousarray(rows, f32)
    live = live_rows(rows)
    cols, kinds, ids = [], [], []
    with np.errstate(all="ignore"):
        dists = cr.distances(arrays, centre_rows(rows))
        for kind, d, p in zip((cr.KIND_SPHERE, cr.KIND_TRIANGLE, cr.KIND_PLANE), dists, passes(arrays, rows)):
            assert d.dtype == f32 and p.shape == d.shape
            admitted = live[:, None] & p & (d == d)      # (the test passed, and dist is no NaN)
            low = (u64(kind) << u64(30)) | np.arange(d.shape[1], dtype=u64)
            key = (np.ascontiguousarray(d).view(u32).astype(u64) << u64(32)) | low[None, :]
            cols.append(np.where(admitted, key, u64(KEY_NONE)))
            kinds.append(np.full(d.shape[1], kind, np.int64))
            ids.append(np.arange(d.shape[1], dtype=np.int64))
    return np.concatenate(cols, axis=1), np.concatenate(kinds), np.concatenate(ids)


def records_of(arrays, rows, first):
    """(hits uint32 [n, k, 6], features float32 [n, k, 8]) of the keys `first`: mirt_closest_points' record of each candidate at m."""
    return kr.records_of(arrays, centre_rows(rows), first)


def brute_force(arrays, rows, k, key=None):
    """(hits [n, k, 6], counts uint32 [n], features [n, k, 8]): the first k of every row's admitted candidates, and their number.
    key: keys(arrays, rows)[0], if the caller has it already."""
    assert 0 <= k <= MAX_K
    if key is None:
        key, _, _ = keys(arrays, rows)
    counts = np.count_nonzero(key != u64(KEY_NONE), axis=1).astype(u32)
    first = np.sort(key, axis=1)[:, :k]
    if first.shape[1] < k:      # (fewer candidates than slots)
        first = np.concatenate([first, np.full((len(key), k - first.shape[1]), KEY_NONE, u64)], axis=1)
    hits, feat = records_of(arrays, rows, first)
    return hits, counts, feat


# ---- the pruning rule as a walk -------------------------------------------------------------------------------------------------------
def pruned_walk(arrays, rows, nodes, refs, k, slack=SLACK, left_first=True, any_overlap=False, key=None):
    """The header's rule over the tree `nodes` (closest_ref.pruned_walk's conventions): the planes, then a stack walk that visits
    a child when its box meets [lo - sigma, hi + sigma] on every axis (negated compares).  any_overlap: the walk ends at the first
    admitted candidate and the count is 0 or 1 (k must be 0).  Returns (hits, counts, features, leaves visited per row)."""
    assert 0 <= k <= MAX_K and not (any_overlap and k)
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = live_rows(rows)
    if key is None:
        key, _, _ = keys(arrays, rows)
    ns, nt = len(arrays["spheres"]), len(arrays["triangles"])
    lo, hi, _, _ = box_quantities(rows)
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        big = np.fmax(np.abs(lo).max(axis=1), np.abs(hi).max(axis=1))
        sigma = (big + C) * f32(slack)
        los = lo - sigma[:, None]
        his = hi + sigma[:, None]
        assert sigma.dtype == f32 and los.dtype == f32 and his.dtype == f32
        if len(nodes):
            meets = np.ones((n, len(nodes)), bool)
            for axis, (fmin, fmax) in enumerate((("xmin", "xmax"), ("ymin", "ymax"), ("zmin", "zmax"))):
                meets &= ~(nodes[fmin][None, :] > his[:, axis:axis + 1]) & ~(nodes[fmax][None, :] < los[:, axis:axis + 1])
            meets = meets.tolist()
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))
    column = [(ns + i) if ty else i for ty, i in zip(refs["type"].tolist(), refs["id"].tolist())]      # a sorted leaf's column of `key`
    first = np.full((n, k), KEY_NONE, u64)
    counts = np.zeros(n, u32)
    visited = np.zeros(n, np.int64)
    for i in np.flatnonzero(live):
        row_key = key[i].tolist()
        best, met = [], 0
        for x in row_key[ns + nt:]:
            if x != KEY_NONE:
                met += 1
                bisect.insort(best, x)
                del best[k:]
        if len(nodes) and not (any_overlap and met):
            row = meets[i]
            stack, cur = [], 0
            while True:
                if count[cur] > 0:
                    visited[i] += 1
                    x = row_key[column[off[cur]]]
                    if x != KEY_NONE:
                        met += 1
                        if any_overlap:
                            break
                        if k and (len(best) < k or x < best[-1]):
                            bisect.insort(best, x)
                            del best[k:]
                    pop = True
                else:
                    a, b = (left[cur], right[cur]) if left_first else (right[cur], left[cur])
                    ha, hb = row[a], row[b]
                    if ha and hb:
                        stack.append(b)
                    cur = a if ha else b
                    pop = not (ha or hb)
                if pop:
                    if not stack:
                        break
                    cur = stack.pop()
        first[i, :len(best)] = np.array(best, u64)
        counts[i] = (1 if met else 0) if any_overlap else met
    hits, feat = records_of(arrays, rows, first)
    return hits, counts, feat, visited

"""include_ext/mirt_contacts.h restated in numpy float32 on top of tests/closest_ref.py (whose candidate functions are the
restatement of mirt_closest.h, which the contacts header adopts): every candidate's distance for every row, the admitted set, its
(dist, kind, id) order, the first k as records and feature rows, and the count.  Then the header's pruning rule as a walk over a
tree given as arrays (oracle_lib.OracleScene.nodes() / refs()), with either bound rule, which must give the brute force's answer
whatever the tree.

Scenes are pyscene.PyScene.arrays() dictionaries (spheres, triangles, planes in file order).  Rows are float32 [n, 4]: (q, R)."""
import bisect

import numpy as np

import closest_ref as cr

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
MAX_K = 8
KEY_NONE = (1 << 64) - 1
MISS = np.array([f32(-1.0).view(u32), 0, 0, 0, 0, 0], u32)


def keys(arrays, rows):
    """(key uint64 [n, candidates]: dist's bits << 32 | kind << 30 | id for an admitted candidate -- dist is non-negative, so the
    keys ascend as (dist, kind, id) does -- and KEY_NONE for one that is not; the columns are the spheres, the triangles, the
    planes, each in file order.  kind, id [candidates]: what each column is."""
    rows = np.ascontiguousarray(rows, f32)
    live = cr.live_rows(rows)
    R = rows[:, 3:4]
    cols, kinds, ids = [], [], []
    with np.errstate(all="ignore"):
        for kind, d in zip((cr.KIND_SPHERE, cr.KIND_TRIANGLE, cr.KIND_PLANE), cr.distances(arrays, rows)):
            assert d.dtype == f32
            admitted = live[:, None] & (d < R)      # (dist < R; a NaN never)
            low = (u64(kind) << u64(30)) | np.arange(d.shape[1], dtype=u64)
            key = (np.ascontiguousarray(d).view(u32).astype(u64) << u64(32)) | low[None, :]
            cols.append(np.where(admitted, key, u64(KEY_NONE)))
            kinds.append(np.full(d.shape[1], kind, np.int64))
            ids.append(np.arange(d.shape[1], dtype=np.int64))
    return np.concatenate(cols, axis=1), np.concatenate(kinds), np.concatenate(ids)


def sorted_admitted(arrays, rows):
    """Per row the admitted candidates in the header's order: a list of (dist float32, kind, id)."""
    key, _, _ = keys(arrays, rows)
    out = []
    for row in np.sort(key, axis=1):
        row = row[row != u64(KEY_NONE)]
        out.append([(np.array(int(x) >> 32, u32).view(f32)[()], (int(x) >> 30) & 3, int(x) & 0x3fffffff) for x in row])
    return out


def records_of(arrays, rows, first):
    """(hits uint32 [n, k, 6], features float32 [n, k, 8]) of the keys `first` (uint64 [n, k], ascending, KEY_NONE: a miss slot):
    every record by closest_ref's operations for that candidate."""
    rows = np.ascontiguousarray(rows, f32)
    n, k = first.shape
    hits = np.zeros((n, k, 6), u32)
    feat = np.zeros((n, k, 8), f32)
    for j in range(k):
        x = first[:, j]
        hit = x != u64(KEY_NONE)
        dist = np.where(hit, (x >> u64(32)).astype(u32), f32(np.inf).view(u32)).astype(u32).view(f32)
        kind = np.where(hit, (x >> u64(30)) & u64(3), 0).astype(np.int64)
        pid = np.where(hit, x & u64(0x3fffffff), 0).astype(np.int64)
        hits[:, j], feat[:, j] = cr._records(arrays, rows, dist, kind, pid)
    return hits, feat


def brute_force(arrays, rows, k):
    """(hits [n, k, 6], counts uint32 [n], features [n, k, 8]): the first k of every row's admitted candidates, and their number."""
    assert 0 <= k <= MAX_K
    key, _, _ = keys(arrays, rows)
    counts = np.count_nonzero(key != u64(KEY_NONE), axis=1).astype(u32)
    first = np.sort(key, axis=1)[:, :k]
    if first.shape[1] < k:      # (fewer candidates than slots)
        first = np.concatenate([first, np.full((len(key), k - first.shape[1]), KEY_NONE, u64)], axis=1)
    hits, feat = records_of(arrays, rows, first)
    return hits, counts, feat


def pruned_walk(arrays, rows, nodes, refs, k, with_counts, slack=cr.SLACK, near_first=True):
    """The header's rule over the tree `nodes` (closest_ref.pruned_walk's conventions): the planes, then a stack walk that leaves a
    subtree out only when its squared box distance exceeds (B + sigma)^2.  with_counts: B is R for the whole walk.  Otherwise B is
    R until the list holds k keys and the list's largest distance from then on.  Returns (hits, counts, features, leaves visited
    per row); without counts the count is that of the candidates the walk met, which the caller must not read."""
    assert 0 <= k <= MAX_K and (with_counts or k > 0)
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = cr.live_rows(rows)
    key, kinds, ids = keys(arrays, rows)
    ns, nt = len(arrays["spheres"]), len(arrays["triangles"])
    q = np.ascontiguousarray(rows[:, 0:3], f32)
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        lb2 = cr.box_distance2(nodes, q).tolist() if len(nodes) else None
        qmax = np.fmax(np.fmax(np.abs(q[:, 0]), np.abs(q[:, 1])), np.abs(q[:, 2]))
        sigma = (qmax + C) * f32(slack)
    assert sigma.dtype == f32
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))
    column = [(ns + i) if ty else i for ty, i in zip(refs["type"].tolist(), refs["id"].tolist())]      # a sorted leaf's column of `key`
    first = np.full((n, k), KEY_NONE, u64)
    counts = np.zeros(n, u32)
    visited = np.zeros(n, np.int64)

    def bound2_of(best, R, s):
        B = R if (with_counts or len(best) < k) else np.array(best[-1] >> 32, u32).view(f32)[()]
        with np.errstate(all="ignore"):
            reach = f32(B + s)
            return float(f32(reach * reach))

    for i in np.flatnonzero(live):
        row_key = key[i].tolist()
        best, met = [], 0
        for x in row_key[ns + nt:]:
            if x != KEY_NONE:
                met += 1
                bisect.insort(best, x)
                del best[k:]
        if len(nodes):
            row_lb2 = lb2[i]
            R, s = rows[i, 3], sigma[i]
            bound2 = bound2_of(best, R, s)
            stack, cur = [], 0
            while True:
                if count[cur] > 0:
                    visited[i] += 1
                    x = row_key[column[off[cur]]]
                    if x != KEY_NONE:
                        met += 1
                        if k and (len(best) < k or x < best[-1]):
                            bisect.insort(best, x)
                            del best[k:]
                            if not with_counts:
                                bound2 = bound2_of(best, R, s)
                    pop = True
                else:
                    l, r = left[cur], right[cur]
                    l2, r2 = row_lb2[l], row_lb2[r]
                    hl, hr = not (l2 > bound2), not (r2 > bound2)
                    a, b = (r, l) if (near_first and r2 < l2) else (l, r)
                    if hl and hr:
                        stack.append(b)
                        cur = a
                    else:
                        cur = l if hl else r
                    pop = not (hl or hr)
                if pop:
                    if not stack:
                        break
                    cur = stack.pop()
        first[i, :len(best)] = np.array(best, u64)
        counts[i] = met
    hits, feat = records_of(arrays, rows, first)
    return hits, counts, feat, visited

"""include_ext3/mirt_cast_lists.h restated in numpy float32 on top of tests/spherecast_ref.py: the set of every row is that
restatement's admitted candidates (`candidates`, `admitted`) -- for a sphere or a triangle also the header's clause (0), the slab test
of the primitive's own builder box made from the scene's arrays --, the order within a row the header's -- the planes by index, then
the spheres and triangles in the scene's leaf order, which is the oracle tree's refs --, a value the t of the matrix, the offsets
overlap_list_ref.offsets_of, and the fill bounded by the caller's offsets and capacity, for words and values alike.  Then the list
walk as the kernel makes it: the bound fixed at tmax + tmax * tau, the left child first, emitting as it goes.

A word is kind << 30 | id (uint32); a value is float32.  Rows are float32 [n, 8]: (ox, oy, oz, tmax) (dx, dy, dz, r)."""
import numpy as np

import overlap_list_ref as olr
import spherecast_ref as sr
from query_lists_ref import bits, fill, leaf_words      # noqa: F401  (the fill rule is the lists': words and values alike)

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
SLACK = sr.SLACK
TAU = sr.TAU
ZERO = f32(0.0)
THIN = f32(0.01)


# ---- clause (0): the primitive's own builder box, from the scene's arrays ----------------------------------------------------------------
def builder_boxes(arrays):
    """(lo [Ns + Nt, 3], hi [Ns + Nt, 3]) float32, spheres then triangles in file order: a sphere's c -/+ rs per axis, swapped where
    lo <= hi is false; a triangle's componentwise fmin / fmax of its vertices, an axis on which hi - lo < 0.01f widened by 0.01f at both
    ends."""
    S, T = arrays["spheres"], arrays["triangles"]
    with np.errstate(all="ignore"):
        c, rs = np.ascontiguousarray(S["c"], f32).reshape(-1, 3), np.ascontiguousarray(S["r"], f32).reshape(-1, 1)
        a, b = c - rs, c + rs
        keep = a <= b
        slo, shi = np.where(keep, a, b), np.where(keep, b, a)
        p0, p1, p2 = (np.ascontiguousarray(T[k], f32).reshape(-1, 3) for k in ("p0", "p1", "p2"))
        tlo, thi = np.fmin(np.fmin(p0, p1), p2), np.fmax(np.fmax(p0, p1), p2)
        thin = (thi - tlo) < THIN
        tlo, thi = np.where(thin, tlo - THIN, tlo), np.where(thin, thi + THIN, thi)
    lo, hi = np.concatenate([slo, tlo]).astype(f32), np.concatenate([shi, thi]).astype(f32)
    return lo, hi


def scene_coord_max(arrays):
    """C: the largest coordinate magnitude of the box of all builder boxes (0 for fewer than two primitives: no box is tested)."""
    lo, hi = builder_boxes(arrays)
    if len(lo) < 2:
        return f32(0.0)
    return f32(max(np.abs(lo.min(axis=0)).max(), np.abs(hi.max(axis=0)).max()))


def row_quantities(rows, C, slack=SLACK, tau=TAU):
    """(o, d^, grow, bound) of every row: sigma = ((max |o| + C) + r) * slack, grow = r + sigma, bound = tmax + tmax * tau."""
    rows = np.ascontiguousarray(rows, f32)
    o = np.ascontiguousarray(rows[:, 0:3])
    with np.errstate(all="ignore"):
        d = sr.directions(rows)
        omax = np.fmax(np.fmax(np.abs(o[:, 0]), np.abs(o[:, 1])), np.abs(o[:, 2]))
        sigma = ((omax + f32(C)) + rows[:, 7]) * f32(slack)
        grow = rows[:, 7] + sigma
        bound = rows[:, 3] + rows[:, 3] * f32(tau)
    assert sigma.dtype == f32 and grow.dtype == f32 and bound.dtype == f32
    return o, d, grow, bound


def box_passes(lo, hi, o, d, grow, bound):
    """[n, boxes]: enter > fminf(leave, bound) is false, by spherecast_ref.slab_intervals' operations (the kernel's box_interval)."""
    boxes = {"xmin": lo[:, 0], "xmax": hi[:, 0], "ymin": lo[:, 1], "ymax": hi[:, 1], "zmin": lo[:, 2], "zmax": hi[:, 2]}
    with np.errstate(all="ignore"):
        enter, leave = sr.slab_intervals(boxes, o, d, grow)
        return ~(enter > np.fmin(leave, bound[:, None]))


def clause0(arrays, rows, slack=SLACK, tau=TAU):
    """[n, Ns + Nt] bool: the header's clause (0) for every sphere and triangle (all True for a scene of fewer than two)."""
    lo, hi = builder_boxes(arrays)
    if len(lo) < 2:
        return np.ones((len(rows), len(lo)), bool)
    o, d, grow, bound = row_quantities(rows, scene_coord_max(arrays), slack, tau)
    return box_passes(lo, hi, o, d, grow, bound)


# ---- the lists --------------------------------------------------------------------------------------------------------------------------
def members(arrays, rows, cands=None, clause=True):
    """(in [n, Ns + Nt + Np] bool, t [n, Ns + Nt + Np] float32), the columns spheres, triangles, planes in file order: the admitted
    candidates of live rows, a sphere or triangle under clause (0) too (clause=False: spherecast_ref's admitted set as it is)."""
    rows = np.ascontiguousarray(rows, f32)
    ts, tt, tp = cands or sr.candidates(arrays, rows)
    t = np.concatenate([ts, tt, tp], axis=1).astype(f32)
    ok = sr.admitted(t, rows) & sr.live_rows(rows)[:, None]
    if clause:
        ok[:, :ts.shape[1] + tt.shape[1]] &= clause0(arrays, rows)
    return ok, t


def lists(arrays, rows, refs, cands=None, clause=True):
    """(offsets int64 [n + 1], words uint32, t float32): every row's set in the header's order, the segments exact."""
    ok, t = members(arrays, rows, cands, clause)
    cols, words = olr.column_order(arrays, refs)
    ok, t = ok[:, cols], t[:, cols]
    return (olr.offsets_of(ok.sum(axis=1)), np.ascontiguousarray(np.broadcast_to(words[None, :], ok.shape)[ok], u32), np.ascontiguousarray(t[ok], f32))


def sorted_rows(offsets, words, t):
    """Per row (t bits, kind, id) in mirt_spherecast.h's order: a sort of the row by t's bits << 32 | word."""
    out = []
    for i in range(len(offsets) - 1):
        w, b = words[offsets[i]:offsets[i + 1]], bits(t[offsets[i]:offsets[i + 1]])
        at = np.argsort((b.astype(u64) << u64(32)) | w.astype(u64))
        kind, pid = olr.unpack(w[at])
        out.append(np.stack([b[at].astype(np.int64), kind, pid], axis=1))
    return out


# ---- the walk as the kernel makes it -------------------------------------------------------------------------------------------------
def walk(arrays, rows, nodes, refs, cands=None, slack=SLACK, tau=TAU, left_first=True):
    """The planes, then a stack walk from the root (entered untested) over `nodes` (oracle_lib.NODE) that enters a child when the
    centre ray meets its box grown by r + sigma within [0, tmax + tmax * tau] -- the bound never moves --, the left child first,
    emitting (word, t) of every leaf whose candidate is admitted, as it is visited.  No clause is applied at a leaf: the boxes on
    the way are the whole test.  Returns per row (words uint32, t float32)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = sr.live_rows(rows)
    ts, tt, tp = cands or sr.candidates(arrays, rows)
    ok_s, ok_t, ok_p = (sr.admitted(t, rows) for t in (ts, tt, tp))
    npl = tp.shape[1]
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    o, d, grow, bound = row_quantities(rows, C, slack, tau)
    if len(nodes):
        with np.errstate(all="ignore"):
            enter, leave = sr.slab_intervals(nodes, o, d, grow)
            enters = (~(enter > np.fmin(leave, bound[:, None]))).tolist()
        left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))
    rtype, rid = np.asarray(refs["type"]).tolist(), np.asarray(refs["id"]).tolist()
    lw = leaf_words(refs).tolist()
    out = []
    for i in range(n):
        w, t = [], []
        if live[i]:
            for j in range(npl):
                if ok_p[i, j]:
                    w.append(int(olr.word(olr.KIND_PLANE, j)))
                    t.append(tp[i, j])
            if len(nodes):
                row = enters[i]
                stack, cur = [], 0
                while True:
                    if count[cur] > 0:
                        r = off[cur]
                        j = rid[r]
                        if (ok_t[i, j] if rtype[r] else ok_s[i, j]):
                            w.append(lw[r])
                            t.append(tt[i, j] if rtype[r] else ts[i, j])
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
        out.append((np.array(w, u32), np.array(t, f32)))
    return out


def leaf_boxes(nodes, refs, arrays):
    """(lo, hi) [Ns + Nt, 3] of the tree's leaves, in builder_boxes' order (spheres then triangles, file order)."""
    ns = len(arrays["spheres"])
    lo = np.zeros((len(refs), 3), f32)
    hi = np.zeros((len(refs), 3), f32)
    for k in np.flatnonzero(nodes["count"] > 0):
        r = int(nodes["prim_offset"][k])
        col = (ns if refs["type"][r] else 0) + int(refs["id"][r])
        lo[col] = [nodes[f][k] for f in ("xmin", "ymin", "zmin")]
        hi[col] = [nodes[f][k] for f in ("xmax", "ymax", "zmax")]
    return lo, hi

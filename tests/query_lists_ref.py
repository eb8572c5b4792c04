"""include_ext/mirt_query_lists.h restated in numpy on top of tests/multihit_ref.py (rays) and tests/contacts_ref.py (balls): the
set of every row is that restatement's admitted set, the order within a row the header's -- the planes by index, then the spheres
and triangles in the scene's leaf order, which is the oracle tree's refs --, a value the t or dist the record call carries, the
offsets overlap_list_ref.offsets_of, and the fill bounded by the caller's offsets and capacity, for words and values alike.
Then the header's order as the two walks the kernels make, left child first over the oracle's nodes, emitting as they go.

A word is kind << 30 | id (uint32); a value is float32.  Rays are float32 [n, 8], ball rows float32 [n, 4]: (q, R)."""
import numpy as np

import closest_ref as cr
import contacts_ref as kr
import multihit_ref as mr
import overlap_list_ref as olr

f32 = np.float32
u32 = np.uint32
u64 = np.uint64


def leaf_words(refs):
    """The word of every leaf, in sorted-leaf order."""
    ty, pid = np.asarray(refs["type"]).astype(np.int64), np.asarray(refs["id"]).astype(np.int64)
    return np.where(ty != 0, olr.word(olr.KIND_TRIANGLE, pid), olr.word(olr.KIND_SPHERE, pid)).astype(u32)


def _pick(admitted, words, values):
    """(offsets, words, values) of an [n, columns] admission in column order."""
    counts = admitted.sum(axis=1)
    return (olr.offsets_of(counts), np.ascontiguousarray(np.broadcast_to(words[None, :], admitted.shape)[admitted], u32),
            np.ascontiguousarray(values[admitted], f32))


def ray_lists(refs, S):
    """(offsets int64 [n + 1], words uint32, t float32) of a multihit_ref.admitted() result S: per row the columns in_p, then in_l --
    the planes by index and the leaves in sorted order already."""
    npl = S["tp"].shape[1]
    words = np.concatenate([olr.word(olr.KIND_PLANE, np.arange(npl)), leaf_words(refs)]).astype(u32)
    return _pick(np.concatenate([S["in_p"], S["in_l"]], axis=1), words, np.concatenate([S["tp"], S["tl"]], axis=1).astype(f32))


def ball_lists(arrays, rows, refs, key=None):
    """(offsets int64 [n + 1], words uint32, dist float32): admitted where contacts_ref's key is not KEY_NONE, dist the key's high
    word, the columns reordered by overlap_list_ref.column_order."""
    if key is None:
        key, _, _ = kr.keys(arrays, rows)
    cols, words = olr.column_order(arrays, refs)
    key = key[:, cols]
    dist = (key >> u64(32)).astype(u32).view(f32)
    return _pick(key != u64(kr.KEY_NONE), words, dist)


def bits(values):
    return np.ascontiguousarray(values, f32).view(u32)


def fill(want_offsets, want, offsets, buffer, capacity=None):
    """What a fill leaves in `buffer` (4-byte entries, its content before the call; a uint32 copy is returned) when the rows' true
    lists are (want_offsets, want) -- the words, or the values -- the caller's offsets are `offsets` and the call's capacity is
    `capacity` (None: the buffer's size): row i writes the first min(|set|, offsets[i + 1] - offsets[i]) entries of its list from
    offsets[i] on, none at an index outside [0, capacity)."""
    out = np.array(np.ascontiguousarray(buffer).view(u32), copy=True)
    want = np.ascontiguousarray(want).view(u32)
    cap = len(out) if capacity is None else int(capacity)
    assert 0 <= cap <= len(out)
    offsets = np.asarray(offsets, np.int64)
    for i in range(len(offsets) - 1):
        mine = want[want_offsets[i]:want_offsets[i + 1]]
        k = min(len(mine), max(int(offsets[i + 1] - offsets[i]), 0))
        at = int(offsets[i]) + np.arange(k)
        ok = (at >= 0) & (at < cap)
        out[at[ok]] = mine[:k][ok]
    return out


def _tree_lists(nodes):
    return (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset"))


def ray_walk(arrays, rays, nodes, refs, left_first=True):
    """The ray fill as the kernel makes it: the planes, then a stack walk from the root (entered untested) that enters a child when
    multihit_ref.box_test says so with the bound at tmax, emitting (word, t) of every leaf whose test admits it, as it is visited.
    Returns per row (words uint32, t float32)."""
    o, d, tmax, live = mr.split(rays)
    n = len(o)
    npl = len(arrays["planes"])
    lw = leaf_words(refs).tolist()
    with np.errstate(all="ignore"):
        tp, in_p = mr._planes(arrays, o, d, tmax, live)
        if len(nodes):
            tl, ok = mr.leaf_tests(arrays, o, d, tmax, refs)
            _, enter = mr.box_test(nodes, o, d, tmax)
            enter = enter.tolist()
            left, right, count, off = _tree_lists(nodes)
    out = []
    for i in range(n):
        w, t = [], []
        if live[i]:
            for j in range(npl):
                if in_p[i, j]:
                    w.append(int(olr.word(olr.KIND_PLANE, j)))
                    t.append(tp[i, j])
            if len(nodes):
                row, row_ok, row_t = enter[i], ok[i].tolist(), tl[i]
                stack, cur = [], 0
                while True:
                    if count[cur] > 0:
                        r = off[cur]
                        if row_ok[r]:
                            w.append(lw[r])
                            t.append(row_t[r])
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


def ball_walk(arrays, rows, nodes, refs, key=None, slack=cr.SLACK, left_first=True):
    """The ball fill as the kernel makes it: the planes, then contacts_ref.pruned_walk's rule in count mode -- a subtree is left out
    only when its squared box distance exceeds (R + sigma)^2 -- with the left child first, emitting (word, dist) of every admitted
    leaf as it is visited.  Returns per row (words uint32, dist float32)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = cr.live_rows(rows)
    if key is None:
        key, _, _ = kr.keys(arrays, rows)
    ns, nt, npl = len(arrays["spheres"]), len(arrays["triangles"]), len(arrays["planes"])
    q = np.ascontiguousarray(rows[:, 0:3], f32)
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        lb2 = cr.box_distance2(nodes, q) if len(nodes) else None
        qmax = np.fmax(np.fmax(np.abs(q[:, 0]), np.abs(q[:, 1])), np.abs(q[:, 2]))
        sigma = (qmax + C) * f32(slack)
        reach = (rows[:, 3] + sigma).astype(f32)
        bound2 = (reach * reach).astype(f32)
        near = (~(lb2 > bound2[:, None])).tolist() if len(nodes) else None
    assert sigma.dtype == f32
    lw = leaf_words(refs).tolist()
    column = [(ns + i) if ty else i for ty, i in zip(np.asarray(refs["type"]).tolist(), np.asarray(refs["id"]).tolist())]
    if len(nodes):
        left, right, count, off = _tree_lists(nodes)
    out = []
    for i in range(n):
        w, dist = [], []
        if live[i]:
            row_key = key[i].tolist()
            for j in range(npl):
                x = row_key[ns + nt + j]
                if x != kr.KEY_NONE:
                    w.append(int(olr.word(olr.KIND_PLANE, j)))
                    dist.append(x >> 32)
            if len(nodes):
                row = near[i]
                stack, cur = [], 0
                while True:
                    if count[cur] > 0:
                        r = off[cur]
                        x = row_key[column[r]]
                        if x != kr.KEY_NONE:
                            w.append(lw[r])
                            dist.append(x >> 32)
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
        out.append((np.array(w, u32), np.array(dist, u32).view(f32)))
    return out


def ray_sorted_rows(offsets, words, t):
    """Per row (t bits, kind, id) in mirt_multihit.h's order: a stable sort of the row by the bits of t."""
    out = []
    for i in range(len(offsets) - 1):
        w, b = words[offsets[i]:offsets[i + 1]], bits(t[offsets[i]:offsets[i + 1]])
        at = np.argsort(b, kind="stable")
        kind, pid = olr.unpack(w[at])
        out.append(np.stack([b[at].astype(np.int64), kind, pid], axis=1))
    return out


def ball_sorted_rows(offsets, words, dist):
    """Per row (dist bits, kind, id) in mirt_contacts.h's order: a sort of the row by dist's bits << 32 | word."""
    out = []
    for i in range(len(offsets) - 1):
        w, b = words[offsets[i]:offsets[i + 1]], bits(dist[offsets[i]:offsets[i + 1]])
        at = np.argsort((b.astype(u64) << u64(32)) | w.astype(u64))
        kind, pid = olr.unpack(w[at])
        out.append(np.stack([b[at].astype(np.int64), kind, pid], axis=1))
    return out

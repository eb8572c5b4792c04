"""include_ext/mirt_overlap_list.h restated in numpy on top of tests/overlap_ref.py: the admitted set of every row is that
restatement's (a column of overlap_ref.keys is admitted when its key is not KEY_NONE), the order within a row the header's -- the
planes by index, then the spheres and triangles in the scene's leaf order, which is the oracle tree's refs
(test_closest_abi._oracle_tree) --, the offsets np.cumsum in int64, and the fill bounded by the caller's offsets and capacity.
Then the header's order as a walk: overlap_ref.pruned_walk's rule, left child first, emitting words.

A word is kind << 30 | id (uint32).  Rows are float32 [n, 8]: (lo, _) (hi, _)."""
import numpy as np

import overlap_ref as ovr

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
KIND_SPHERE, KIND_TRIANGLE, KIND_PLANE = 1, 2, 3


def word(kind, pid):
    return (u32(kind) << u32(30)) | np.asarray(pid, u32)


def unpack(words):
    """(kind, id) of words."""
    w = np.asarray(words, u32)
    return (w >> u32(30)).astype(np.int64), (w & u32(0x3fffffff)).astype(np.int64)


def offsets_of(counts):
    """int64 [n + 1]: 0, then the running sums of the counts."""
    out = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts).astype(np.int64), out=out[1:])
    return out


def column_order(arrays, refs):
    """(the columns of overlap_ref.keys in the header's order within a row, their words): the planes ascending, then the leaves as
    `refs` (the oracle's sorted primitive references: type 0 sphere / 1 triangle, file-order id) has them."""
    ns, nt, npl = len(arrays["spheres"]), len(arrays["triangles"]), len(arrays["planes"])
    ty, pid = np.asarray(refs["type"]).astype(np.int64), np.asarray(refs["id"]).astype(np.int64)
    assert len(ty) == ns + nt and sorted(np.where(ty != 0, ns + pid, pid).tolist()) == list(range(ns + nt))      # every primitive once
    cols = np.concatenate([ns + nt + np.arange(npl, dtype=np.int64), np.where(ty != 0, ns + pid, pid)]).astype(np.int64)
    words = np.concatenate([word(KIND_PLANE, np.arange(npl)), np.where(ty != 0, word(KIND_TRIANGLE, pid), word(KIND_SPHERE, pid))]).astype(u32)
    return cols, words


def lists(arrays, rows, refs, key=None):
    """(offsets int64 [n + 1], words uint32 [offsets[n]]): every row's admitted set in the header's order, the segments exact."""
    if key is None:
        key, _, _ = ovr.keys(arrays, rows)
    cols, words = column_order(arrays, refs)
    admitted = (key != u64(ovr.KEY_NONE))[:, cols]
    counts = admitted.sum(axis=1)
    return offsets_of(counts), np.ascontiguousarray(np.broadcast_to(words[None, :], admitted.shape)[admitted], u32)


def fill(want_offsets, want_words, offsets, buffer, capacity=None):
    """What mirt_overlap_list leaves in `buffer` (uint32, its content before the call; a copy is returned) when the rows' true lists
    are (want_offsets, want_words), the caller's offsets are `offsets` and the call's capacity is `capacity` (None: the buffer's
    size): row i writes the first min(|A_i|, offsets[i + 1] - offsets[i]) words of its list from offsets[i] on, none at an index
    outside [0, capacity)."""
    out = np.array(buffer, u32, copy=True)
    cap = len(out) if capacity is None else int(capacity)
    assert 0 <= cap <= len(out)
    offsets = np.asarray(offsets, np.int64)
    for i in range(len(offsets) - 1):
        mine = want_words[want_offsets[i]:want_offsets[i + 1]]
        k = min(len(mine), max(int(offsets[i + 1] - offsets[i]), 0))
        for j in range(k):
            at = int(offsets[i]) + j
            if 0 <= at < cap:
                out[at] = mine[j]
    return out


def walk_words(arrays, rows, nodes, refs, key=None, slack=ovr.SLACK, left_first=True):
    """The header's order as the kernel makes it: the planes, then overlap_ref.pruned_walk's rule over the tree `nodes`, emitting
    the word of every admitted leaf as it is visited.  Returns the list of every row's words (a list of uint32 arrays)."""
    rows = np.ascontiguousarray(rows, f32)
    n = len(rows)
    live = ovr.live_rows(rows)
    if key is None:
        key, _, _ = ovr.keys(arrays, rows)
    ns, nt, npl = len(arrays["spheres"]), len(arrays["triangles"]), len(arrays["planes"])
    lo, hi, _, _ = ovr.box_quantities(rows)
    single = len(nodes) == 1
    C = f32(0.0) if single or not len(nodes) else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        big = np.fmax(np.abs(lo).max(axis=1), np.abs(hi).max(axis=1))
        sigma = (big + C) * f32(slack)
        los, his = lo - sigma[:, None], hi + sigma[:, None]
        if len(nodes):
            meets = np.ones((n, len(nodes)), bool)
            for axis, (fmin, fmax) in enumerate((("xmin", "xmax"), ("ymin", "ymax"), ("zmin", "zmax"))):
                meets &= ~(nodes[fmin][None, :] > his[:, axis:axis + 1]) & ~(nodes[fmax][None, :] < los[:, axis:axis + 1])
            meets = meets.tolist()
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset")) if len(nodes) else ([], [], [], [])
    ty, pid = np.asarray(refs["type"]).tolist(), np.asarray(refs["id"]).tolist()
    out = []
    for i in range(n):
        got = []
        if live[i]:
            row_key = key[i].tolist()
            got += [int(word(KIND_PLANE, j)) for j in range(npl) if row_key[ns + nt + j] != ovr.KEY_NONE]
            if len(nodes):
                row = meets[i]
                stack, cur = [], 0
                while True:
                    if count[cur] > 0:
                        r = off[cur]
                        if row_key[(ns + pid[r]) if ty[r] else pid[r]] != ovr.KEY_NONE:
                            got.append(int(word(KIND_TRIANGLE if ty[r] else KIND_SPHERE, pid[r])))
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
        out.append(np.array(got, u32))
    return out

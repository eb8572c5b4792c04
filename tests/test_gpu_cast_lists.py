"""Cast lists on the GPU (include_ext3/mirt_cast_lists.h: mirt_cast_counts, mirt_cast_list; cast_lists.count_casts, cast_list,
cast_lists).  The yardstick is tests/cast_lists_ref.py: spherecast_ref's admitted candidates of every row (under the header's
clause (0)) in the oracle tree's leaf order, with the t of each, compared with np.array_equal on the counts, the words and the
values' bits, order included.  The inputs are those tests/test_cast_lists_abi.py checks the restatement on.  Then the GPU against
itself: every row's smallest key is mirt_cast_spheres' record on that row."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
import cast_lists_ref as clr
import overlap_list_ref as olr
import spherecast_ref as sr
from test_cast_lists_abi import case, reference
from test_gpu_multihit import Scene      # (a built scene with its host arrays and the library's tree)
from test_spherecast_abi import UPDATE_MOVED

pytestmark = pytest.mark.gpu

MOD = importlib.import_module("cuda_ray_tracer_amd.cast_lists")      # (the package's attribute of that name is the function)

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32
u64 = np.uint64
SENTINEL = 0x5eed5eed      # (no word: kind 1 with an id no test scene has; as a value's bits, a float no test computes)
PAST = 64                  # sentinel entries past the end of every array of words and of values


def _buffer(count):
    return torch.full((count,), SENTINEL, dtype=torch.int32, device=DEV)


def _np(t):
    return t.cpu().numpy().view(u32)


def _counts(raw, rows, stream=None):
    """mirt_cast_counts on the rows (numpy): uint32 [n]; the entry after the last keeps its sentinel."""
    n = len(rows)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    counts = _buffer(n + 1)
    torch.cuda.synchronize()
    m.count_casts(raw, d_rows, counts[:n], stream=stream)
    torch.cuda.synchronize()
    assert int(counts[n]) == SENTINEL
    return _np(counts[:n])


def _fill(raw, rows, offsets=None, capacity=None, size=None, values=True, stream=None):
    """The fill on the rows (numpy) with the caller's offsets (numpy int64; None: the GPU's own counts through the GPU's scan) into
    arrays of `size` entries (None: the offsets' total) plus PAST sentinel entries, the call's capacity being `capacity` (None:
    size).  Returns (offsets numpy, the whole array of words as uint32, the whole array of values as uint32 bits or None)."""
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    d_off = m.list_offsets(raw, m.count_casts(raw, d_rows)) if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(DEV)
    off = d_off.cpu().numpy()
    size = int(off[-1]) if size is None else size
    cap = size if capacity is None else capacity
    words, vals = _buffer(size + PAST), (_buffer(size + PAST) if values else None)
    torch.cuda.synchronize()
    m.cast_list(raw, d_rows, d_off, words[:cap], vals[:cap].view(torch.float32) if values else None, stream=stream)
    torch.cuda.synchronize()
    return off, _np(words), (_np(vals) if values else None)


def _assert_equals(raw, rows, want, **kw):
    """The counts; then with the value array and without it: the offsets, the words, the values' bits, the sentinels past the end."""
    want_off, want_words, want_vals = want
    total = int(want_off[-1])
    counts = _counts(raw, rows)
    bad = np.flatnonzero(counts.astype(np.int64) != np.diff(want_off))
    assert len(bad) == 0, (len(bad), bad[:5], counts[bad[:5]], np.diff(want_off)[bad[:5]], rows[bad[:5]])
    for values in (True, False):
        off, words, vals = _fill(raw, rows, values=values, **kw)
        assert np.array_equal(off, want_off)      # (the GPU's counts through the GPU's scan)
        bad = np.flatnonzero(words[:total] != want_words)
        assert len(bad) == 0, (len(bad), bad[:5], words[bad[:5]], want_words[bad[:5]])
        assert len(words) == total + PAST and np.all(words[total:] == SENTINEL)
        if values:
            assert np.array_equal(vals[:total], clr.bits(want_vals)) and len(vals) == total + PAST and np.all(vals[total:] == SENTINEL)
    return off, words[:total]


# ---- 1. against the reference, order included ---------------------------------------------------------------------------------------
LISTED = ["mixed", "mixed_planes", "single_sphere", "single_triangle", "empty", "plane_only", "far_1e3", "far_1e5", "chosen", "along_edges", "dense"]


@pytest.mark.parametrize("name", LISTED)
def test_lists_equal_the_reference_in_the_reference_order(name):
    text, arrays, rows = case(name)
    sc = Scene(text)
    try:
        off, words = _assert_equals(sc.raw, rows, reference(name)[0])
    finally:
        sc.close()
    lens = np.diff(off)
    kinds = set(olr.unpack(words)[0].tolist())
    if name == "dense":      # the case that matters: lists far longer than the one record of the record call, rows that are not live
        dead = ~sr.live_rows(rows)
        assert np.mean(lens > 8) > 0.10 and kinds == {1, 2, 3} and dead.sum() == 80 and np.all(lens[dead] == 0)
    if name in ("single_sphere", "single_triangle", "empty", "plane_only"):
        assert kinds == {"empty": set(), "plane_only": {3}, "single_sphere": {1}, "single_triangle": {2}}[name]
        assert lens.max() == (0 if name == "empty" else 1)


# ---- 2. the spill path; a wave, a block, more rows than a grid of lanes -------------------------------------------------------------------
@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, arrays, rows = case("deep_stack")
    sc = Scene(text)
    try:
        assert sc.raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            sc.raw.set_option("stack_lds_depth", depth)
        off, _ = _assert_equals(sc.raw, rows, reference("deep_stack")[0])
    finally:
        sc.close()
    assert len(rows) == 240 and np.diff(off).max() == 3000


def test_row_counts_around_a_wave_a_block_and_a_grid():
    text, arrays, base = case("row_counts")
    want_off, want_words, want_vals = reference("row_counts")[0]
    assert len(base) == 4096 and want_off[-1] > 0
    sc = Scene(text)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257):
            assert np.array_equal(_counts(sc.raw, base[:n]).astype(np.int64), np.diff(want_off)[:n]), n
        _assert_equals(sc.raw, base, (want_off, want_words, want_vals))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37      # every lane takes a second row
        reps = -(-n // len(base))
        rows = np.tile(base, (reps, 1))[:n]
        lens = np.tile(np.diff(want_off), reps)[:n]
        off, words, vals = _fill(sc.raw, rows)
    finally:
        sc.close()
    assert np.array_equal(off, olr.offsets_of(lens))
    whole, per = n // len(base), len(want_words)
    assert np.array_equal(words[:whole * per].reshape(whole, per), np.broadcast_to(want_words, (whole, per)))
    assert np.array_equal(vals[:whole * per].reshape(whole, per), np.broadcast_to(clr.bits(want_vals), (whole, per)))
    rest = int(off[-1]) - whole * per
    assert np.array_equal(words[whole * per:off[-1]], want_words[:rest]) and np.array_equal(vals[whole * per:off[-1]], clr.bits(want_vals)[:rest])
    assert np.all(words[off[-1]:] == SENTINEL) and np.all(vals[off[-1]:] == SENTINEL)


# ---- 3. the GPU against itself: mirt_cast_spheres in the same process ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense", "mixed_planes", "along_edges"])
def test_every_rows_smallest_key_is_the_first_contact_and_any_contact_is_listed(name):
    text, arrays, rows = case(name)
    n = len(rows)
    sc = Scene(text)
    try:
        d_rows = torch.from_numpy(rows).to(DEV)
        first = torch.full((n, 6), -7, dtype=torch.int32, device=DEV)
        some = torch.full((n, 6), -7, dtype=torch.int32, device=DEV)
        m.cast_spheres(sc.raw, d_rows, first)
        m.cast_spheres(sc.raw, d_rows, some, any_hit=True)
        off, words, vals = m.cast_lists(sc.raw, d_rows)
        soff, swords, svals = m.cast_lists(sc.raw, d_rows, sort=True)
        no_values = m.cast_lists(sc.raw, d_rows, values=False, sort=True, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
    finally:
        sc.close()
    assert off.dtype == torch.int64 and words.dtype == torch.int32 and vals.dtype == torch.float32
    first, some, off = _np(first), _np(some), off.cpu().numpy()
    words, vals = _np(words), _np(vals.view(torch.int32))
    want = reference(name)[0]
    assert np.array_equal(off, want[0]) and np.array_equal(words, want[1]) and np.array_equal(vals, clr.bits(want[2]))
    lens = np.diff(off)
    # a row is empty exactly on a miss; its smallest t bits << 32 | word is the first contact's record
    assert np.array_equal(lens == 0, first[:, 1] == 0) and np.any(lens == 0) and np.any(lens > 1)
    key = (vals.astype(u64) << u64(32)) | words.astype(u64)
    has = np.flatnonzero(lens > 0)
    smallest = np.minimum.reduceat(key, off[:-1][has])
    record = (first[has, 0].astype(u64) << u64(32)) | (first[has, 1].astype(u64) << u64(30)) | first[has, 2].astype(u64)
    assert np.array_equal(smallest, record)
    # MIRT_CAST_ANY_HIT's record names a listed surface with its listed t
    assert np.array_equal(some[:, 1] != 0, first[:, 1] != 0)
    row = np.repeat(np.arange(n), lens)
    listed = set(zip(row.tolist(), key.tolist()))
    any_key = (some[has, 0].astype(u64) << u64(32)) | (some[has, 1].astype(u64) << u64(30)) | some[has, 2].astype(u64)
    assert all((int(i), int(k)) in listed for i, k in zip(has, any_key))
    # sort=True: every segment is non-decreasing in that key, begins with the record, and holds the same entries
    swords, svals = _np(swords), _np(svals.view(torch.int32))
    skey = (svals.astype(u64) << u64(32)) | swords.astype(u64)
    assert np.array_equal(soff.cpu().numpy(), off)
    same = row[1:] == row[:-1]
    assert np.all(skey[1:][same] >= skey[:-1][same]) and np.array_equal(skey[off[:-1][has]], record)
    assert sorted(zip(row.tolist(), skey.tolist())) == sorted(listed)
    assert no_values[2] is None and np.array_equal(_np(no_values[1]), swords)
    if name == "dense":
        assert not np.array_equal(swords, words) and np.mean(lens > 8) > 0.10


# ---- 4. writes are bounded by the caller's offsets and capacity, words and values both ----------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    sc = Scene(case("dense")[0])
    yield sc
    sc.close()


def _want_fill(want, offsets, size, capacity):
    blank = np.full(size + PAST, SENTINEL, u32)
    return clr.fill(want[0], want[1], offsets, blank, capacity=capacity), clr.fill(want[0], want[2], offsets, blank, capacity=capacity)


def _assert_bounded(sc, rows, want, offsets, size, capacity):
    _, words, vals = _fill(sc.raw, rows, offsets=offsets, size=size, capacity=capacity)
    want_words, want_vals = _want_fill(want, offsets, size, capacity)
    assert np.array_equal(words, want_words) and np.array_equal(vals, want_vals)
    only = _fill(sc.raw, rows, offsets=offsets, size=size, capacity=capacity, values=False)[1]
    assert np.array_equal(only, want_words)
    return words, vals


def test_offsets_from_smaller_counts_truncate_every_row_in_order(dense):
    rows, want = case("dense")[2], reference("dense")[0]
    short = olr.offsets_of(np.minimum(np.diff(want[0]), 3))
    total = int(short[-1])
    assert total < want[0][-1]
    words, vals = _assert_bounded(dense, rows, want, short, total, total)
    first3 = np.concatenate([np.arange(want[0][i], min(want[0][i] + 3, want[0][i + 1])) for i in range(len(rows))])      # every row's first three, in order
    assert np.array_equal(words[:total], want[1][first3]) and np.array_equal(vals[:total], clr.bits(want[2])[first3])
    assert np.all(words[total:] == SENTINEL) and np.all(vals[total:] == SENTINEL)


def test_a_capacity_below_the_total_keeps_everything_from_it_on(dense):
    rows, want = case("dense")[2], reference("dense")[0]
    want_off = want[0]
    total = int(want_off[-1])
    i = int(np.flatnonzero((np.diff(want_off) >= 3) & (want_off[:-1] >= total // 2))[0])
    half = int(want_off[i]) + 1      # inside the first row of three words or more past the middle
    assert np.any((want_off[:-1] < half) & (want_off[1:] > half))      # a row's segment straddles the capacity
    words, vals = _assert_bounded(dense, rows, want, want_off, total, half)
    assert np.array_equal(words[:half], want[1][:half]) and np.all(words[half:] == SENTINEL) and np.all(vals[half:] == SENTINEL)
    # a row whose segment starts at the capacity, and beyond it, writes nothing; capacity 0 writes nothing
    at = int(want_off[np.searchsorted(want_off, half)])
    words, vals = _assert_bounded(dense, rows, want, want_off, total, at)
    assert np.array_equal(vals[:at], clr.bits(want[2])[:at]) and np.all(words[at:] == SENTINEL) and np.all(vals[at:] == SENTINEL)
    words, vals = _assert_bounded(dense, rows, want, want_off, total, 0)
    assert np.all(words == SENTINEL) and np.all(vals == SENTINEL)


def test_a_segment_longer_than_the_row_keeps_its_tail_and_odd_offsets_write_nothing(dense):
    rows, want = case("dense")[2], reference("dense")[0]
    want_off = want[0]
    longer = olr.offsets_of(np.diff(want_off) + 1)      # every segment one longer than its row's list, the empty and the dead rows' too
    words, vals = _assert_bounded(dense, rows, want, longer, int(longer[-1]), int(longer[-1]))
    assert np.all(words[longer[1:] - 1] == SENTINEL) and np.count_nonzero(words == SENTINEL) == len(rows) + PAST
    assert np.all(vals[longer[1:] - 1] == SENTINEL) and np.count_nonzero(vals == SENTINEL) == len(rows) + PAST
    # offsets that run backwards, or lie below 0, are segments without room: nothing is written
    for odd in (want_off[::-1].copy(), want_off - want_off[-1] - 5):
        _, words, vals = _fill(dense.raw, rows, offsets=odd, size=int(want_off[-1]))
        assert np.all(words == SENTINEL) and np.all(vals == SENTINEL) and len(words) == int(want_off[-1]) + PAST


# ---- 5. streams and state -------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_and_another_stream_the_same(dense):
    rows = case("dense")[2]
    a = _fill(dense.raw, rows)
    b = _fill(dense.raw, rows)
    c = _fill(dense.raw, rows, stream=torch.cuda.Stream())
    for x in (b, c):
        assert all(np.array_equal(p, q) for p, q in zip(a, x))
    assert np.array_equal(_counts(dense.raw, rows), _counts(dense.raw, rows, stream=torch.cuda.Stream()))


def test_lists_follow_geometry_updated_in_place():
    moved, arrays, rows = case("update")
    text = moved.replace(UPDATE_MOVED[1], UPDATE_MOVED[0])
    assert moved != text
    sc = Scene(text)
    try:
        before = _fill(sc.raw, rows)
        m.update_spheres(sc.raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        d_rows, d_off = torch.from_numpy(rows).to(DEV), torch.from_numpy(before[0]).to(DEV)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.count_casts(sc.raw, d_rows)
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_cast_counts:")
        with pytest.raises(m.MirtError) as e:
            m.cast_list(sc.raw, d_rows, d_off, _buffer(int(before[0][-1])))
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_cast_list:")
        m.build_lbvh_karas(sc.raw)
        off, words = _assert_equals(sc.raw, rows, reference("update")[0])
        assert not (np.array_equal(off, before[0]) and np.array_equal(words, before[1][:len(words)]))
    finally:
        sc.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
TWINS = """png 8 8 twins.png
sphere 0 0 -4 1
sphere 0 0 -8 1
plane 0 1 0 3
"""


def test_argument_errors():
    raw = m.initRawConfigFromStl(m.parseText(TWINS), 0)
    try:
        n, cap = 8, 64
        Q = torch.zeros((4 * n, 8), dtype=torch.float32, device=DEV)
        Q[:, 3], Q[:, 6], Q[:, 7] = float("inf"), -1.0, 0.25      # (live balls through both spheres; the plane is never met)
        O = torch.arange(0, 8 * (4 * n + 1), 8, dtype=torch.int64, device=DEV)
        W, V, Cn = _buffer(4 * cap), _buffer(4 * cap), _buffer(4 * n)
        with pytest.raises(m.MirtError) as e:
            m.cast_list(raw, Q[:n], O[:n + 1], W[:cap], V[:cap].view(torch.float32))
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_cast_list:")
        with pytest.raises(m.MirtError) as e:
            m.count_casts(raw, Q[:n], Cn[:n])
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_cast_counts:")
        L = MOD.lib()
        # the state is checked before n: an unbuilt scene with n == 0 is MIRT_ERR_STATE as well
        assert L.mirt_cast_counts(raw._h, None, 0, None, 0, None) == 6 and L.mirt_cast_list(raw._h, None, 0, None, None, None, 0, 0, None) == 6
        m.build_lbvh_karas(raw)
        pQ, pO, pW, pV, pC = Q.data_ptr(), O.data_ptr(), W.data_ptr(), V.data_ptr(), Cn.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        # -- mirt_cast_counts
        def count(q=pQ, rows=n, c=pC, flags=0):
            return L.mirt_cast_counts(raw._h, vp(q), rows, vp(c), flags, None)

        def count_refused(**kw):
            return count(**kw) == 3 and m.lib().mirt_last_error().startswith(b"mirt_cast_counts:")

        assert count_refused(rows=-1) and all(count_refused(flags=f) for f in (1, 2, 0x80000000))
        assert count_refused(q=0) and count_refused(c=0) and count_refused(q=pQ + 4) and count_refused(q=pQ + 8) and count_refused(c=pC + 2)
        assert count_refused(c=pQ) and count_refused(c=pQ + 32 * n - 4) and count_refused(q=pC + 16)
        torch.cuda.synchronize()
        assert bool(torch.all(Cn == SENTINEL))      # nothing ran
        assert count(rows=0) == 0 and count(q=0, rows=0, c=0) == 0
        assert count(c=pC + 4 * n) == 0 and count(q=pQ + 32 * n, c=pC + 8 * n) == 0
        # touching ranges are not overlaps: the counts of rows 3n.. end where those rows begin (in the rows 2n..3n, not used again)
        assert count(q=pQ + 96 * n, c=pQ + 96 * n - 4 * n) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Cn[:n] == SENTINEL)) and bool(torch.all(Cn[n:3 * n] == 2)) and bool(torch.all(Cn[3 * n:] == SENTINEL))
        assert bool(torch.all(Q.view(torch.int32).reshape(-1)[24 * n - n:24 * n] == 2))

        # -- mirt_cast_list
        def call(q=pQ, rows=n, o=pO, w=pW, v=pV, capacity=cap, flags=0):
            return L.mirt_cast_list(raw._h, vp(q), rows, vp(o), vp(w), vp(v), capacity, flags, None)

        def refused(**kw):
            return call(**kw) == 3 and m.lib().mirt_last_error().startswith(b"mirt_cast_list:")

        assert refused(rows=-1) and refused(capacity=-1)
        for flags in (1, 2, 0x80000000):
            assert refused(flags=flags)
        assert refused(q=0) and refused(o=0) and refused(w=0) and refused(q=0, o=0, w=0, v=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(o=pO + 4) and refused(w=pW + 2) and refused(v=pV + 2)
        nq, no, nw = 32 * n, 8 * (n + 1), 4 * cap
        assert refused(o=pQ) and refused(o=pQ + nq - 8) and refused(q=pO)                                  # offsets over the rows
        assert refused(w=pQ) and refused(w=pQ + nq - 4) and refused(w=pQ - nw + 4)                         # words over the rows
        assert refused(w=pO) and refused(w=pO + no - 4) and refused(o=pW + nw - 8)                         # words over the offsets
        assert refused(v=pQ) and refused(v=pQ + nq - 4) and refused(v=pO) and refused(v=pO + no - 4)       # values over the rows, the offsets
        assert refused(v=pW) and refused(v=pW + nw - 4) and refused(v=pW - nw + 4)                         # values over the words
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(V == SENTINEL))      # nothing ran
        # no rows and no capacity are no work; with capacity 0 the words' and the values' pointers are no ranges
        assert call(rows=0) == 0 and call(q=0, rows=0, o=0, w=0, v=0, capacity=0) == 0 and call(w=0, v=0, capacity=0) == 0
        assert call(w=pQ, v=pQ, capacity=0) == 0 and call(rows=0, q=0, o=0) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(V == SENTINEL))
        # touching ranges are not overlaps; the values are optional
        written = 2 * n      # (segments of eight, two words each)
        assert call(v=pW + nw) == 0
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(W[:cap] != SENTINEL)) == written and int(torch.count_nonzero(W[cap:2 * cap] != SENTINEL)) == written
        assert bool(torch.all(W[2 * cap:] == SENTINEL)) and bool(torch.all(V == SENTINEL))
        W.fill_(SENTINEL)
        assert call(v=0) == 0 and call(q=pQ + nq, v=0) == 0      # (the values are optional; rows n..2n of Q are the same rows)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(W[:cap] != SENTINEL)) == written and bool(torch.all(W[cap:] == SENTINEL)) and bool(torch.all(V == SENTINEL))
        assert call() == 0
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(V[:cap] != SENTINEL)) == written and bool(torch.all(V[cap:] == SENTINEL))
        kind, pid = olr.unpack(_np(W[:2]))
        assert kind.tolist() == [1, 1] and sorted(pid.tolist()) == [0, 1] and sorted(V[:2].view(torch.float32).tolist()) == [2.75, 6.75]
    finally:
        raw.close()

"""Overlap lists on the GPU (include_ext/mirt_overlap_list.h: mirt_list_offsets, mirt_overlap_list; overlap_list.list_offsets,
overlap_list, overlap_lists, voxel_lists).  The yardsticks are np.cumsum for the offsets and tests/overlap_list_ref.py for the words:
the brute force's admitted set of every row in the oracle tree's leaf order, compared with np.array_equal, order included.  The
inputs are those tests/test_overlap_abi.py checks the restatement on."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
import overlap_list_ref as olr
import overlap_ref as ovr
from test_gpu_contacts import _scene      # (a built scene from its text)
from test_overlap_abi import CASES, CHOSEN_ROWS, MOVED, VOXEL_BOX, reference
from test_overlap_list_abi import list_reference

# (the package exports a function of the module's name, which `from cuda_ray_tracer_amd import overlap_list` would give)
overlap_list = importlib.import_module("cuda_ray_tracer_amd.overlap_list")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32
SENTINEL = 0x5eed5eed      # (no word: kind 1 with an id no test scene has)
PAST = 64                  # sentinel words past the end of every buffer of words


def _words_buffer(count):
    return torch.full((count,), SENTINEL, dtype=torch.int32, device=DEV)


def _np_words(t):
    return t.cpu().numpy().view(u32)


def _gpu_offsets(raw, d_rows):
    """The offsets of the GPU's own counts: count_overlaps through list_offsets."""
    return m.list_offsets(raw, m.count_overlaps(raw, d_rows))


def _fill(raw, rows, offsets=None, capacity=None, size=None, stream=None):
    """mirt_overlap_list on the rows (numpy [n, 8]) with the caller's offsets (numpy int64; None: the GPU's own) into a buffer of
    `size` words (None: the offsets' total) plus PAST sentinel words, the call's capacity being `capacity` (None: size).  Returns
    (offsets numpy, the whole buffer as uint32)."""
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    d_off = _gpu_offsets(raw, d_rows) if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(DEV)
    off = d_off.cpu().numpy()
    size = int(off[-1]) if size is None else size
    buf = _words_buffer(size + PAST)
    torch.cuda.synchronize()
    m.overlap_list(raw, d_rows, d_off, buf[:size if capacity is None else capacity], stream=stream)
    torch.cuda.synchronize()
    return off, _np_words(buf)


# ---- 1. offsets on synthetic counts: no scene walk, and no built scene ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def unbuilt():
    raw = m.initRawConfigFromStl(m.parseText(CASES["chosen"]()[0]), 0)
    yield raw
    raw.close()


def _offsets_equal_cumsum(raw, counts, stream=None):
    n = len(counts)
    d_counts = torch.from_numpy(counts.view(np.int32)).to(DEV)
    d_off = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    got = m.list_offsets(raw, d_counts, d_off[:n + 1], stream=stream)
    torch.cuda.synchronize()
    assert got.data_ptr() == d_off.data_ptr() and int(d_off[n + 1]) == -7
    want = olr.offsets_of(counts)
    assert want.dtype == np.int64 and np.array_equal(want[1:], np.cumsum(counts.astype(np.int64)))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(m.list_offsets(raw, d_counts).cpu().numpy(), want)      # (a tensor of its own)
    return want


# 2048 counts are one block's tile (one launch, no workspace); 256 * 2048 counts are as many block partials as the second level scans at once
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 65537, 256 * 2048 + 1])
def test_offsets_of_random_counts_equal_cumsum(unbuilt, n):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 40, n).astype(u32)
    counts[rng.random(n) < 0.3] = 0
    _offsets_equal_cumsum(unbuilt, counts)
    if n in (257, 65537):      # counts are unsigned 32-bit: values with bit 31 set, and the largest
        counts[rng.integers(0, n, 5)] = rng.integers(1 << 31, 1 << 32, 5).astype(u32)
        counts[n // 2] = 0xffffffff
        want = _offsets_equal_cumsum(unbuilt, counts, stream=torch.cuda.Stream())
        assert want[-1] > 1 << 32


def test_offsets_past_two_to_the_32_are_exact_and_zero_counts_are_zero(unbuilt):
    want = _offsets_equal_cumsum(unbuilt, np.full(65537, 70000, u32))
    assert want[-1] == 4587590000 and want[-1] > 1 << 32
    assert not np.any(_offsets_equal_cumsum(unbuilt, np.zeros(5000, u32)))
    assert m.list_offsets(unbuilt, torch.zeros(0, dtype=torch.int32, device=DEV)).cpu().tolist() == [0]


# ---- 2. the fill against the reference, order included ----------------------------------------------------------------------------------
def _assert_case(raw, name):
    _, rows = CASES[name]()
    want_off, want_words = list_reference(name)
    off, buf = _fill(raw, rows)
    assert np.array_equal(off, want_off)      # (the GPU's counts through the GPU's scan)
    total = int(off[-1])
    bad = np.flatnonzero(buf[:total] != want_words)
    assert len(bad) == 0, (name, len(bad), bad[:5], buf[bad[:5]], want_words[bad[:5]])
    assert np.array_equal(buf[:total], want_words) and np.all(buf[total:] == SENTINEL) and len(buf) == total + PAST
    return off, buf[:total]


@pytest.mark.parametrize("name", ["dense", "chosen", "far_1e5", "voxels", "empty", "plane_only", "single_triangle"])
def test_lists_equal_the_reference_in_the_reference_order(name):
    text, rows = CASES[name]()
    raw = _scene(text)
    try:
        off, words = _assert_case(raw, name)
    finally:
        raw.close()
    lens = np.diff(off)
    kind, _ = olr.unpack(words)
    if name == "dense":      # the case that matters: lists longer than the eight records of the record call
        assert np.mean(lens > 8) > 0.10 and set(kind.tolist()) == {1, 2, 3}
    if name == "chosen":
        assert lens[:len(CHOSEN_ROWS)].tolist() == [r[2] for r in CHOSEN_ROWS] and lens[17] == 7 and words[off[17]] == 3 << 30
    if name == "empty":
        assert len(words) == 0
    if name in ("plane_only", "single_triangle"):
        assert set(kind.tolist()) == ({3} if name == "plane_only" else {2}) and set(lens.tolist()) == {0, 1}
    dead = ~ovr.live_rows(rows)
    assert np.all(lens[dead] == 0)      # dead rows have empty segments


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, _ = CASES["deep_stack"]()
    raw = _scene(text)
    try:
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            raw.set_option("stack_lds_depth", depth)
        off, _ = _assert_case(raw, "deep_stack")
    finally:
        raw.close()
    assert np.diff(off).max() > 500


def test_more_rows_than_a_grid_of_lanes():
    text, base = CASES["mixed"]()
    want_off, want_words = list_reference("mixed")
    raw = _scene(text)
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37      # every lane takes a second row
        reps = -(-n // len(base))
        rows = np.tile(base, (reps, 1))[:n]
        lens = np.tile(np.diff(want_off), reps)[:n]
        off, buf = _fill(raw, rows)
        assert np.array_equal(off, olr.offsets_of(lens))
        whole = (n // len(base)) * len(want_words)
        assert np.array_equal(buf[:whole].reshape(n // len(base), -1), np.broadcast_to(want_words, (n // len(base), len(want_words))))
        assert np.array_equal(buf[whole:off[-1]], want_words[:off[-1] - whole]) and np.all(buf[off[-1]:] == SENTINEL)
    finally:
        raw.close()


# ---- 3. writes are bounded by the caller's offsets and capacity --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    text, rows = CASES["dense"]()
    raw = _scene(text)
    yield raw, rows
    raw.close()


def test_offsets_from_smaller_counts_truncate_every_row_in_order(dense):
    raw, rows = dense
    want_off, want_words = list_reference("dense")
    short = olr.offsets_of(np.minimum(np.diff(want_off), 3))
    off, buf = _fill(raw, rows, offsets=short)
    total = int(short[-1])
    assert total < want_off[-1]
    first3 = np.concatenate([want_words[want_off[i]:min(want_off[i] + 3, want_off[i + 1])] for i in range(len(rows))])      # every row's first three, in order
    assert np.array_equal(buf[:total], first3) and np.all(buf[total:] == SENTINEL)
    assert np.array_equal(buf, olr.fill(want_off, want_words, short, np.full(total + PAST, SENTINEL, u32), capacity=total))


def test_a_capacity_of_half_the_total_keeps_everything_from_it_on(dense):
    raw, rows = dense
    want_off, want_words = list_reference("dense")
    total = int(want_off[-1])
    half = total // 2
    assert np.any((want_off[:-1] < half) & (want_off[1:] > half))      # a row's segment straddles the capacity
    _, buf = _fill(raw, rows, offsets=want_off, capacity=half, size=total)
    assert np.array_equal(buf[:half], want_words[:half]) and np.all(buf[half:] == SENTINEL) and len(buf) == total + PAST
    # a row whose segment starts at the capacity, and beyond it, writes nothing; capacity 0 writes nothing
    at = int(want_off[np.searchsorted(want_off, half)])
    _, buf = _fill(raw, rows, offsets=want_off, capacity=at, size=total)
    assert np.array_equal(buf[:at], want_words[:at]) and np.all(buf[at:] == SENTINEL)
    _, buf = _fill(raw, rows, offsets=want_off, capacity=0, size=total)
    assert np.all(buf == SENTINEL)


def test_a_segment_longer_than_the_row_keeps_its_tail(dense):
    raw, rows = dense
    want_off, want_words = list_reference("dense")
    lens = np.diff(want_off)
    longer = olr.offsets_of(lens + 1)      # every segment one longer than its row's list, the empty rows' too
    off, buf = _fill(raw, rows, offsets=longer)
    want = olr.fill(want_off, want_words, longer, np.full(int(longer[-1]) + PAST, SENTINEL, u32), capacity=int(longer[-1]))
    assert np.array_equal(buf, want)
    assert np.all(buf[longer[1:] - 1] == SENTINEL) and np.count_nonzero(buf == SENTINEL) == len(rows) + PAST
    # offsets that run backwards, or lie below 0, are segments without room: nothing is written
    for odd in (want_off[::-1].copy(), want_off - want_off[-1] - 5):
        _, buf = _fill(raw, rows, offsets=odd, size=int(want_off[-1]))
        assert np.all(buf == SENTINEL) and len(buf) == int(want_off[-1]) + PAST


# ---- 4. further properties ------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_and_another_stream_the_same(dense):
    raw, rows = dense
    _, a = _fill(raw, rows)
    _, b = _fill(raw, rows)
    _, c = _fill(raw, rows, stream=torch.cuda.Stream())
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_overlap_lists_unsorted_and_sorted(dense):
    raw, rows = dense
    want_off, want_words = list_reference("dense")
    d_rows = torch.from_numpy(rows).to(DEV)
    off, words = m.overlap_lists(raw, d_rows)
    assert off.dtype == torch.int64 and words.dtype == torch.int32 and words.shape == (int(want_off[-1]),)
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(_np_words(words), want_words)
    off_s, sorted_words = m.overlap_lists(raw, d_rows, sort=True)
    got = _np_words(sorted_words)
    assert np.array_equal(off_s.cpu().numpy(), want_off)
    want = np.concatenate([np.sort(want_words[want_off[i]:want_off[i + 1]]) for i in range(len(rows))])
    assert np.array_equal(got, want) and not np.array_equal(got, want_words)
    row = np.repeat(np.arange(len(rows)), np.diff(want_off))
    same = row[1:] == row[:-1]
    assert np.all(got[1:][same] > got[:-1][same])      # each segment ascends strictly: no surface twice
    kind, pid = m.unpack_words(sorted_words)
    assert np.array_equal(kind.cpu().numpy(), olr.unpack(want)[0]) and np.array_equal(pid.cpu().numpy(), olr.unpack(want)[1])
    on_stream = m.overlap_lists(raw, d_rows, sort=True, stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert np.array_equal(_np_words(on_stream[1]), want)


def test_voxel_lists_agree_with_the_occupancy_grid():
    text, _ = CASES["voxels"]()
    want_off, want_words = list_reference("voxels")
    raw = _scene(text)
    try:
        off, words = m.voxel_lists(raw, *VOXEL_BOX)
        grid = m.occupancy_grid(raw, *VOXEL_BOX)
        off_s, words_s = m.voxel_lists(raw, *VOXEL_BOX, sort=True)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(_np_words(words), want_words)
    assert np.array_equal((np.diff(off.cpu().numpy()) > 0).reshape(16, 16, 16), grid.cpu().numpy())      # non-empty exactly where occupied
    assert np.array_equal(off_s.cpu().numpy(), want_off) and np.array_equal(np.sort(_np_words(words_s)), np.sort(want_words))
    assert 0.05 < grid.float().mean().item() < 0.5


# ---- 5. after an update in place and a rebuild ------------------------------------------------------------------------------------------
def test_lists_follow_geometry_updated_in_place():
    moved, rows = CASES["moved"]()
    text = moved.replace(MOVED[1], MOVED[0])
    assert text != moved
    raw = _scene(text)
    try:
        before_off, before = _fill(raw, rows)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        d_rows = torch.from_numpy(rows).to(DEV)
        d_off = torch.from_numpy(before_off).to(DEV)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.overlap_list(raw, d_rows, d_off, _words_buffer(int(before_off[-1])))
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_overlap_list:")
        assert np.array_equal(m.list_offsets(raw, torch.ones(3, dtype=torch.int32, device=DEV)).cpu().numpy(), [0, 1, 2, 3])      # (needs no built scene)
        m.build_lbvh_karas(raw)
        off, words = _assert_case(raw, "moved")
    finally:
        raw.close()
    assert not (np.array_equal(off, before_off) and np.array_equal(words, before[:len(words)]))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_both_calls():
    import light_scenes
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n, cap = 8, 64
        Q = torch.zeros((4 * n, 8), dtype=torch.float32, device=DEV)
        Q[:, 0:3], Q[:, 4:7] = -100.0, 100.0      # (live rows that hold the whole scene)
        O = torch.arange(0, 8 * (4 * n + 1), 8, dtype=torch.int64, device=DEV)
        W = torch.full((4 * cap,), SENTINEL, dtype=torch.int32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.overlap_list(raw, Q[:n], O[:n + 1], W[:cap])
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_overlap_list:")
        m.build_lbvh_karas(raw)
        L = overlap_list.lib()
        pQ, pO, pW = Q.data_ptr(), O.data_ptr(), W.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def fill(q=pQ, count=n, o=pO, w=pW, capacity=cap):
            return L.mirt_overlap_list(raw._h, vp(q), count, vp(o), vp(w), capacity, None)

        def refused(call, who, **kw):
            rc = call(**kw)
            return rc == 3 and m.lib().mirt_last_error().startswith(who + b":")

        who = b"mirt_overlap_list"
        assert refused(fill, who, count=-1) and refused(fill, who, capacity=-1)
        assert refused(fill, who, q=0) and refused(fill, who, o=0) and refused(fill, who, w=0) and refused(fill, who, q=0, o=0, w=0)
        assert refused(fill, who, q=pQ + 4) and refused(fill, who, q=pQ + 8) and refused(fill, who, o=pO + 4) and refused(fill, who, w=pW + 2)
        nq, no, nw = 32 * n, 8 * (n + 1), 4 * cap
        assert refused(fill, who, o=pQ) and refused(fill, who, o=pQ + nq - 8) and refused(fill, who, q=pO)      # offsets over the boxes
        assert refused(fill, who, w=pQ) and refused(fill, who, w=pQ + nq - 4) and refused(fill, who, w=pQ - nw + 4)      # words over the boxes
        assert refused(fill, who, w=pO) and refused(fill, who, w=pO + no - 4) and refused(fill, who, o=pW + nw - 8)      # words over the offsets
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL))      # nothing ran
        # n == 0 and capacity == 0 are no work; adjacent is not overlapping; with capacity 0 the words' pointer is no range
        assert fill(count=0) == 0 and fill(q=0, count=0, o=0, w=0, capacity=0) == 0 and fill(w=0, capacity=0) == 0 and fill(w=pQ, capacity=0) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL))
        # ... and offsets that are no offsets (the rows after the boxes, read as int64) write nowhere but inside [0, capacity)
        assert fill(w=pQ + nq, capacity=8) == 0 and fill(o=pQ + nq) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(W[cap:] == SENTINEL))
        W.fill_(SENTINEL)
        counts = m.count_overlaps(raw, Q[:n]).cpu().numpy()
        assert fill() == 0
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(W[:cap] != SENTINEL)) == int(np.minimum(counts, 8).sum()) > 0 and bool(torch.all(W[cap:] == SENTINEL))

        # mirt_list_offsets
        big = 4096      # (two tiles: the call needs a workspace)
        Cn = torch.ones(4 * big, dtype=torch.int32, device=DEV)      # (the counts, and room for offsets right after them)
        D = torch.full((2 * big + 2,), -7, dtype=torch.int64, device=DEV)
        Wk = torch.full((16,), -7, dtype=torch.int64, device=DEV)
        pC, pD, pK = Cn.data_ptr(), D.data_ptr(), Wk.data_ptr()
        assert m.list_offsets_work_bytes(big) == 16 and m.list_offsets_work_bytes(n) == 0

        def scan(c=pC, count=big, d=pD, k=pK):
            return L.mirt_list_offsets(raw._h, vp(c), count, vp(d), vp(k), None)

        who = b"mirt_list_offsets"
        assert refused(scan, who, count=-1) and refused(scan, who, count=(1 << 40) + 1)
        assert refused(scan, who, d=0) and refused(scan, who, c=0) and refused(scan, who, k=0) and refused(scan, who, c=0, count=n)
        assert refused(scan, who, c=pC + 2) and refused(scan, who, d=pD + 4) and refused(scan, who, k=pK + 4)
        assert refused(scan, who, d=pC) and refused(scan, who, d=pC + 4 * big - 8) and refused(scan, who, c=pD + 8 * big)      # offsets over the counts
        assert refused(scan, who, k=pC) and refused(scan, who, k=pC + 4 * big - 8) and refused(scan, who, k=pD + 8 * big)      # the workspace over either
        torch.cuda.synchronize()
        assert bool(torch.all(D == -7)) and bool(torch.all(Wk == -7))      # nothing ran
        # a small n needs no workspace, and its pointer is then no range; n == 0 writes the total alone
        assert scan(count=n, k=0) == 0 and scan(count=n, k=pC) == 0 and scan(count=0, c=0, d=pD + 8 * (n + 2), k=0) == 0
        torch.cuda.synchronize()
        assert D[:n + 1].tolist() == list(range(n + 1)) and int(D[n + 1]) == -7 and int(D[n + 2]) == 0 and int(D[n + 3]) == -7
        assert scan(d=pC + 4 * big) == 0 and scan() == 0      # adjacent is not overlapping
        torch.cuda.synchronize()
        assert Cn.view(torch.int64)[big // 2:big // 2 + big + 1].tolist() == list(range(big + 1)) and bool(torch.all(Cn[:big] == 1))
        assert D[:big + 1].tolist() == list(range(big + 1)) and int(D[big + 1]) == -7 and bool(torch.all(Wk[2:] == -7))
    finally:
        raw.close()

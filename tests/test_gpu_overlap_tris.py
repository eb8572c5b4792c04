"""Triangle overlap queries on the GPU (include_ext2/mirt_overlap_tris.h: mirt_overlap_triangles, mirt_triangle_list;
overlap_tris.overlap_triangles, triangle_list, triangle_lists, scene_triangle_rows).  The yardstick is tests/overlap_tris_ref.py: the
brute force's admitted set of every row in the oracle tree's leaf order, compared with np.array_equal, order included.  The inputs
are those tests/test_overlap_tris_abi.py checks the restatement on."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
import overlap_list_ref as olr
import overlap_tris_ref as otr
from test_gpu_contacts import _scene      # (a built scene from its text)
from test_overlap_tris_abi import CASES, HAND_ROWS, MOVED_TRI, _well_shaped_scene, reference

overlap_tris = importlib.import_module("cuda_ray_tracer_amd.overlap_tris")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32
SENTINEL = 0x5eed5eed      # (no word: kind 1 with an id no test scene has)
PAST = 64                  # sentinel words past the end of every buffer of words


def _np_words(t):
    return t.cpu().numpy().view(u32)


def _rows(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)


def _counts(raw, rows, any=False, stream=None):
    """mirt_overlap_triangles on the rows (numpy [n, 9]): uint32 [n]; the count after the last keeps its sentinel."""
    n = len(rows)
    d_rows = _rows(rows)
    out = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    got = m.overlap_triangles(raw, d_rows, out[:n], any=any, stream=stream)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and int(out[n]) == -7
    return out[:n].cpu().numpy().view(u32)


def _fill(raw, rows, offsets, capacity=None, size=None, stream=None):
    """mirt_triangle_list on the rows with the caller's offsets (numpy int64) into a buffer of `size` words (None: the offsets'
    total) plus PAST sentinel words, the call's capacity being `capacity` (None: size).  Returns the whole buffer as uint32."""
    d_rows = _rows(rows)
    d_off = torch.from_numpy(np.array(offsets, np.int64)).to(DEV)      # (a copy: the reference's arrays are read-only)
    size = int(offsets[-1]) if size is None else size
    buf = torch.full((size + PAST,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    m.triangle_list(raw, d_rows, d_off, buf[:size if capacity is None else capacity], stream=stream)
    torch.cuda.synchronize()
    return _np_words(buf)


def _assert_case(raw, name):
    """Counts, any-counts and the filled list of a case against the reference, the offsets from the GPU's own counts."""
    _, rows = CASES[name]()
    want_counts, want_off, want_words = reference(name)
    counts = _counts(raw, rows)
    bad = np.flatnonzero(counts != want_counts)
    assert len(bad) == 0, (name, len(bad), bad[:5], counts[bad[:5]], want_counts[bad[:5]])
    assert np.array_equal(_counts(raw, rows, any=True), np.minimum(want_counts, 1))
    off = m.list_offsets(raw, torch.from_numpy(counts.view(np.int32)).to(DEV)).cpu().numpy()
    assert np.array_equal(off, want_off)
    buf = _fill(raw, rows, off)
    total = int(off[-1])
    bad = np.flatnonzero(buf[:total] != want_words)
    assert len(bad) == 0, (name, len(bad), bad[:5], buf[bad[:5]], want_words[bad[:5]])
    assert np.all(buf[total:] == SENTINEL) and len(buf) == total + PAST
    return counts, off, buf[:total]


# ---- 1. counts and lists against the reference, order included --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand", "dense", "far_1e5", "empty", "plane_only", "single_triangle"])
def test_counts_and_lists_equal_the_reference_in_the_reference_order(name):
    text, rows = CASES[name]()
    raw = _scene(text)
    try:
        counts, off, words = _assert_case(raw, name)
    finally:
        raw.close()
    kind, _ = olr.unpack(words)
    if name == "hand":
        assert counts.tolist() == [r[3] for r in HAND_ROWS]
    if name == "dense":
        assert np.mean(counts > 0) >= 0.10 and set(kind.tolist()) == {1, 2, 3} and counts.max() > 8
    if name == "empty":
        assert len(words) == 0
    if name in ("plane_only", "single_triangle"):
        assert set(kind.tolist()) == ({3} if name == "plane_only" else {2})
    assert np.all(counts[~otr.live_rows(rows)] == 0)      # dead rows count 0 and have empty segments


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, _ = CASES["deep_stack"]()
    raw = _scene(text)
    try:
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            raw.set_option("stack_lds_depth", depth)
        counts, _, _ = _assert_case(raw, "deep_stack")
    finally:
        raw.close()
    assert counts.max() > 500


def test_a_mesh_against_itself_lists_every_triangle_that_shares_a_vertex():
    text, rows = CASES["mesh"]()
    raw = _scene(text)
    try:
        d_rows = m.scene_triangle_rows(raw)
        assert np.array_equal(d_rows.cpu().numpy(), rows)
        part = m.scene_triangle_rows(raw, first=3, count=4)
        assert np.array_equal(part.cpu().numpy(), rows[3:7]) and m.scene_triangle_rows(raw, first=len(rows)).shape == (0, 9)
        off, words = m.triangle_lists(raw, d_rows)
        torch.cuda.synchronize()
        _assert_case(raw, "mesh")
    finally:
        raw.close()
    want_counts, want_off, want_words = reference("mesh")
    off, words = off.cpu().numpy(), _np_words(words)
    assert np.array_equal(off, want_off) and np.array_equal(words, want_words)
    v = rows.reshape(-1, 3, 3)
    for i in range(len(v)):
        mine = set(words[off[i]:off[i + 1]].tolist())
        assert int(olr.word(2, i)) in mine, i
        for j in range(len(v)):
            if any(np.array_equal(p, q) for p in v[i] for q in v[j]):
                assert int(olr.word(2, j)) in mine, (i, j)


# ---- 2. writes are bounded by the caller's offsets and capacity --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    text, rows = CASES["dense"]()
    raw = _scene(text)
    yield raw, rows
    raw.close()


def test_offsets_from_other_counts_truncate_rows_and_keep_tails(dense):
    raw, rows = dense
    _, want_off, want_words = reference("dense")
    lens = np.diff(want_off)
    for other in (olr.offsets_of(np.minimum(lens, 3)), olr.offsets_of(lens + 1)):      # (shorter segments; one longer than every list, a dead row's too)
        total = int(other[-1])
        buf = _fill(raw, rows, other)
        assert np.array_equal(buf, olr.fill(want_off, want_words, other, np.full(total + PAST, SENTINEL, u32), capacity=total))
    assert np.all(buf[other[1:] - 1] == SENTINEL)      # every tail word stays, a dead row's whole segment
    # offsets that run backwards, or lie below 0, are segments without room: nothing is written
    for odd in (want_off[::-1].copy(), want_off - want_off[-1] - 5):
        buf = _fill(raw, rows, odd, size=int(want_off[-1]))
        assert np.all(buf == SENTINEL)


def test_a_capacity_below_the_total_keeps_everything_from_it_on(dense):
    raw, rows = dense
    _, want_off, want_words = reference("dense")
    total = int(want_off[-1])
    half = total // 2
    assert np.any((want_off[:-1] < half) & (want_off[1:] > half))      # a row's segment straddles the capacity
    buf = _fill(raw, rows, want_off, capacity=half, size=total)
    assert np.array_equal(buf[:half], want_words[:half]) and np.all(buf[half:] == SENTINEL) and len(buf) == total + PAST
    buf = _fill(raw, rows, want_off, capacity=0, size=total)
    assert np.all(buf == SENTINEL)


def test_another_stream_gives_the_same_bytes(dense):
    raw, rows = dense
    want_counts, want_off, want_words = reference("dense")
    s = torch.cuda.Stream()
    assert np.array_equal(_counts(raw, rows, stream=s), want_counts)
    assert np.array_equal(_counts(raw, rows, any=True, stream=s), np.minimum(want_counts, 1))
    buf = _fill(raw, rows, want_off, stream=s)
    assert np.array_equal(buf[:len(want_words)], want_words) and np.all(buf[len(want_words):] == SENTINEL)
    off, words = m.triangle_lists(raw, _rows(rows), sort=True, stream=s)
    torch.cuda.synchronize()
    want = np.concatenate([np.sort(want_words[want_off[i]:want_off[i + 1]]) for i in range(len(rows))])
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(_np_words(words), want)


# ---- 3. after an update in place and a rebuild ------------------------------------------------------------------------------------------
def test_lists_follow_geometry_updated_in_place():
    _, rows = CASES["moved"]()
    raw = _scene(_well_shaped_scene())
    try:
        before = _counts(raw, rows)
        m.update_triangles(raw, torch.from_numpy(MOVED_TRI).to(DEV), first=0)
        d_rows, n = _rows(rows), len(rows)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.overlap_triangles(raw, d_rows)
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_overlap_triangles:")
        with pytest.raises(m.MirtError) as e:
            m.triangle_list(raw, d_rows, torch.zeros(n + 1, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV))
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_triangle_list:")
        m.build_lbvh_karas(raw)
        counts, _, _ = _assert_case(raw, "moved")
    finally:
        raw.close()
    assert not np.array_equal(counts, before) and counts[-1] >= 1      # (the last row is the moved triangle itself)


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_both_calls():
    text, _ = CASES["hand"]()
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    try:
        n, cap = 8, 64
        T = torch.zeros((4 * n, 9), dtype=torch.float32, device=DEV)
        T[:, 0:3], T[:, 3:6], T[:, 6:9] = torch.tensor([1.0, 1, 2]), torch.tensor([0.0, 0, -10]), torch.tensor([2.0, 1, 2])      # (the row that touches two)
        Cn = torch.full((4 * n,), -7, dtype=torch.int32, device=DEV)
        O = torch.arange(0, 8 * (4 * n + 1), 8, dtype=torch.int64, device=DEV)
        W = torch.full((4 * cap,), SENTINEL, dtype=torch.int32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.overlap_triangles(raw, T[:n], Cn[:n])
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_overlap_triangles:")
        m.build_lbvh_karas(raw)
        L = overlap_tris.lib()
        pT, pC, pO, pW = T.data_ptr(), Cn.data_ptr(), O.data_ptr(), W.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def count(t=pT, rows=n, c=pC, flags=0):
            return L.mirt_overlap_triangles(raw._h, vp(t), rows, vp(c), flags, None)

        def fill(t=pT, rows=n, o=pO, w=pW, capacity=cap):
            return L.mirt_triangle_list(raw._h, vp(t), rows, vp(o), vp(w), capacity, None)

        def refused(call, who, **kw):
            return call(**kw) == 3 and m.lib().mirt_last_error().startswith(who + b":")

        who = b"mirt_overlap_triangles"
        assert refused(count, who, rows=-1) and refused(count, who, flags=2) and refused(count, who, flags=0x80000001)
        assert refused(count, who, t=0) and refused(count, who, c=0) and refused(count, who, t=pT + 2) and refused(count, who, c=pC + 1)
        assert refused(count, who, c=pT) and refused(count, who, c=pT + 36 * n - 4) and refused(count, who, t=pC + 4 * n - 4)
        who = b"mirt_triangle_list"
        assert refused(fill, who, rows=-1) and refused(fill, who, capacity=-1)
        assert refused(fill, who, t=0) and refused(fill, who, o=0) and refused(fill, who, w=0)
        assert refused(fill, who, t=pT + 2) and refused(fill, who, o=pO + 4) and refused(fill, who, w=pW + 2)
        assert refused(fill, who, o=pT) and refused(fill, who, w=pT + 36 * n - 4) and refused(fill, who, w=pO) and refused(fill, who, o=pW + 4 * cap - 8)
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(Cn == -7))      # nothing ran
        # n == 0 and capacity == 0 are no work; rows need 4-byte alignment only; adjacent is not overlapping
        assert count(rows=0) == 0 and count(t=0, rows=0, c=0) == 0 and fill(rows=0) == 0 and fill(t=0, rows=0, o=0, w=0, capacity=0) == 0 and fill(w=0, capacity=0) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(Cn == -7))
        assert count(t=pT + 36, c=pC + 4, rows=n) == 0 and count(c=pT + 36 * n, rows=n) == 0
        torch.cuda.synchronize()
        assert Cn[1:n + 1].tolist() == [2] * n and int(Cn[0]) == -7 and T.view(torch.int32).reshape(-1)[9 * n:10 * n].tolist() == [2] * n
        assert fill() == 0      # offsets 0, 8, 16, ...: each row writes its two words and keeps its tail
        torch.cuda.synchronize()
        got = _np_words(W)
        assert np.count_nonzero(got[:cap] != SENTINEL) == 2 * n and np.all(got[cap:] == SENTINEL)
        assert sorted(got[:2].tolist()) == [int(olr.word(1, 0)), int(olr.word(2, 0))] and got[2] == SENTINEL and got[8:10].tolist() == got[:2].tolist()
    finally:
        raw.close()

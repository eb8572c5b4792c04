"""Ray and ball lists on the GPU (include_ext/mirt_query_lists.h: mirt_ray_list, mirt_ball_list; query_lists.ray_list, ball_list,
ray_lists, ball_lists).  The yardstick is tests/query_lists_ref.py: the record references' admitted set of every row in the
oracle tree's leaf order, with the t or dist of each, compared with np.array_equal on the words and on the values' bits, order
included.  The inputs are those tests/test_multihit_abi.py and tests/test_contacts_abi.py check the restatements on.  Then the GPU
against itself: every sorted row begins with the record call's eight records."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import query_lists
import contacts_ref as kr
import closest_ref as cr
import edge_scenes
import multihit_ref as mr
import overlap_list_ref as olr
import query_lists_ref as qlr
import test_contacts_abi as tca
import test_multihit_abi as tma
from test_gpu_multihit import Scene      # (a built scene with its host arrays and the library's tree)
from test_query_lists_abi import ball_reference, ray_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32
SENTINEL = 0x5eed5eed      # (no word: kind 1 with an id no test scene has; as a value's bits, a float no test computes)
PAST = 64                  # sentinel entries past the end of every array of words and of values

RAY_CASES, BALL_CASES = list(tma.CASES), list(tca.CASES)
KINDS = {"ray": (m.count_hits, m.ray_list, m.ray_lists), "ball": (m.count_within, m.ball_list, m.ball_lists)}


def case(kind, name):
    """(scene text, rows, (offsets, words, values) of the reference)."""
    if kind == "ray":
        return tma.case_input(name) + (ray_reference(name),)
    return tuple(tca.CASES[name]()) + (ball_reference(name),)


def _buffer(count):
    return torch.full((count,), SENTINEL, dtype=torch.int32, device=DEV)


def _np(t):
    return t.cpu().numpy().view(u32)


def _fill(kind, raw, rows, offsets=None, capacity=None, size=None, values=True, stream=None):
    """The fill on the rows (numpy) with the caller's offsets (numpy int64; None: the GPU's own counts through the GPU's scan) into
    arrays of `size` entries (None: the offsets' total) plus PAST sentinel entries, the call's capacity being `capacity` (None:
    size).  Returns (offsets numpy, the whole array of words as uint32, the whole array of values as uint32 bits or None)."""
    count, fill, _ = KINDS[kind]
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    d_off = m.list_offsets(raw, count(raw, d_rows)) if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(DEV)
    off = d_off.cpu().numpy()
    size = int(off[-1]) if size is None else size
    cap = size if capacity is None else capacity
    words, vals = _buffer(size + PAST), (_buffer(size + PAST) if values else None)
    torch.cuda.synchronize()
    fill(raw, d_rows, d_off, words[:cap], vals[:cap].view(torch.float32) if values else None, stream=stream)
    torch.cuda.synchronize()
    return off, _np(words), (_np(vals) if values else None)


def _assert_equals(kind, raw, rows, want, **kw):
    """With the value array and without it: the offsets, the words, the values' bits, the sentinels past the end."""
    want_off, want_words, want_vals = want
    total = int(want_off[-1])
    for values in (True, False):
        off, words, vals = _fill(kind, raw, rows, values=values, **kw)
        assert np.array_equal(off, want_off)      # (the GPU's counts through the GPU's scan)
        bad = np.flatnonzero(words[:total] != want_words)
        assert len(bad) == 0, (kind, len(bad), bad[:5], words[bad[:5]], want_words[bad[:5]])
        assert len(words) == total + PAST and np.all(words[total:] == SENTINEL)
        if values:
            assert np.array_equal(vals[:total], qlr.bits(want_vals)) and len(vals) == total + PAST and np.all(vals[total:] == SENTINEL)
    return off, words[:total]


def _library_reference(kind, sc, rows):
    """The reference over the library's own tree (scenes the ABI tests hold no reference of)."""
    if kind == "ray":
        return qlr.ray_lists(sc.refs, mr.admitted(sc.arrays, rows, sc.nodes, sc.refs))
    return qlr.ball_lists(sc.arrays, rows, sc.refs)


# ---- 1. against the reference, order included ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("ray", n) for n in RAY_CASES] + [("ball", n) for n in BALL_CASES])
def test_lists_equal_the_reference_in_the_reference_order(kind, name):
    text, rows, want = case(kind, name)
    sc = Scene(text)
    try:
        off, words = _assert_equals(kind, sc.raw, rows, want)
    finally:
        sc.close()
    lens = np.diff(off)
    kinds = set(olr.unpack(words)[0].tolist())
    if name in ("A_inf", "dense"):      # the cases that matter: lists longer than the eight records of the record calls
        assert np.mean(lens > 8) > 0.10 and kinds == {1, 2, 3} and np.any(lens == 0)
    if name in ("C", "deep_stack"):
        assert np.all(lens == 600)


# ---- 2. the GPU against itself: a sorted row begins with the record call's records ---------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("ray", "A_inf"), ("ball", "dense")])
def test_sorted_rows_begin_with_the_record_calls_records(kind, name):
    text, rows, want = case(kind, name)
    n = len(rows)
    sc = Scene(text)
    try:
        d_rows = torch.from_numpy(rows).to(DEV)
        hits = torch.full((n, 8, 6), -7, dtype=torch.int32, device=DEV)
        counts = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        (m.trace_rays_multi if kind == "ray" else m.closest_points_multi)(sc.raw, d_rows, hits, counts)
        off, words, vals = KINDS[kind][2](sc.raw, d_rows, sort=True)
        plain = KINDS[kind][2](sc.raw, d_rows)
        no_values = KINDS[kind][2](sc.raw, d_rows, values=False, sort=True, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
    finally:
        sc.close()
    hits, counts, off = _np(hits), _np(counts).astype(np.int64), off.cpu().numpy()
    assert off.dtype == np.int64 and words.dtype == torch.int32 and vals.dtype == torch.float32
    assert np.array_equal(np.diff(off), counts) and np.array_equal(off, want[0])      # every row's length is the record call's count
    words, vals = _np(words), _np(vals.view(torch.int32))
    kind_of, pid = olr.unpack(words)
    for j in range(8):
        has = np.flatnonzero(counts > j)
        at = off[:-1][has] + j
        assert np.array_equal(vals[at], hits[has, j, 0]) and np.array_equal(kind_of[at], hits[has, j, 1]) and np.array_equal(pid[at], hits[has, j, 2]), j
        assert np.all(hits[np.flatnonzero(counts <= j), j, 1] == 0)
    assert np.mean(counts > 8) > 0.10
    # every segment ascends by value; the unsorted call is the reference; values=False gives the same words and no values
    row = np.repeat(np.arange(n), counts)
    same = row[1:] == row[:-1]
    assert np.all(vals[1:][same] >= vals[:-1][same])
    assert np.array_equal(_np(plain[1]), want[1]) and np.array_equal(_np(plain[2].view(torch.int32)), qlr.bits(want[2]))
    assert no_values[2] is None and np.array_equal(_np(no_values[1]), words) and not np.array_equal(words, want[1])


# ---- 3. the smallest scenes, the duplicated sphere, rows that are not live --------------------------------------------------------------
def _small_rows(kind):
    rng = np.random.default_rng(5)
    n = 300
    o = rng.uniform(-1.5, 1.5, (n, 3))
    if kind == "ray":
        target = np.array([0, 0, -2.0]) + rng.normal(size=(n, 3)) * 0.6
        rays = tma.pack(o.astype(f32), (target - o).astype(f32), tma.INF)
        rays[:20, 0:3] = np.array([0.1, 0.2, -2.1], f32)      # from inside the sphere of single_sphere
        rays[::7, 3] = 2.0
        return rays
    q = rng.uniform(-3, 3, (n, 3)).astype(f32)
    return np.concatenate([q, np.exp(rng.uniform(np.log(0.1), np.log(8.0), (n, 1))).astype(f32)], axis=1)


@pytest.mark.parametrize("kind", ["ray", "ball"])
@pytest.mark.parametrize("name", ["empty", "plane_only", "single_sphere", "single_triangle"])
def test_smallest_scenes(kind, name):
    rows = _small_rows(kind)
    sc = Scene(edge_scenes.ALL[name]())
    try:
        want = _library_reference(kind, sc, rows)
        off, words = _assert_equals(kind, sc.raw, rows, want)
    finally:
        sc.close()
    kinds = set(olr.unpack(words)[0].tolist())
    assert kinds == {"empty": set(), "plane_only": {3}, "single_sphere": {1}, "single_triangle": {2}}[name]
    assert np.diff(off).max() == (0 if name == "empty" else 1)


def test_the_duplicated_sphere_is_listed_twice_in_leaf_order():
    sc = Scene(tma.TWINS)
    try:
        rays = tma.twin_rays()
        want = _library_reference("ray", sc, rays)
        off, words = _assert_equals("ray", sc.raw, rays, want)
        order = [int(i) for i in sc.refs["id"] if i in (1, 3)]
        balls = np.array([(0, 0, -4, 1.5), (0.1, 0.05, -3.5, 2.0), (0, 9, 0, 1.0)], f32)
        boff, bwords = _assert_equals("ball", sc.raw, balls, _library_reference("ball", sc, balls))
    finally:
        sc.close()
    assert np.diff(off).tolist() == [2, 2, 0]
    for r in (0, 1):
        kind, pid = olr.unpack(words[off[r]:off[r + 1]])
        assert kind.tolist() == [1, 1] and pid.tolist() == order
    pid = olr.unpack(bwords[boff[0]:boff[1]])[1].tolist()
    assert [i for i in pid if i in (1, 3)] == order and np.diff(boff)[2] == 0


@pytest.fixture(scope="module")
def dense():
    sc = Scene(tma.dense_scene_text())
    yield sc
    sc.close()


def test_rows_that_are_not_live_have_empty_segments_among_live_rows(dense):
    rays = tma.case_input("A_inf")[1][:512].copy()
    rays[0::8, 3] = 0.0
    rays[1::8, 3] = -1.0
    rays[2::8, 3] = np.nan
    rays[3::8, 4:7] = 0.0
    rays[4::16, 4:7] = np.nan
    rays[12::16, 4:7] = [1e-8, 0, 0]
    dead = ~mr.split(rays)[3]
    assert dead.sum() == 5 * 64 and not np.all(dead.reshape(-1, 64), axis=1).any()      # mixed into every wave
    off, _ = _assert_equals("ray", dense.raw, rays, _library_reference("ray", dense, rays))
    assert np.all(np.diff(off)[dead] == 0) and np.diff(off)[~dead].sum() > 200
    balls = tca.CASES["dense"]()[1][:512].copy()
    balls[:, 3] = 1.0
    balls[0::8, 3] = 0.0
    balls[1::8, 3] = -1.0
    balls[2::8, 3] = np.nan
    balls[3::8, 0] = np.inf
    balls[4::16, 1] = np.nan
    balls[12::16, 2] = -np.inf
    dead = ~cr.live_rows(balls)
    assert dead.sum() == 5 * 64
    off, _ = _assert_equals("ball", dense.raw, balls, _library_reference("ball", dense, balls))
    assert np.all(np.diff(off)[dead] == 0) and np.diff(off)[~dead].sum() > 200
    # a dead row does not need its offsets: with offsets that give the dead rows room, nothing of theirs is written
    lens = np.diff(off) + dead * 5
    got = _fill("ball", dense.raw, balls, offsets=olr.offsets_of(lens))[1]
    assert np.count_nonzero(got != SENTINEL) == np.diff(off).sum()


# ---- 4. the spill path; more rows than a grid of lanes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("ray", "C"), ("ball", "deep_stack")])
@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(kind, name, depth):
    text, rows, want = case(kind, name)
    sc = Scene(text)
    try:
        assert sc.raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            sc.raw.set_option("stack_lds_depth", depth)
        off, _ = _assert_equals(kind, sc.raw, rows, want)
    finally:
        sc.close()
    assert np.all(np.diff(off) == 600)


@pytest.mark.parametrize("kind,name", [("ray", "A_2.5"), ("ball", "far_1e3")])
def test_more_rows_than_a_grid_of_lanes(kind, name):
    text, base, (want_off, want_words, want_vals) = case(kind, name)
    sc = Scene(text)
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37      # every lane takes a second row
        reps = -(-n // len(base))
        rows = np.tile(base, (reps, 1))[:n]
        lens = np.tile(np.diff(want_off), reps)[:n]
        off, words, vals = _fill(kind, sc.raw, rows)
    finally:
        sc.close()
    assert np.array_equal(off, olr.offsets_of(lens)) and want_off[-1] > 0
    whole, per = n // len(base), len(want_words)
    assert np.array_equal(words[:whole * per].reshape(whole, per), np.broadcast_to(want_words, (whole, per)))
    assert np.array_equal(vals[:whole * per].reshape(whole, per), np.broadcast_to(qlr.bits(want_vals), (whole, per)))
    rest = int(off[-1]) - whole * per
    assert np.array_equal(words[whole * per:off[-1]], want_words[:rest]) and np.array_equal(vals[whole * per:off[-1]], qlr.bits(want_vals)[:rest])
    assert np.all(words[off[-1]:] == SENTINEL) and np.all(vals[off[-1]:] == SENTINEL)


# ---- 5. writes are bounded by the caller's offsets and capacity, words and values both ----------------------------------------------------
BOUNDED = [("ray", "A_inf"), ("ball", "dense")]


def _want_fill(want, offsets, size, capacity):
    blank = np.full(size + PAST, SENTINEL, u32)
    return qlr.fill(want[0], want[1], offsets, blank, capacity=capacity), qlr.fill(want[0], want[2], offsets, blank, capacity=capacity)


def _assert_bounded(kind, sc, rows, want, offsets, size, capacity):
    _, words, vals = _fill(kind, sc.raw, rows, offsets=offsets, size=size, capacity=capacity)
    want_words, want_vals = _want_fill(want, offsets, size, capacity)
    assert np.array_equal(words, want_words) and np.array_equal(vals, want_vals)
    only = _fill(kind, sc.raw, rows, offsets=offsets, size=size, capacity=capacity, values=False)[1]
    assert np.array_equal(only, want_words)
    return words, vals


@pytest.mark.parametrize("kind,name", BOUNDED)
def test_offsets_from_smaller_counts_truncate_every_row_in_order(dense, kind, name):
    _, rows, want = case(kind, name)
    short = olr.offsets_of(np.minimum(np.diff(want[0]), 3))
    total = int(short[-1])
    assert total < want[0][-1]
    words, vals = _assert_bounded(kind, dense, rows, want, short, total, total)
    first3 = np.concatenate([np.arange(want[0][i], min(want[0][i] + 3, want[0][i + 1])) for i in range(len(rows))])      # every row's first three, in order
    assert np.array_equal(words[:total], want[1][first3]) and np.array_equal(vals[:total], qlr.bits(want[2])[first3])
    assert np.all(words[total:] == SENTINEL) and np.all(vals[total:] == SENTINEL)


@pytest.mark.parametrize("kind,name", BOUNDED)
def test_a_capacity_below_the_total_keeps_everything_from_it_on(dense, kind, name):
    _, rows, want = case(kind, name)
    want_off = want[0]
    total = int(want_off[-1])
    half = total // 2
    if not np.any((want_off[:-1] < half) & (want_off[1:] > half + 1)):
        half += 1
    assert np.any((want_off[:-1] < half) & (want_off[1:] > half))      # a row's segment straddles the capacity
    words, vals = _assert_bounded(kind, dense, rows, want, want_off, total, half)
    assert np.array_equal(words[:half], want[1][:half]) and np.all(words[half:] == SENTINEL) and np.all(vals[half:] == SENTINEL)
    # a row whose segment starts at the capacity, and beyond it, writes nothing; capacity 0 writes nothing
    at = int(want_off[np.searchsorted(want_off, half)])
    words, vals = _assert_bounded(kind, dense, rows, want, want_off, total, at)
    assert np.array_equal(vals[:at], qlr.bits(want[2])[:at]) and np.all(words[at:] == SENTINEL) and np.all(vals[at:] == SENTINEL)
    words, vals = _assert_bounded(kind, dense, rows, want, want_off, total, 0)
    assert np.all(words == SENTINEL) and np.all(vals == SENTINEL)


@pytest.mark.parametrize("kind,name", BOUNDED)
def test_a_segment_longer_than_the_row_keeps_its_tail_and_odd_offsets_write_nothing(dense, kind, name):
    _, rows, want = case(kind, name)
    want_off = want[0]
    longer = olr.offsets_of(np.diff(want_off) + 1)      # every segment one longer than its row's list, the empty rows' too
    words, vals = _assert_bounded(kind, dense, rows, want, longer, int(longer[-1]), int(longer[-1]))
    assert np.all(words[longer[1:] - 1] == SENTINEL) and np.count_nonzero(words == SENTINEL) == len(rows) + PAST
    assert np.all(vals[longer[1:] - 1] == SENTINEL) and np.count_nonzero(vals == SENTINEL) == len(rows) + PAST
    # offsets that run backwards, or lie below 0, are segments without room: nothing is written
    for odd in (want_off[::-1].copy(), want_off - want_off[-1] - 5):
        _, words, vals = _fill(kind, dense.raw, rows, offsets=odd, size=int(want_off[-1]))
        assert np.all(words == SENTINEL) and np.all(vals == SENTINEL) and len(words) == int(want_off[-1]) + PAST


# ---- 6. further properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", BOUNDED)
def test_two_calls_give_identical_bytes_and_another_stream_the_same(dense, kind, name):
    _, rows, _ = case(kind, name)
    a = _fill(kind, dense.raw, rows)
    b = _fill(kind, dense.raw, rows)
    c = _fill(kind, dense.raw, rows, stream=torch.cuda.Stream())
    for x in (b, c):
        assert all(np.array_equal(p, q) for p, q in zip(a, x))


def test_lists_follow_geometry_updated_in_place():
    text = tma.dense_scene_text()
    lines = text.split("\n")
    first = next(i for i, l in enumerate(lines) if l.startswith("sphere "))
    moved = "\n".join(lines[:first] + ["sphere 0.30000 0.40000 -0.20000 0.70000"] + lines[first + 1:])
    rays, balls = tma.case_input("A_2.5")[1][:1024], tca.CASES["dense"]()[1][:512]
    sc = Scene(text)
    try:
        before = {kind: _fill(kind, sc.raw, rows) for kind, rows in (("ray", rays), ("ball", balls))}
        m.update_spheres(sc.raw, torch.tensor([[0.3, 0.4, -0.2, 0.7]], dtype=torch.float32, device=DEV), first=0)
        for kind, rows in (("ray", rays), ("ball", balls)):      # updated, not yet built
            d_off = torch.from_numpy(before[kind][0]).to(DEV)
            with pytest.raises(m.MirtError) as e:
                KINDS[kind][1](sc.raw, torch.from_numpy(rows).to(DEV), d_off, _buffer(int(before[kind][0][-1])))
            assert e.value.status == 6 and m.lib().mirt_last_error().startswith(b"mirt_%s_list:" % kind.encode())
        m.build_lbvh_karas(sc.raw)
        after = Scene(moved)      # (its arrays and tree: the moved scene built afresh)
        try:
            for kind, rows in (("ray", rays), ("ball", balls)):
                off, words = _assert_equals(kind, sc.raw, rows, _library_reference(kind, after, rows))
                assert not (np.array_equal(off, before[kind][0]) and np.array_equal(words, before[kind][1][:len(words)]))
        finally:
            after.close()
    finally:
        sc.close()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ray", "ball"])
def test_argument_errors(kind):
    who = b"mirt_%s_list" % kind.encode()
    width = 8 if kind == "ray" else 4
    raw = m.initRawConfigFromStl(m.parseText(tma.TWINS), 0)
    try:
        n, cap = 8, 64
        Q = torch.zeros((4 * n, width), dtype=torch.float32, device=DEV)
        if kind == "ray":
            Q[:, 3], Q[:, 6] = float("inf"), -1.0      # (live rays through the twins)
        else:
            Q[:, 3] = 100.0                            # (live balls that hold the whole scene)
        O = torch.arange(0, 8 * (4 * n + 1), 8, dtype=torch.int64, device=DEV)
        W, V = _buffer(4 * cap), _buffer(4 * cap)
        fill = KINDS[kind][1]
        with pytest.raises(m.MirtError) as e:
            fill(raw, Q[:n], O[:n + 1], W[:cap], V[:cap].view(torch.float32))
        assert e.value.status == 6 and m.lib().mirt_last_error().startswith(who + b":")
        m.build_lbvh_karas(raw)
        f = getattr(query_lists.lib(), who.decode())
        pQ, pO, pW, pV = Q.data_ptr(), O.data_ptr(), W.data_ptr(), V.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(q=pQ, count=n, o=pO, w=pW, v=pV, capacity=cap, flags=0):
            return f(raw._h, vp(q), count, vp(o), vp(w), vp(v), capacity, flags, None)

        def refused(**kw):
            return call(**kw) == 3 and m.lib().mirt_last_error().startswith(who + b":")

        assert refused(count=-1) and refused(capacity=-1)
        for flags in (1, 2, 0x80000000):
            assert refused(flags=flags)
        assert refused(q=0) and refused(o=0) and refused(w=0) and refused(q=0, o=0, w=0, v=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(o=pO + 4) and refused(w=pW + 2) and refused(v=pV + 2)
        nq, no, nw = 4 * width * n, 8 * (n + 1), 4 * cap
        assert refused(o=pQ) and refused(o=pQ + nq - 8) and refused(q=pO)                                  # offsets over the rows
        assert refused(w=pQ) and refused(w=pQ + nq - 4) and refused(w=pQ - nw + 4)                         # words over the rows
        assert refused(w=pO) and refused(w=pO + no - 4) and refused(o=pW + nw - 8)                         # words over the offsets
        assert refused(v=pQ) and refused(v=pQ + nq - 4) and refused(v=pO) and refused(v=pO + no - 4)       # values over the rows, the offsets
        assert refused(v=pW) and refused(v=pW + nw - 4) and refused(v=pW - nw + 4)                         # values over the words
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(V == SENTINEL))      # nothing ran
        # no rows and no capacity are no work; with capacity 0 the words' and the values' pointers are no ranges
        assert call(count=0) == 0 and call(q=0, count=0, o=0, w=0, v=0, capacity=0) == 0 and call(w=0, v=0, capacity=0) == 0
        assert call(w=pQ, v=pQ, capacity=0) == 0 and call(count=0, q=0, o=0) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(W == SENTINEL)) and bool(torch.all(V == SENTINEL))
        # touching ranges are not overlaps; the values are optional
        counts = _np(KINDS[kind][0](raw, Q[:n])).astype(np.int64)
        assert counts.min() >= 2
        written = int(np.minimum(counts, 8).sum())
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
    finally:
        raw.close()

"""Ray and ball lists (include_ext/mirt_query_lists.h: mirt_ray_list, mirt_ball_list): what the header's text says, the wrappers'
checks, the fill kernels' code generation, and the numpy restatement (tests/query_lists_ref.py) against itself over the oracle's
tree: on the inputs the GPU tests use, the two left-first walks emit the reference's words and values in the reference's order, every
row's length is the record reference's count, and every row sorted begins with the record reference's eight records.  The header
against query_lists.py's signature table and the built library is a row of tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import re
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, query_lists
from cuda_ray_tracer_amd import build as B
import contacts_ref as kr
import multihit_ref as mr
import overlap_list_ref as olr
import query_lists_ref as qlr
import test_contacts_abi as tca
import test_multihit_abi as tma
from codegen_lib import _kernel_body, _resource_usage, _strip
from test_closest_abi import _oracle_tree
from test_extension_abi import EXTENSIONS, other_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "mirt_query_lists.h")
ROW = next(x for x in EXTENSIONS if x.module == "query_lists")
u32 = np.uint32
u64 = np.uint64
f32 = np.float32


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_refers_to_the_sets_and_states_the_order_the_values_and_the_bounded_writes():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert "the count-only call of mirt_multihit.h" in text and "of mirt_contacts.h" in text and "the offsets call of the overlap-list extension" in text
    assert "kind << 30 | id" in text and "bit for bit" in text
    # the sets are referred to by the defining header's file name and section, not restated -- and the sections exist
    for section, where in (("Rays that are not live", "include/mirt_multihit.h"), ("The admitted set S", "include/mirt_multihit.h"),
                           ("Candidates are not redefined here", "include_ext/mirt_contacts.h")):
        assert '"%s"' % section in text
        assert section in " ".join(open(os.path.join(ROOT, where)).read().replace(" *", " ").split()), section
    assert "sqrtf" not in text and "fabsf" not in text and "hit_aabb" not in text and "checkPlane" not in text
    assert "first the planes of the set, ascending by index" in text and "LEAF ORDER" in text and "ties in input order" in text
    assert "A rebuild after a geometry update may reorder a row" in text and "neither set depends on the order of the visits" in text
    assert "A STABLE sort of a row by the bits of t" in text and "(t, class, index)" in text
    assert "dist's bits << 32 | word" in text and "(dist, kind, id)" in text
    assert "min(|set|, d_offsets[i + 1] - d_offsets[i])" in text and "never write outside [0, capacity)" in text
    assert "keeps its tail untouched" in text and "a row that is not live writes nothing and does not read its offsets" in text
    assert "no allocation, no synchronisation, no atomics" in text and "One lane per row" in text


def test_the_header_has_one_include_and_names_no_other_extensions_entry_point_in_its_comments_either():
    """(nor the overlap-list header, whose file name is an entry point's name)"""
    assert len(re.findall(r"^#include", _strip(HEADER), flags=re.M)) == 1
    raw, others = open(HEADER).read(), other_entry_points(ROW)
    assert len(others) >= 11 and "mirt_trace_rays_multi" in others and "mirt_closest_points_multi" in others and "mirt_list_offsets" in others
    assert [k for k in others if k in raw] == []
    assert "mirt_overlap_list" not in raw and "mirt_trace_rays" not in raw and "mirt_closest_points" not in raw


def test_unpack_words_is_the_overlap_lists():
    assert m.unpack_words is api.unpack_words and not hasattr(query_lists, "unpack_words")      # (the existing one)


def test_the_bounded_write_rule_has_one_copy():
    """list_cursor.h holds the room of a row's segment; the three fill kernels take it from there and restate none of it."""
    read = lambda name: open(os.path.join(B.CSRC, name)).read()
    rule = ("lim < capacity", "0xffffffffll")
    assert all(w in read("list_cursor.h") for w in rule)
    for src in ("overlap_list.hip", "query_lists.hip"):
        text = read(src)
        assert '#include "list_cursor.h"' in text and "list_room(" in text, src
        assert not any(w in text for w in rule), src
    # the walks are written out in the new file, and say whose copies they are
    text = read("query_lists.hip")
    assert "multihit_kernel<0>" in text and "contacts_kernel<0>" in text and text.count("stack_pop(") == 2 and "atomic" not in text


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    Of, W, V = torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros(9)
    for fill, lists, width, other in ((m.ray_list, m.ray_lists, 8, 4), (m.ball_list, m.ball_lists, 4, 8)):
        Q = torch.zeros((4, width))
        with pytest.raises(ValueError, match="dtype"):
            fill(raw, Q.double(), Of, W)
        with pytest.raises(ValueError, match="dtype"):
            fill(raw, Q, Of.int(), W)
        with pytest.raises(ValueError, match="dtype"):
            fill(raw, Q, Of, W.long())
        with pytest.raises(ValueError, match="dtype"):
            fill(raw, Q, Of, W, V.double())
        with pytest.raises(ValueError, match="dtype"):
            fill(raw, Q, Of, W, W)                                   # (values are float32)
        with pytest.raises(ValueError, match="shape"):
            fill(raw, torch.zeros((4, other)), Of, W)
        with pytest.raises(ValueError, match="shape"):
            fill(raw, Q, torch.zeros(4, dtype=torch.int64), W)       # (n + 1 offsets)
        with pytest.raises(ValueError, match="shape"):
            fill(raw, Q, Of, torch.zeros((3, 3), dtype=torch.int32))
        with pytest.raises(ValueError, match="shape"):
            fill(raw, Q, Of, W, torch.zeros(8))                      # (a value per word)
        with pytest.raises(ValueError, match="contiguous"):
            fill(raw, Q, Of, torch.zeros(18, dtype=torch.int32)[::2])
        with pytest.raises(ValueError, match="contiguous"):
            fill(raw, Q, Of, W, torch.zeros(18)[::2])
        with pytest.raises(ValueError, match="cuda"):
            fill(raw, Q, Of, W)
        with pytest.raises(ValueError, match="cuda"):
            fill(raw, Q, Of, W, V)
        with pytest.raises(ValueError, match="dtype"):
            lists(raw, Q.double())
        with pytest.raises(ValueError, match="shape"):
            lists(raw, torch.zeros(32))
        with pytest.raises(ValueError, match="cuda"):
            lists(raw, Q, sort=True)


# ---- code generation ----------------------------------------------------------------------------------------------------------------
# kernel, with values: (VGPRs, waves per SIMD) the compiler reported
PINNED = {("ray_list_kernel", False): (64, 8), ("ray_list_kernel", True): (64, 8), ("ball_list_kernel", False): (56, 8), ("ball_list_kernel", True): (56, 8)}


def test_fill_kernels_codegen_has_no_spill_and_one_scratch_store_each():
    """query_lists.hip compiled for gfx950, from the compiler's report: four kernels -- the ray and the ball fill, each without and
    with the value array --, none with a register spill or an AGPR, each with the 20-entry LDS stack per lane of a 256-thread block,
    the private segment of trace_rays_kernel (the stack's spill array and nothing else) and exactly one scratch store, the push of
    a stack entry beyond the LDS part.  Registers and waves per SIMD as pinned above.  No atomic anywhere, and the instance without
    values has one global store (the word), the one with values two."""
    res, asm = _resource_usage("query_lists.hip")
    by = {(re.search(r"\d+(ray|ball)_list_kernel", k).group(0).lstrip("0123456789"), "ILb1E" in k): k for k in res}
    assert sorted(by) == sorted(PINNED) and len(res) == 4, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    for key, name in by.items():
        r = res[name]
        print(key, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (key, r)
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, (key, r)
        assert {r["ScratchSize [bytes/lane]"]} == private, (key, r)
        assert r["VGPRs"] <= PINNED[key][0] and r["Occupancy [waves/SIMD]"] >= PINNED[key][1], (key, r)
        body = _kernel_body(asm, name)
        assert len([t for t in body if t.startswith("scratch_store")]) == 1, key
        assert not [t for t in body if "atomic" in t], key
        stores = [t for t in body if t.startswith(("global_store", "flat_store"))]
        # (the plane loop and the walk each hold a copy of the emission)
        assert stores and all(t.startswith("global_store_dword ") for t in stores) and len(stores) % (2 if key[1] else 1) == 0, (key, stores)


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ray_reference(name):
    """(offsets int64 [n + 1], words uint32, t float32) of a multihit case: what the GPU tests compare against."""
    arrays, nodes, refs, rays, S = tma._cpu_case(name)
    return qlr.ray_lists(refs, S)


@functools.lru_cache(maxsize=None)
def ball_tree(name):
    text, _ = tca.CASES[name]()
    return _oracle_tree(text)


@functools.lru_cache(maxsize=None)
def ball_reference(name):
    """(offsets int64 [n + 1], words uint32, dist float32) of a contacts case: what the GPU tests compare against."""
    text, rows = tca.CASES[name]()
    arrays, nodes, refs = ball_tree(name)
    return qlr.ball_lists(arrays, rows, refs)


def _check_shapes(offsets, words, values, n):
    assert offsets.dtype == np.int64 and offsets.shape == (n + 1,) and offsets[0] == 0
    assert words.dtype == u32 and values.dtype == f32 and len(words) == len(values) == offsets[n]


def _planes_first(offsets, words):
    kind, pid = olr.unpack(words)
    for i in np.flatnonzero(np.diff(offsets) > 0)[:200]:
        k, p = kind[offsets[i]:offsets[i + 1]], pid[offsets[i]:offsets[i + 1]]
        npl = int(np.sum(k == 3))
        assert np.all(k[:npl] == 3) and np.all(np.diff(p[:npl]) > 0) and np.all(k[npl:] != 3)


@pytest.mark.parametrize("name", list(tma.CASES))
def test_the_ray_walk_emits_the_reference_and_sorted_rows_begin_with_the_records(name):
    arrays, nodes, refs, rays, S = tma._cpu_case(name)
    offsets, words, t = ray_reference(name)
    n = len(rays)
    _check_shapes(offsets, words, t, n)
    hits, counts = mr.records(arrays, refs, S, 8)
    assert np.array_equal(np.diff(offsets), counts.astype(np.int64))                # every row's length is the record reference's count
    walked = qlr.ray_walk(arrays, rays, nodes, refs)
    assert len(walked) == n and [len(w) for w, _ in walked] == np.diff(offsets).tolist()
    assert np.array_equal(np.concatenate([w for w, _ in walked]), words)            # the reference's words in the reference's order
    assert np.array_equal(qlr.bits(np.concatenate([v for _, v in walked])), qlr.bits(t))
    assert np.all(t > 0)                                                            # (so the bits order as unsigned integers)
    _planes_first(offsets, words)
    for i, row in enumerate(qlr.ray_sorted_rows(offsets, words, t)):
        k = min(8, len(row))
        assert np.array_equal(row[:k], hits[i, :k, :3].astype(np.int64)), i
        assert np.all(hits[i, k:, 1] == 0)
    if name == "A_inf":
        assert np.mean(np.diff(offsets) > 8) > 0.10                                 # the lists the record call truncates
        # the sets do not depend on the visiting order; the order of a row does
        other = qlr.ray_walk(arrays, rays[:500], nodes, refs, left_first=False)
        assert all(np.array_equal(np.sort(a[0]), np.sort(b[0])) for a, b in zip(walked, other))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(walked, other))
    if name == "C":
        assert np.all(np.diff(offsets) == 600)


@pytest.mark.parametrize("name", list(tca.CASES))
def test_the_ball_walk_emits_the_reference_and_sorted_rows_begin_with_the_records(name):
    text, rows = tca.CASES[name]()
    arrays, nodes, refs = ball_tree(name)
    offsets, words, dist = ball_reference(name)
    n = len(rows)
    _check_shapes(offsets, words, dist, n)
    hits, counts, _ = tca.reference(name, 8)
    assert np.array_equal(np.diff(offsets), counts.astype(np.int64))
    walked = qlr.ball_walk(arrays, rows, nodes, refs)
    assert len(walked) == n and [len(w) for w, _ in walked] == np.diff(offsets).tolist()
    assert np.array_equal(np.concatenate([w for w, _ in walked]), words)
    assert np.array_equal(qlr.bits(np.concatenate([v for _, v in walked])), qlr.bits(dist))
    assert np.all(dist >= 0)
    _planes_first(offsets, words)
    for i, row in enumerate(qlr.ball_sorted_rows(offsets, words, dist)):
        k = min(8, len(row))
        assert np.array_equal(row[:k], hits[i, :k, :3].astype(np.int64)), i
        assert np.all(hits[i, k:, 1] == 0)
    lens = np.diff(offsets)
    if name == "dense":
        print(f"dense: more than 8: {np.mean(lens > 8):.3f}, none: {np.mean(lens == 0):.3f}, mean {lens.mean():.1f}, max {lens.max()}")
        assert np.mean(lens > 8) >= 0.15 and np.mean(lens == 0) >= 0.30
        other = qlr.ball_walk(arrays, rows[:300], nodes, refs, left_first=False)
        assert all(np.array_equal(np.sort(a[0]), np.sort(b[0])) for a, b in zip(walked, other))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(walked, other))
    if name == "deep_stack":
        assert np.all(lens == 600)


def test_the_duplicated_sphere_is_listed_twice_in_leaf_order():
    arrays, nodes, refs = tma.oracle_tree(tma.TWINS)
    rays = tma.twin_rays()
    offsets, words, t = qlr.ray_lists(refs, mr.admitted(arrays, rays, nodes, refs))
    assert np.diff(offsets).tolist() == [2, 2, 0]
    order = [int(i) for ty, i in zip(refs["type"], refs["id"]) if i in (1, 3)]
    for r in (0, 1):
        kind, pid = olr.unpack(words[offsets[r]:offsets[r + 1]])
        assert kind.tolist() == [1, 1] and pid.tolist() == order and t[offsets[r]] == t[offsets[r] + 1]
    assert t[0] == 3.0


def test_fill_honours_truncating_offsets_and_a_capacity_for_words_and_values():
    offsets, words, dist = ball_reference("dense")
    total = int(offsets[-1])
    for want in (words, dist):
        sentinel = np.full(total + 4, 0xdeadbeef, u32)
        whole = qlr.fill(offsets, want, offsets, sentinel)
        assert np.array_equal(whole[:total], qlr.bits(want) if want.dtype == f32 else want) and np.all(whole[total:] == 0xdeadbeef)
        short = olr.offsets_of(np.minimum(np.diff(offsets), 3))
        got = qlr.fill(offsets, want, short, sentinel)
        i = int(np.argmax(np.diff(offsets)))
        assert got[short[i]:short[i + 1]].tolist() == np.ascontiguousarray(want[offsets[i]:offsets[i] + 3]).view(u32).tolist() and np.all(got[short[-1]:] == 0xdeadbeef)
        half = qlr.fill(offsets, want, offsets, sentinel, capacity=total // 2)
        assert np.array_equal(half[:total // 2], whole[:total // 2]) and np.all(half[total // 2:] == 0xdeadbeef)
        assert np.all(qlr.fill(offsets, want, offsets[::-1].copy(), sentinel) == 0xdeadbeef)
        assert np.all(qlr.fill(offsets, want, offsets - total - 5, sentinel) == 0xdeadbeef)

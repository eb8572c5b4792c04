"""Overlap lists (include_ext/mirt_overlap_list.h: mirt_list_offsets_work_bytes, mirt_list_offsets, mirt_overlap_list): what the
header's text says, the wrappers' checks, the fill kernel's code generation, and the numpy restatement (tests/overlap_list_ref.py)
against itself over the oracle's tree: on the inputs the GPU tests use, the left-first pruned walk emits the reference's words in the
reference's order, every row's words are the brute force's admitted set, and the segment lengths are its counts.  The header
against overlap_list.py's signature table and the built library is a row of tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import build as B
import overlap_list_ref as olr
import overlap_ref as ovr
from codegen_lib import _kernel_body, _resource_usage
from test_closest_abi import _oracle_tree
from test_extension_abi import EXTENSIONS, _module, other_entry_points
from test_overlap_abi import CASES, CHOSEN_ROWS, case_keys, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "mirt_overlap_list.h")
ROW = next(x for x in EXTENSIONS if x.module == "overlap_list")
u32 = np.uint32
u64 = np.uint64


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_order_and_the_bounded_writes():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert "the count-only call of mirt_overlap.h" in text and "kind << 30 | id" in text
    assert "first the planes of A_i, ascending by index" in text and "LEAF ORDER" in text and "ties in input order" in text
    assert "The SET is defined by the scene's arrays alone; the ORDER within a row is the builder's" in text
    assert "sorts each segment's words" in text and "A rebuild after a geometry update may reorder a row" in text
    assert "min(|A_i|, d_offsets[i + 1] - d_offsets[i])" in text and "never write outside [0, capacity)" in text
    assert "keeps its tail untouched" in text and "a row that is not live writes nothing" in text
    assert "a total past 2^32 is exact" in text and "no order of arrival is observable" in text
    for section in ('"Row rule"', '"Candidates"', '"Admission"', '"Arithmetic"'):      # (referred to, not restated)
        assert section in text
    assert "dmin2" not in text and "fabsf" not in text


def test_the_header_names_no_other_extensions_entry_point_in_its_comments_either():
    raw, others = open(HEADER).read(), other_entry_points(ROW)
    assert len(others) >= 10 and "mirt_overlap_boxes" in others
    assert [k for k in others if k in raw] == []
    assert "mirt_overlap_boxes" not in raw and not any("mirt_overlap_boxes" in s.name for s in ROW.symbols)


def test_the_shared_device_code_has_one_copy():
    """The scan, the overlap tests and the walks' slack are in headers: overlap.hip, overlap_list.hip and lbvh_build.hip include them
    and define none of them.  The fill kernel takes the tests through overlap_walk.h, which holds its walk (the leaf tests and the
    register fences; overlap.hip keeps its own), and the slack is point_query.h's, the only one in csrc."""
    read = lambda name: open(os.path.join(B.CSRC, name)).read()
    tests = ("bool sphere_overlaps(", "bool triangle_overlaps(", "bool edge_axis(")
    walk = ("triangle_overlaps(m, h", "sphere_overlaps(lo, hi", "asm volatile", "stack_pop(")
    for src, header, words in (("overlap.hip", "overlap_tests.h", tests + ("float SLACK",)),
                               ("overlap.hip", "point_query.h", ()),
                               ("overlap_list.hip", "overlap_walk.h", tests + walk + ("float SLACK",)),
                               ("overlap_walk.h", "overlap_tests.h", tests + ("float SLACK",)),
                               ("overlap_list.hip", "block_scan.h", (" block_exclusive_scan(T v",)),
                               ("lbvh_build.hip", "block_scan.h", (" block_exclusive_scan(T v", "uint32_t block_exclusive_scan("))):
        text = read(src)
        assert '#include "%s"' % header in text, (src, header)
        for w in words:
            assert w not in text, (src, w)
    assert all(w in read("overlap_tests.h") for w in tests)
    assert all(w in read("overlap_walk.h") for w in walk)
    assert [f for f in sorted(os.listdir(B.CSRC)) if "float SLACK" in read(f)] == ["point_query.h"]
    assert " block_exclusive_scan(T v" in read("block_scan.h")


def test_the_work_bytes_are_host_arithmetic():
    L = _module(ROW).lib()
    want = {-5: 0, 0: 0, 1: 0, 2048: 0, 2049: 16, 4096: 16, 4097: 24, 65537: 8 * 33, 1 << 33: 8 * (1 << 22)}
    assert {n: L.mirt_list_offsets_work_bytes(n) for n in want} == want
    assert {n: m.list_offsets_work_bytes(n) for n in want} == want


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    Bx, Of, W, Cn = torch.zeros((4, 8)), torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        m.list_offsets(raw, Cn.float())
    with pytest.raises(ValueError, match="dtype"):
        m.list_offsets(raw, Cn.long())
    with pytest.raises(ValueError, match="dtype"):
        m.list_offsets(raw, Cn, Of.int())
    with pytest.raises(ValueError, match="shape"):
        m.list_offsets(raw, torch.zeros((4, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.list_offsets(raw, Cn, torch.zeros(4, dtype=torch.int64))      # (n + 1 offsets)
    with pytest.raises(ValueError, match="contiguous"):
        m.list_offsets(raw, torch.zeros(8, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.list_offsets(raw, Cn)
    with pytest.raises(ValueError, match="cuda"):
        m.list_offsets(raw, Cn, Of)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_list(raw, Bx.double(), Of, W)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_list(raw, Bx, Of.int(), W)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_list(raw, Bx, Of, W.long())
    with pytest.raises(ValueError, match="shape"):
        m.overlap_list(raw, torch.zeros((4, 4)), Of, W)
    with pytest.raises(ValueError, match="shape"):
        m.overlap_list(raw, Bx, torch.zeros(4, dtype=torch.int64), W)
    with pytest.raises(ValueError, match="shape"):
        m.overlap_list(raw, Bx, Of, torch.zeros((3, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        m.overlap_list(raw, Bx, Of, torch.zeros(18, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.overlap_list(raw, Bx, Of, W)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_lists(raw, Bx.double())
    with pytest.raises(ValueError, match="shape"):
        m.overlap_lists(raw, torch.zeros(32))
    with pytest.raises(ValueError, match="cuda"):
        m.overlap_lists(raw, Bx, sort=True)
    with pytest.raises(ValueError, match="shape"):
        m.voxel_lists(raw, (0, 0, 0), (1, 1, 1), (4, 4))
    # unpack_words reads kind and id back, the plane's kind (bit 31 set: a negative int32) too
    words = np.array([(1 << 30) | 5, (2 << 30) | 0x3fffffff, (3 << 30) | 7, 3 << 30], u32)
    kind, pid = m.unpack_words(torch.from_numpy(words.view(np.int32)))
    assert kind.tolist() == [1, 2, 3, 3] and pid.tolist() == [5, 0x3fffffff, 7, 0] and kind.dtype == torch.int32
    assert [x.tolist() for x in olr.unpack(words)] == [kind.tolist(), pid.tolist()]
    with pytest.raises(ValueError, match="dtype"):
        m.unpack_words(torch.zeros(3))


# ---- code generation ----------------------------------------------------------------------------------------------------------------
PINNED = (80, 6)      # (VGPRs, waves per SIMD) the compiler reported: the count-only instance's of overlap.hip


def test_fill_kernel_codegen_has_no_vgpr_spill_and_one_scratch_store():
    """overlap_list.hip compiled for gfx950, from the compiler's report: one fill kernel, without a VGPR spill or an AGPR, with the
    20-entry LDS stack per lane of a 256-thread block, the private segment of trace_rays_kernel (the stack's spill array and nothing
    else) and exactly one scratch store, the push of a stack entry beyond the LDS part.  Registers and waves per SIMD as pinned
    above; the three scan kernels beside it spill nothing and use no scratch."""
    res, asm = _resource_usage("overlap_list.hip")
    fill = [k for k in res if "overlap_list_kernel" in k]
    scans = [k for k in res if "offsets_kernel" in k or "offset_sums_kernel" in k]
    assert len(fill) == 1 and len(scans) == 3 and len(res) == 4, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    r = res[fill[0]]
    print(r)
    assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, r
    assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
    assert {r["ScratchSize [bytes/lane]"]} == private, r
    assert r["VGPRs"] <= PINNED[0] and r["Occupancy [waves/SIMD]"] >= PINNED[1], r
    assert len([t for t in _kernel_body(asm, fill[0]) if t.startswith("scratch_store")]) == 1
    for k in scans:
        print(k, res[k])
        assert res[k]["VGPRs Spill"] == 0 and res[k]["ScratchSize [bytes/lane]"] == 0 and res[k]["LDS Size [bytes/block]"] == 256 * 8, (k, res[k])


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree_of(name):
    text, _ = CASES[name]()
    _, nodes, refs = _oracle_tree(text)
    return nodes, refs


@functools.lru_cache(maxsize=None)
def list_reference(name):
    """(offsets int64 [n + 1], words uint32) of a case: what the GPU tests compare against."""
    arrays, rows, key = case_keys(name)
    return olr.lists(arrays, rows, tree_of(name)[1], key=key)


@pytest.mark.parametrize("name", list(CASES))
def test_left_first_walk_emits_the_reference_and_every_row_is_the_admitted_set(name):
    arrays, rows, key = case_keys(name)
    nodes, refs = tree_of(name)
    offsets, words = list_reference(name)
    n = len(rows)
    assert offsets.dtype == np.int64 and offsets.shape == (n + 1,) and offsets[0] == 0 and words.dtype == u32 and len(words) == offsets[n]
    # segment lengths are the brute force's counts
    _, counts, _ = reference(name, 0)
    assert np.array_equal(np.diff(offsets), counts.astype(np.int64))
    # the left-first pruned walk emits exactly these words in exactly this order
    walked = olr.walk_words(arrays, rows, nodes, refs, key=key)
    assert len(walked) == n
    assert np.array_equal(np.concatenate(walked) if n else np.zeros(0, u32), words)
    assert [len(w) for w in walked] == np.diff(offsets).tolist()
    # each row's words, sorted, are the brute force's admitted set: the low words of its keys
    admitted = key != u64(ovr.KEY_NONE)
    low = (key & u64(0xffffffff)).astype(u32)
    for i in range(n):
        assert np.array_equal(np.sort(words[offsets[i]:offsets[i + 1]]), np.sort(low[i][admitted[i]])), i
    # planes first, ascending; then no plane
    kind, pid = olr.unpack(words)
    for i in np.flatnonzero(np.diff(offsets) > 0)[:200]:
        k, p = kind[offsets[i]:offsets[i + 1]], pid[offsets[i]:offsets[i + 1]]
        npl = int(np.sum(k == 3))
        assert np.all(k[:npl] == 3) and np.all(np.diff(p[:npl]) > 0) and np.all(k[npl:] != 3)
    # the right-first walk emits the same sets in another order wherever two leaves of a row lie in both subtrees of a node
    if name == "dense":
        other = olr.walk_words(arrays, rows, nodes, refs, key=key, left_first=False)
        assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(walked, other))
        assert any(not np.array_equal(a, b) for a, b in zip(walked, other))


def test_the_chosen_row_that_holds_everything_lists_all_seven_with_the_plane_first():
    offsets, words = list_reference("chosen")
    assert np.diff(offsets)[:len(CHOSEN_ROWS)].tolist() == [r[2] for r in CHOSEN_ROWS] and np.all(np.diff(offsets)[len(CHOSEN_ROWS):] == 0)
    mine = words[offsets[17]:offsets[18]]
    kind, pid = olr.unpack(mine)
    assert len(mine) == 7 and (kind[0], pid[0]) == (3, 0)
    assert sorted(zip(kind.tolist(), pid.tolist())) == [(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]
    # the twins (triangles 0 and 1: one centroid, one Morton code) stay in input order: the sort is stable
    order = list(zip(kind.tolist(), pid.tolist()))
    assert order.index((2, 0)) + 1 == order.index((2, 1))
    # the row of the plane alone, and the empty row
    assert words[offsets[4]:offsets[5]].tolist() == [3 << 30] and offsets[18] == offsets[19]


def test_fill_honours_truncating_offsets_and_a_capacity():
    offsets, words = list_reference("chosen")
    total = int(offsets[-1])
    sentinel = np.full(total + 4, 0xdeadbeef, u32)
    assert np.array_equal(olr.fill(offsets, words, offsets, sentinel)[:total], words) and np.all(olr.fill(offsets, words, offsets, sentinel)[total:] == 0xdeadbeef)
    short = olr.offsets_of(np.minimum(np.diff(offsets), 3))
    got = olr.fill(offsets, words, short, sentinel)
    assert got[short[17]:short[18]].tolist() == words[offsets[17]:offsets[17] + 3].tolist() and np.all(got[short[-1]:] == 0xdeadbeef)
    half = olr.fill(offsets, words, offsets, sentinel, capacity=total // 2)
    assert np.array_equal(half[:total // 2], words[:total // 2]) and np.all(half[total // 2:] == 0xdeadbeef)
    assert olr.offsets_of(np.full(65537, 70000, u32))[-1] == 4587590000 > 1 << 32


def test_the_dense_case_has_lists_longer_than_eight():
    offsets, _ = list_reference("dense")
    assert np.mean(np.diff(offsets) > 8) > 0.10 and np.diff(offsets).max() > 50

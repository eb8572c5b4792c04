"""Contact queries (include_ext/mirt_contacts.h: mirt_closest_points_multi): what the header's text says, the wrappers' checks, the
kernel's code generation, and the numpy restatement of the header (tests/contacts_ref.py) against itself over the oracle's tree:
on the inputs the GPU tests use, the pruned walk with either bound rule gives the brute force's bits on every row, and the
records, counts and order have the properties the header states.  The header against contacts.py's signature table and the built
library is a row of tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import re
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import closest_ref as cr
import contacts_ref as kr
import edge_scenes
import pyscene
from codegen_lib import _kernel_body, _resource_usage
from test_closest_abi import _oracle_tree, _points_about, with_tight_radii
from test_multihit_abi import dense_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "mirt_contacts.h")
f32 = np.float32
u32 = np.uint32


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_adopts_the_candidates_of_mirt_closest_h_and_states_the_rules():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert "Candidates are not redefined here" in text and "never by the tree" in text and "(dist, kind, id)" in text
    assert "bit for bit, on every row without exception" in text
    assert "B is R for the whole walk" in text and "until the list holds k entries" in text and "sigma = 2^-18" in text
    assert "R = +inf visits every leaf" in text


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    P, Hh, Cn, F = torch.zeros((4, 4)), torch.zeros((4, 3, 6), dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros((4, 3, 8))
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points_multi(raw, P.double(), Hh)
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points_multi(raw, P, Hh.to(torch.int16))
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points_multi(raw, P, Hh, Cn.float())
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points_multi(raw, P, Hh, Cn, F.double())
    with pytest.raises(ValueError, match="dtype"):
        m.count_within(raw, P.double())
    with pytest.raises(ValueError, match="dtype"):
        m.count_within(raw, P, Cn.float())
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, torch.zeros((4, 3)), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, torch.zeros((4, 18), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, torch.zeros((5, 3, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, torch.zeros((4, 3, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape.*at most 8"):
        m.closest_points_multi(raw, P, torch.zeros((4, 9, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, Hh, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, Hh, Cn, torch.zeros((4, 2, 8)))      # (the features' k is the records')
    with pytest.raises(ValueError, match="shape"):
        m.closest_points_multi(raw, P, Hh, Cn, torch.zeros((4, 3, 6)))
    with pytest.raises(ValueError, match="shape"):
        m.count_within(raw, torch.zeros(16))
    with pytest.raises(ValueError, match="shape"):
        m.count_within(raw, P, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="d_counts"):
        m.closest_points_multi(raw, P, None)
    with pytest.raises(ValueError, match="d_counts"):
        m.closest_points_multi(raw, P, torch.zeros((4, 0, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points_multi(raw, torch.zeros((4, 8))[:, ::2], Hh)
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points_multi(raw, P, torch.zeros((4, 3, 12), dtype=torch.int32)[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points_multi(raw, P, Hh, torch.zeros(8, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points_multi(raw, P, Hh, Cn, torch.zeros((4, 3, 16))[:, :, ::2])
    with pytest.raises(ValueError, match="cuda"):
        m.closest_points_multi(raw, P, Hh, Cn, F)
    with pytest.raises(ValueError, match="cuda"):
        m.count_within(raw, P)
    # pack_points makes the rows, unpack_hits reads the records of every row, flattened
    assert m.pack_points(torch.zeros((4, 3)), 0.5).shape == P.shape
    t, kind, pid, nn = m.unpack_hits(Hh.reshape(-1, 6))
    assert t.shape == (12,) and nn.shape == (12, 3)


# ---- code generation ----------------------------------------------------------------------------------------------------------------
PINNED = {0: (54, 8), 1: (66, 7), 4: (74, 6), 8: (84, 5)}      # capacity: (VGPRs, waves per SIMD) the compiler reported


def test_contacts_kernel_codegen_keeps_the_list_in_registers():
    """closest_multi.hip compiled for gfx950, from the compiler's report: four instances (capacity 0, 1, 4, 8), none with a register
    spill or an AGPR, each with the 20-entry LDS stack per lane of a 256-thread block, the private segment of trace_rays_kernel
    (the stack's spill array and nothing else: a list indexed at run time would add to it) and exactly one scratch store, the push
    of a stack entry beyond the LDS part.  Registers and waves per SIMD as pinned above: 8 waves for the count-only instance, 7
    for capacity 1, 6 for capacity 4, 5 for capacity 8 (84 VGPRs: at 6 waves it spills two registers)."""
    res, asm = _resource_usage("closest_multi.hip")
    by_cap = {int(re.search(r"contacts_kernelILi(\d+)E", k).group(1)): k for k in res}
    assert sorted(by_cap) == [0, 1, 4, 8] and len(res) == 4, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    for cap, name in by_cap.items():
        r = res[name]
        print(cap, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (cap, r)
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, (cap, r)
        assert {r["ScratchSize [bytes/lane]"]} == private, (cap, r)
        assert r["VGPRs"] <= PINNED[cap][0] and r["Occupancy [waves/SIMD]"] >= PINNED[cap][1], (cap, r)
        body = _kernel_body(asm, name)
        assert len([t for t in body if t.startswith("scratch_store")]) == 1, cap


# ---- the inputs (the GPU tests use the same) -----------------------------------------------------------------------------------------
def _arrays(text):
    return pyscene.parse_lines(text.split("\n")).arrays()


def shuffled(rows, seed=1):
    """(so that rows with and without a radius, tight and loose, sit in the same wave)"""
    return np.ascontiguousarray(rows[np.random.default_rng(seed).permutation(len(rows))])


@functools.lru_cache(maxsize=None)
def dense_case():
    """(text, rows): the dense scene (300 spheres, 200 triangles, 2 planes) and 2000 shuffled rows -- 300 points with R = inf, with
    R the nearest distance (a miss) and one step above it (that one surface), and 1100 points with R log-uniform in 0.05..1.5."""
    text = dense_scene_text()
    arrays = _arrays(text)
    tight, nhas = with_tight_radii(arrays, _points_about(arrays, 300, 51, 0.5))
    assert nhas == 300
    rng = np.random.default_rng(52)
    loose = np.concatenate([_points_about(arrays, 1100, 53, 0.5), np.exp(rng.uniform(np.log(0.05), np.log(1.5), (1100, 1))).astype(f32)], axis=1)
    rows = shuffled(np.concatenate([tight, loose]).astype(f32))
    assert rows.shape == (2000, 4)
    return text, rows


@functools.lru_cache(maxsize=None)
def far_case(offset):
    """(text, rows): far_from_origin and the rows of the closest-point query's far-from-origin test, with tight radii."""
    text = edge_scenes.far_from_origin(offset=offset)
    arrays = _arrays(text)
    q = _points_about(arrays, 500, 31, 0.5)
    S = arrays["spheres"]
    rng = np.random.default_rng(32)
    off = np.zeros((len(S), 3))
    off[np.arange(len(S)), rng.integers(0, 3, len(S))] = (S["r"] + rng.uniform(0.001, 0.05, len(S))) * rng.choice([-1, 1], len(S))
    q = np.concatenate([q, (S["c"].astype(np.float64) + off).astype(f32)])
    rows, _ = with_tight_radii(arrays, q)
    return text, shuffled(rows)


@functools.lru_cache(maxsize=None)
def deep_case():
    """(text, rows): deep_stack(600) and 250 rows with R = inf, inside the nest and outside."""
    text = edge_scenes.deep_stack(600)
    arrays = _arrays(text)
    q = _points_about(arrays, 250, 44, 1.5)
    return text, np.concatenate([q, np.full((250, 1), np.inf, f32)], axis=1)


CASES = {"dense": dense_case, "far_1e3": lambda: far_case(1000.0), "far_1e5": lambda: far_case(100000.0), "deep_stack": deep_case}


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """(hits, counts, features) of a case by the brute force: what the GPU tests compare against."""
    text, rows = CASES[name]()
    return kr.brute_force(_arrays(text), rows, k)


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pruned_walk_with_either_bound_rule_equals_the_brute_force_bit_for_bit(name):
    text, rows = CASES[name]()
    arrays, nodes, refs = _oracle_tree(text)
    k = 8 if name in ("dense", "deep_stack") else 4
    want_hits, want_counts, want_feat = reference(name, k)
    for near_first in (True, False):
        for with_counts in (True, False):
            hits, counts, feat, visited = kr.pruned_walk(arrays, rows, nodes, refs, k, with_counts, near_first=near_first)
            assert np.array_equal(hits, want_hits) and np.array_equal(feat.view(u32), want_feat.view(u32)), (near_first, with_counts)
            if with_counts:
                assert np.array_equal(counts, want_counts), near_first
            print(f"{name}: near first {near_first}, counts {with_counts}: {visited.mean():.1f} of {len(refs)} leaves visited per row")
    if name == "deep_stack":
        assert np.all(want_counts == 600)


@pytest.mark.parametrize("name", ["far_1e3", "far_1e5"])
def test_without_the_slack_the_shrinking_bound_loses_answers(name):
    """The negative control: sigma = 0 away from the origin, where a sphere's float32 box does not bound its float32 distance."""
    text, rows = CASES[name]()
    arrays, nodes, refs = _oracle_tree(text)
    want_hits, _, _ = reference(name, 4)
    hits, _, _, _ = kr.pruned_walk(arrays, rows, nodes, refs, 4, False, slack=0.0)
    differ = np.any(hits.reshape(len(rows), -1) != want_hits.reshape(len(rows), -1), axis=1)
    print(f"{name}: {int(differ.sum())} of {len(rows)} rows differ without the slack")
    assert differ.sum() >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_records_counts_and_order(name):
    text, rows = CASES[name]()
    arrays = _arrays(text)
    h8, c8, f8 = reference(name, 8)
    h4, c4, f4 = reference(name, 4)
    h1, c1, f1 = reference(name, 1)
    h0, c0, f0 = reference(name, 0)
    n = len(rows)
    assert h8.shape == (n, 8, 6) and f8.shape == (n, 8, 8) and h0.shape == (n, 0, 6)
    assert np.array_equal(h4, h8[:, :4]) and np.array_equal(f4.view(u32), f8[:, :4].view(u32))      # the k = 4 records are the first four of k = 8
    assert np.array_equal(c4, c8) and np.array_equal(c1, c8) and np.array_equal(c0, c8)            # the counts do not depend on k
    past = np.arange(8)[None, :] >= c8[:, None]
    assert np.all(h8[past] == kr.MISS) and np.all(f8[past] == 0) and np.all(h8[~past][:, 1] != 0) and np.all(f8[~past][:, 3] == 1)
    t = h8[:, :, 0].view(f32)
    both = ~past[:, 1:]
    assert np.all((t[:, 1:] >= t[:, :-1])[both]) and np.all(t[~past] >= 0)                           # t is non-decreasing along a row
    tie = (t[:, 1:] == t[:, :-1]) & both
    order = h8[:, :, 1].astype(np.int64) * (1 << 32) + h8[:, :, 2]
    assert np.all((order[:, 1:] > order[:, :-1])[tie])                                             # ties are in (kind, id) order
    # k = 1 is mirt_closest_points' answer
    want_hits, want_feat = cr.brute_force(arrays, rows)
    assert np.array_equal(h1[:, 0], want_hits) and np.array_equal(f1[:, 0].view(u32), want_feat.view(u32))
    # the sorted list agrees with the records
    lists = kr.sorted_admitted(arrays, rows[:50])
    for i, lst in enumerate(lists):
        assert len(lst) == c8[i]
        assert [(d.view(u32), kd, j) for d, kd, j in lst[:8]] == [(int(r[0]), int(r[1]), int(r[2])) for r in h8[i, :min(8, len(lst))]]


def test_the_dense_rows_fill_truncate_and_empty_the_list():
    _, c, _ = reference("dense", 0)
    print(f"dense: more than 8: {np.mean(c > 8):.3f}, 1 to 8: {np.mean((c >= 1) & (c <= 8)):.3f}, none: {np.mean(c == 0):.3f}, max {c.max()}")
    assert np.mean(c > 8) > 0.10 and np.mean((c >= 1) & (c <= 8)) > 0.30 and np.mean(c == 0) > 0.01
    h8, _, _ = reference("dense", 8)
    assert set(h8[:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}

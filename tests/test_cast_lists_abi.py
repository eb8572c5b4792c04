"""Cast lists (include_ext3/mirt_cast_lists.h: mirt_cast_counts, mirt_cast_list): the header against cast_lists.py's signature table
and the built library, what the header's text says, the wrappers' checks, the kernels' code generation, and the numpy restatement
(tests/cast_lists_ref.py) against itself over the oracle's tree on the inputs the GPU tests use: the left-first walk with the bound
held at tmax emits the reference's words and t bits in the reference's order, clause (0) of the header removes nothing from
spherecast_ref's admitted set on these inputs, every sorted row begins with the first-contact reference's (t, kind, id), and without
the slacks the walk loses words.  No GPU needed.

The header lies in include_ext3/, whose listing is not pinned here: the next extension may join it."""
import ctypes as C
import functools
import importlib
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, binding
from cuda_ray_tracer_amd import build as B
import cast_lists_ref as clr
import overlap_list_ref as olr
import spherecast_ref as sr
import test_spherecast_abi as tsa
from codegen_lib import _kernel_body, _resource_usage, _strip
from test_binding_header import compare_prototypes, constants, prototypes
from test_closest_abi import _oracle_tree
from test_extension_abi import EXTENSIONS, _header_path, _table, mentions
from test_multihit_abi import dense_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext3", "mirt_cast_lists.h")
MOD = importlib.import_module("cuda_ray_tracer_amd.cast_lists")
PTR, I32, I64, U32 = "pointer", (4, True, False), (8, True, False), (4, False, False)
SYMBOLS = [("mirt_cast_counts", I32, [PTR, PTR, I64, PTR, U32, PTR]), ("mirt_cast_list", I32, [PTR, PTR, I64, PTR, PTR, PTR, I64, U32, PTR])]
NAMES = ("count_casts", "cast_list", "cast_lists")
f32 = np.float32
u32 = np.uint32


# ---- header, table, library ------------------------------------------------------------------------------------------------------------
def test_the_header_agrees_with_the_signature_table():
    header, table = _strip(HEADER), MOD.CAST_LISTS_SIGNATURES
    assert prototypes(header) == SYMBOLS
    assert [name for name, _, _ in prototypes(header)] == list(table)
    assert sorted(set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", header))) == sorted(table)
    assert compare_prototypes(header, table) == []
    assert constants(header) == {}
    assert re.findall(r'^#include "[./a-z]*mirt\.h"$', header, flags=re.M) == ['#include "../include/mirt.h"']
    assert len(re.findall(r"^#include", header, flags=re.M)) == 1
    restype, argtypes = table["mirt_cast_list"]
    doctored = {**table, "mirt_cast_list": (restype, [C.c_int if t is C.c_int64 else t for t in argtypes])}
    assert compare_prototypes(header, doctored) == [f"mirt_cast_list: parameter {p} is (8, True, False), the table says (4, True, False)" for p in (2, 6)]
    for name, (restype, argtypes) in table.items():
        k = len(argtypes)
        assert compare_prototypes(header, {**table, name: (restype, argtypes[:-1])}) == [f"{name}: {k} parameters, the table has {k - 1}"]
    assert re.search(r"#define MIRT_VERSION 3\b", open(os.path.join(ROOT, "include", "mirt.h")).read())


def test_library_exports_the_symbols_and_the_signatures_are_applied():
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    for name, ret, _ in SYMBOLS:
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
        f = getattr(MOD.lib(), name)
        restype, argtypes = MOD.CAST_LISTS_SIGNATURES[name]
        assert f.restype is restype is C.c_int and list(f.argtypes) == argtypes, name
    for name in NAMES:
        assert getattr(m, name) is getattr(MOD, name) is getattr(api, name) and name in m.__all__, name
    assert m.pack_casts is api.pack_casts and not hasattr(MOD, "pack_casts") and not hasattr(MOD, "unpack_words")      # (the existing ones)


def test_null_scene_is_an_argument_error():
    calls = {"mirt_cast_counts": [(None, 0, None, 0, None), (None, 5, None, 1, None), (None, -1, None, 0, None)],
             "mirt_cast_list": [(None, 0, None, None, None, 0, 0, None), (None, 5, None, None, None, 7, 1, None), (None, -1, None, None, None, -1, 0, None)]}
    for name, _, _ in SYMBOLS:
        for args in calls[name]:
            # (another call's message first, so that the one read back is this call's)
            assert m.lib().mirt_build_lbvh(None, None, None) == 3 and name.encode() not in m.lib().mirt_last_error()
            assert getattr(MOD.lib(), name)(None, *args) == 3
            assert m.lib().mirt_last_error() == name.encode() + b": null scene"


def test_the_module_needs_neither_torch_nor_numpy():
    code = "import sys; import cuda_ray_tracer_amd.cast_lists; assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_depends_on_the_header_and_the_sources():
    deps = [os.path.normpath(d) for d in B._all_deps()]
    for path in (HEADER, *(os.path.join(B.CSRC, f) for f in ("cast_lists.hip", "cast_tests.h", "spherecast.hip", "list_cursor.h", "point_query.h", "query_walk.h"))):
        assert os.path.normpath(path) in deps, path
    assert "cast_lists.hip" in B.LIB_SOURCES and "spherecast.hip" in B.LIB_SOURCES
    assert "mirt_cast_lists.h" in os.listdir(os.path.join(ROOT, "include_ext3"))      # (the folder's listing is not pinned)


def test_no_other_header_or_table_names_the_new_symbols():
    texts = {"mirt.h": open(os.path.join(ROOT, "include", "mirt.h")).read(), **{x.header: open(_header_path(x)).read() for x in EXTENSIONS},
             "mirt_overlap_tris.h": open(os.path.join(ROOT, "include_ext2", "mirt_overlap_tris.h")).read()}
    assert len(texts) == 12
    for name, _, _ in SYMBOLS:
        assert name not in binding.SIGNATURES
        for header, text in texts.items():
            assert mentions(text, name) == [], (name, header)
        for x in EXTENSIONS:
            assert name not in _table(x), (name, x.table)


def test_the_candidate_functions_have_one_copy():
    """cast_tests.h holds the contact parameters and the slab interval; both kernels' files include it and restate none of it."""
    read = lambda name: open(os.path.join(B.CSRC, name)).read()
    shared = ("float triangle_cast(", "float sphere_cast(", "float plane_cast(", "float edge_cast(", "void box_interval(", "constexpr float TAU")
    assert all(w in read("cast_tests.h") for w in shared)
    for src in ("spherecast.hip", "cast_lists.hip"):
        text = read(src)
        assert '#include "cast_tests.h"' in text and not any(w in text for w in shared), src
    text = read("cast_lists.hip")
    assert '#include "list_cursor.h"' in text and "list_room(" in text and "lim < capacity" not in text
    assert "atomic" not in text and "right_first" not in text and "wins_tie" not in text and text.count("stack_pop(") == 1


def test_the_header_spells_out_the_sets_source_the_once_rule_the_order_and_the_bounded_writes():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    # the set is referred to by the defining header's file name and sections, not restated -- and the sections exist
    assert "Nothing about a candidate's parameter is restated here" in text and "include_ext/mirt_spherecast.h" in text
    defining = " ".join(open(os.path.join(ROOT, "include_ext", "mirt_spherecast.h")).read().replace(" *", " ").split())
    for section in ("Row rule", "Helpers", "Sphere", "Plane rule", "Plane j", "Triangle"):
        assert '"%s"' % section in text and section in defining, section
    assert "sqrtf" not in text and "h2" not in text and "fabsf" not in text and "dot(" not in text
    for words in ("0 <= t < tmax", "A surface appears ONCE, with the parameter of its FIRST contact", "0 when the ball touches or overlaps it at the start",
                  "A sphere gives one word, also for r = 0", "this is not the pair of crossings a ray list holds",
                  "Clause (0)", "OWN BUILDER BOX", "the very operations mirt_build_lbvh makes a leaf's box with", "bound = tmax + tmax",
                  "+inf stays +inf", "enter > fminf(leave, bound) is false", "Why it is part of the definition", "nearly along the edge",
                  "it does not depend on the tree, its inner boxes or any visiting order", "the only primitive of a scene",
                  "kind << 30 | id", "bit for bit", "first the planes of L_i, ascending by index", "LEAF ORDER", "ties in input order",
                  "A rebuild after a geometry update may reorder a row", "t's bits << 32 | word", "(t, kind, id)",
                  "L_i is empty exactly where that call misses",
                  "min(|L_i|, d_offsets[i + 1] - d_offsets[i])", "never write outside [0, capacity)", "keeps its tail untouched",
                  "a row that is not live writes nothing and does not read its offsets", "A row that is not live writes 0",
                  "no allocation, no synchronisation, no atomics", "One lane per row", "touches no render context",
                  "Every message names mirt_cast_counts", "Every message names mirt_cast_list", "ranges that only touch do not overlap"):
        assert words in text, words
    assert text.count("flags: must be 0") == 2


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    Q, Of, W, V = torch.zeros((4, 8)), torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros(9)
    Cn = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        m.count_casts(raw, Q.double())
    with pytest.raises(ValueError, match="dtype"):
        m.count_casts(raw, Q, Cn.float())
    with pytest.raises(ValueError, match="shape"):
        m.count_casts(raw, torch.zeros((4, 4)))
    with pytest.raises(ValueError, match="shape"):
        m.count_casts(raw, Q, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        m.count_casts(raw, torch.zeros((4, 16))[:, ::2])
    with pytest.raises(ValueError, match="cuda"):
        m.count_casts(raw, Q)
    with pytest.raises(ValueError, match="dtype"):
        m.cast_list(raw, Q.double(), Of, W)
    with pytest.raises(ValueError, match="dtype"):
        m.cast_list(raw, Q, Of.int(), W)
    with pytest.raises(ValueError, match="dtype"):
        m.cast_list(raw, Q, Of, W.long())
    with pytest.raises(ValueError, match="dtype"):
        m.cast_list(raw, Q, Of, W, V.double())
    with pytest.raises(ValueError, match="dtype"):
        m.cast_list(raw, Q, Of, W, W)                                   # (values are float32)
    with pytest.raises(ValueError, match="shape"):
        m.cast_list(raw, torch.zeros((4, 4)), Of, W)
    with pytest.raises(ValueError, match="shape"):
        m.cast_list(raw, Q, torch.zeros(4, dtype=torch.int64), W)       # (n + 1 offsets)
    with pytest.raises(ValueError, match="shape"):
        m.cast_list(raw, Q, Of, torch.zeros((3, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.cast_list(raw, Q, Of, W, torch.zeros(8))                      # (a value per word)
    with pytest.raises(ValueError, match="contiguous"):
        m.cast_list(raw, Q, Of, torch.zeros(18, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.cast_list(raw, Q, Of, W, torch.zeros(18)[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.cast_list(raw, Q, Of, W)
    with pytest.raises(ValueError, match="cuda"):
        m.cast_list(raw, Q, Of, W, V)
    with pytest.raises(ValueError, match="dtype"):
        m.cast_lists(raw, Q.double())
    with pytest.raises(ValueError, match="shape"):
        m.cast_lists(raw, torch.zeros(32))
    with pytest.raises(ValueError, match="cuda"):
        m.cast_lists(raw, Q, sort=True)


# ---- code generation ----------------------------------------------------------------------------------------------------------------
# kernel: (VGPRs, waves per SIMD) the compiler reported: at 6 waves (80 VGPRs) it spills 9, 13 and 13 registers
PINNED = {"count": (92, 5), "words": (96, 5), "values": (96, 5)}


def test_kernel_codegen_has_no_spill_one_scratch_store_and_dword_stores_only():
    """cast_lists.hip compiled for gfx950, from the compiler's report: three kernels -- the count, the fill without and with the
    value array --, none with a register spill or an AGPR, each with the 20-entry LDS stack per lane of a 256-thread block, the
    private segment of trace_rays_kernel (the stack's spill array and nothing else) and exactly one scratch store, the push of a
    stack entry beyond the LDS part.  Registers and waves per SIMD as pinned above.  No atomic anywhere.  The count has one global
    store, the row's count; the plane loop and the walk each hold a copy of the emission: one global_store_dword per copy without
    values, two with."""
    res, asm = _resource_usage("cast_lists.hip")
    by = {("count" if "cast_count_kernel" in k else "values" if "ILb1E" in k else "words"): k for k in res}
    assert sorted(by) == sorted(PINNED) and len(res) == 3, list(res)
    assert "cast_list_kernelILb0E" in by["words"] and "cast_list_kernelILb1E" in by["values"]
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    emissions = 2
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
        assert all(t.startswith("global_store_dword ") for t in stores), (key, stores)
        assert len(stores) == {"count": 1, "words": emissions, "values": 2 * emissions}[key], (key, stores)


# ---- the inputs (the GPU tests use the same) ---------------------------------------------------------------------------------------------
def _dense_case():
    """dense_scene_text() -- 300 spheres, 200 triangles, 2 planes -- and 800 rows about it: half with a finite tmax, and rows that are
    not live (tmax 0, r < 0, a NaN origin, no direction) mixed in."""
    text = dense_scene_text()
    rows = tsa.casts_about(tsa._arrays(text), 800, 61, 1.0, 0.5)
    rng = np.random.default_rng(62)
    finite = rng.random(800) < 0.5
    rows[finite, 3] = rng.uniform(0.5, 6.0, int(finite.sum())).astype(f32)
    rows[5::40, 3] = 0.0
    rows[15::40, 7] = -1.0
    rows[25::40, 0] = np.nan
    rows[35::40, 4:7] = 0.0
    return text, rows


CASES = {**tsa.CASES, "dense": _dense_case}
NEGATIVE = ("far_1e3", "far_1e5", "chosen", "along_edges")


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, arrays, rows) of a case."""
    text, rows = CASES[name]()
    return text, tsa._arrays(text), rows


@functools.lru_cache(maxsize=None)
def tree(name):
    return _oracle_tree(case(name)[0])[1:]


@functools.lru_cache(maxsize=None)
def reference(name):
    """((offsets int64 [n + 1], words uint32, t float32), candidates) of a case: what the GPU tests compare against."""
    _, arrays, rows = case(name)
    cands = sr.candidates(arrays, rows)
    return clr.lists(arrays, rows, tree(name)[1], cands), cands


def _planes_first(offsets, words):
    kind, pid = olr.unpack(words)
    for i in np.flatnonzero(np.diff(offsets) > 0)[:200]:
        k, p = kind[offsets[i]:offsets[i + 1]], pid[offsets[i]:offsets[i + 1]]
        npl = int(np.sum(k == 3))
        assert np.all(k[:npl] == 3) and np.all(np.diff(p[:npl]) > 0) and np.all(k[npl:] != 3)
        assert len(set(zip(k.tolist(), p.tolist()))) == len(k)      # a surface appears once


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_walk_emits_the_reference_and_sorted_rows_begin_with_the_first_contact(name):
    text, arrays, rows = case(name)
    nodes, refs = tree(name)
    (offsets, words, t), cands = reference(name)
    n = len(rows)
    assert offsets.dtype == np.int64 and offsets.shape == (n + 1,) and offsets[0] == 0
    assert words.dtype == u32 and t.dtype == f32 and len(words) == len(t) == offsets[n]
    # clause (0) is made of the scene's arrays: the builder's leaf boxes and the scene's box are what the arrays give ...
    if len(refs) >= 2:
        lo, hi = clr.builder_boxes(arrays)
        tlo, thi = clr.leaf_boxes(nodes, refs, arrays)
        assert np.array_equal(lo, tlo) and np.array_equal(hi, thi)
        assert float(clr.scene_coord_max(arrays)) == max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"))
    # ... and it removes nothing from the brute force's admitted set on these inputs
    plain = clr.lists(arrays, rows, refs, cands, clause=False)
    assert all(np.array_equal(a, b) for a, b in zip(plain[:2], (offsets, words))) and np.array_equal(clr.bits(plain[2]), clr.bits(t))
    # the walk as the kernel makes it: the reference's words and t bits in the reference's order
    walked = clr.walk(arrays, rows, nodes, refs, cands)
    assert len(walked) == n and [len(w) for w, _ in walked] == np.diff(offsets).tolist()
    assert np.array_equal(np.concatenate([w for w, _ in walked]), words)
    assert np.array_equal(clr.bits(np.concatenate([v for _, v in walked])), clr.bits(t))
    assert np.all(t >= 0) and not np.any(np.signbit(t))                  # (so the bits order as unsigned integers)
    assert np.all(np.diff(offsets)[~sr.live_rows(rows)] == 0)
    _planes_first(offsets, words)
    # every sorted row begins with the first contact's (t, kind, id), and is empty exactly on a miss
    hits, _ = sr.brute_force(arrays, rows, cands)
    for i, row in enumerate(clr.sorted_rows(offsets, words, t)):
        if hits[i, 1] == 0:
            assert len(row) == 0, i
        else:
            assert len(row) and row[0].tolist() == hits[i, :3].astype(np.int64).tolist(), i
    # the sets do not depend on the visiting order; the order of a row does
    if name in ("dense", "mixed", "far_1e3"):
        some = slice(0, 300)
        sub = tuple(c[some] for c in cands)
        other = clr.walk(arrays, rows[some], nodes, refs, sub, left_first=False)
        assert all(np.array_equal(np.sort(a[0]), np.sort(b[0])) for a, b in zip(walked[some], other))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(walked[some], other))
    lens = np.diff(offsets)
    if name == "dense":
        kinds = set(olr.unpack(words)[0].tolist())
        dead = ~sr.live_rows(rows)
        print(f"dense: not empty {np.mean(lens > 0):.3f}, more than 8: {np.mean(lens > 8):.3f}, longest {lens.max()}, finite tmax {np.mean(np.isfinite(rows[:, 3])):.2f}")
        assert np.mean(lens > 8) > 0.10 and kinds == {1, 2, 3} and dead.sum() == 80 and np.all(lens[dead] == 0)
        assert 0.4 < np.mean(np.isfinite(rows[:, 3])) < 0.6 and np.any(t == 0) and np.any(t > 0)
    if name == "deep_stack":
        assert len(rows) == 240 and lens.max() == 3000


@pytest.mark.parametrize("name", NEGATIVE)
def test_without_the_slacks_the_walk_loses_words(name):
    """The negative control: sigma = 0 and tau = 0.  A float32 box does not bound a float32 contact: 61 words of far_1e3, 60 of
    far_1e5, 5 of chosen and 2 of along_edges were lost when this was written."""
    text, arrays, rows = case(name)
    nodes, refs = tree(name)
    (offsets, words, t), cands = reference(name)
    walked = clr.walk(arrays, rows, nodes, refs, cands, slack=0.0, tau=0.0)
    lost = int(offsets[-1]) - sum(len(w) for w, _ in walked)
    print(f"{name}: {lost} of {int(offsets[-1])} words lost without the slacks")
    assert all(set(w.tolist()) <= set(words[offsets[i]:offsets[i + 1]].tolist()) for i, (w, _) in enumerate(walked))      # (it adds nothing)
    assert lost >= 1


def test_fill_honours_truncating_offsets_and_a_capacity_for_words_and_values():
    (offsets, words, t), _ = reference("dense")
    total = int(offsets[-1])
    for want in (words, t):
        sentinel = np.full(total + 4, 0xdeadbeef, u32)
        whole = clr.fill(offsets, want, offsets, sentinel)
        assert np.array_equal(whole[:total], clr.bits(want) if want.dtype == f32 else want) and np.all(whole[total:] == 0xdeadbeef)
        short = olr.offsets_of(np.minimum(np.diff(offsets), 3))
        got = clr.fill(offsets, want, short, sentinel)
        i = int(np.argmax(np.diff(offsets)))
        assert got[short[i]:short[i + 1]].tolist() == np.ascontiguousarray(want[offsets[i]:offsets[i] + 3]).view(u32).tolist() and np.all(got[short[-1]:] == 0xdeadbeef)
        half = clr.fill(offsets, want, offsets, sentinel, capacity=total // 2)
        assert np.array_equal(half[:total // 2], whole[:total // 2]) and np.all(half[total // 2:] == 0xdeadbeef)
        assert np.all(clr.fill(offsets, want, offsets[::-1].copy(), sentinel) == 0xdeadbeef)
        assert np.all(clr.fill(offsets, want, offsets - total - 5, sentinel) == 0xdeadbeef)

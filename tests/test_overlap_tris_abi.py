"""Triangle overlap queries (include_ext2/mirt_overlap_tris.h: mirt_overlap_triangles, mirt_triangle_list): the header against
overlap_tris.py's signature table and the built library, the wrappers' checks, the kernels' code generation, and the numpy
restatement of the header (tests/overlap_tris_ref.py) against hand-made rows with counts written out by hand, against float64 on
random scenes, and against itself over the oracle's tree on the inputs the GPU tests use.  No GPU needed.

The header lies in include_ext2/: tests/test_extension_abi.py lists include/ and include_ext/ against its own table, so this
extension's row is here."""
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
import edge_scenes
import overlap_list_ref as olr
import overlap_tris_ref as otr
import pyscene
from codegen_lib import _kernel_body, _resource_usage, _strip
from test_binding_header import compare_prototypes, constants, prototypes
from test_closest_abi import _oracle_tree, _well_shaped_scene
from test_extension_abi import EXTENSIONS, _header_path, _table, mentions
from test_multihit_abi import dense_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext2", "mirt_overlap_tris.h")
MOD = importlib.import_module("cuda_ray_tracer_amd.overlap_tris")
PTR, I32, I64, U32 = "pointer", (4, True, False), (8, True, False), (4, False, False)
SYMBOLS = [("mirt_overlap_triangles", I32, [PTR, PTR, I64, PTR, U32, PTR]), ("mirt_triangle_list", I32, [PTR, PTR, I64, PTR, PTR, I64, PTR])]
NAMES = ("overlap_triangles", "triangle_list", "triangle_lists", "pack_triangles", "scene_triangle_rows")
f32 = np.float32
u32 = np.uint32
NAN, INF = float("nan"), float("inf")


# ---- header, table, library ------------------------------------------------------------------------------------------------------------
def test_the_header_agrees_with_the_signature_table():
    header, table = _strip(HEADER), MOD.OVERLAP_TRIS_SIGNATURES
    assert prototypes(header) == SYMBOLS
    assert [name for name, _, _ in prototypes(header)] == list(table)
    assert sorted(set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", header))) == sorted(table)
    assert compare_prototypes(header, table) == []
    assert constants(header) == {"MIRT_TRIS_ANY": 1} and MOD.MIRT_TRIS_ANY == 1
    assert re.findall(r'^#include "[./a-z]*mirt\.h"$', header, flags=re.M) == ['#include "../include/mirt.h"']
    restype, argtypes = table["mirt_triangle_list"]
    doctored = {**table, "mirt_triangle_list": (restype, [C.c_int if t is C.c_int64 else t for t in argtypes])}
    assert compare_prototypes(header, doctored) == [f"mirt_triangle_list: parameter {p} is (8, True, False), the table says (4, True, False)" for p in (2, 5)]
    for name, (restype, argtypes) in table.items():
        k = len(argtypes)
        assert compare_prototypes(header, {**table, name: (restype, argtypes[:-1])}) == [f"{name}: {k} parameters, the table has {k - 1}"]
    assert re.search(r"#define MIRT_VERSION 3\b", open(os.path.join(ROOT, "include", "mirt.h")).read())


def test_library_exports_the_symbols_and_the_signatures_are_applied():
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    for name, ret, _ in SYMBOLS:
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
        f = getattr(MOD.lib(), name)
        restype, argtypes = MOD.OVERLAP_TRIS_SIGNATURES[name]
        assert f.restype is restype is C.c_int and list(f.argtypes) == argtypes, name
    for name in NAMES:
        assert getattr(m, name) is getattr(MOD, name) is getattr(api, name) and name in m.__all__, name


def test_null_scene_is_an_argument_error():
    calls = {"mirt_overlap_triangles": [(None, 0, None, 0, None), (None, 5, None, 1, None)],
             "mirt_triangle_list": [(None, 0, None, None, 0, None), (None, 5, None, None, 7, None), (None, -1, None, None, -1, None)]}
    for name, _, _ in SYMBOLS:
        for args in calls[name]:
            # (another call's message first, so that the one read back is this call's)
            assert m.lib().mirt_build_lbvh(None, None, None) == 3 and name.encode() not in m.lib().mirt_last_error()
            assert getattr(MOD.lib(), name)(None, *args) == 3
            assert m.lib().mirt_last_error() == name.encode() + b": null scene"


def test_the_module_needs_neither_torch_nor_numpy():
    code = "import sys; import cuda_ray_tracer_amd.overlap_tris; assert 'torch' not in sys.modules and 'numpy' not in sys.modules, sorted(sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_build_depends_on_the_header_and_the_sources():
    deps = [os.path.normpath(d) for d in B._all_deps()]
    for path in (HEADER, *(os.path.join(B.CSRC, f) for f in ("overlap_tris.hip", "tri_tests.h", "list_cursor.h", "point_query.h", "query_walk.h"))):
        assert os.path.normpath(path) in deps, path
    assert "overlap_tris.hip" in B.LIB_SOURCES
    assert sorted(os.listdir(os.path.join(ROOT, "include_ext2"))) == ["mirt_overlap_tris.h"]


def test_no_other_header_or_table_names_the_new_symbols():
    texts = {"mirt.h": open(os.path.join(ROOT, "include", "mirt.h")).read(), **{x.header: open(_header_path(x)).read() for x in EXTENSIONS}}
    assert len(texts) == 11
    for name, _, _ in SYMBOLS:
        assert name not in binding.SIGNATURES
        for header, text in texts.items():
            assert mentions(text, name) == [], (name, header)
        for x in EXTENSIONS:
            assert name not in _table(x), (name, x.table)
    assert not hasattr(binding, "MIRT_TRIS_ANY")
    # ... and this header names no other extension's entry point, in its comments either
    raw = open(HEADER).read()
    assert [s.name for x in EXTENSIONS for s in x.symbols if s.name in raw] == []


def test_the_header_spells_out_the_set():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    for words in ("never over the tree", "A row without area", "is dead", "Common origin", "PROPERTY", "shares a vertex", "SEVENTEEN AXES",
                  "a zero axis projects everything to 0 and never separates", "the last six decide the coplanar case", "A NaN admits nothing",
                  "A triangle wholly inside a sphere does not touch it", "rmax < smin || smax < rmin", "dn <= rs", "df >= rs",
                  "the very operations mirt_build_lbvh makes a sphere's leaf box with", "first the planes of A_i, ascending by index", "LEAF ORDER",
                  "min(|A_i|, d_offsets[i + 1] - d_offsets[i])", "never write outside [0, capacity)", "a row that is not live writes nothing",
                  "no allocation, no synchronisation, no atomics", "touches no render context"):
        assert words in text, words


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None, desc=types.SimpleNamespace(num_triangles=4))
    T, Of, W, Cn = torch.zeros((4, 9)), torch.zeros(5, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_triangles(raw, T.double())
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_triangles(raw, T, Cn.float())
    with pytest.raises(ValueError, match="shape"):
        m.overlap_triangles(raw, torch.zeros((4, 8)))
    with pytest.raises(ValueError, match="shape"):
        m.overlap_triangles(raw, T, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        m.overlap_triangles(raw, torch.zeros((4, 18))[:, ::2])
    with pytest.raises(ValueError, match="cuda"):
        m.overlap_triangles(raw, T, any=True)
    with pytest.raises(ValueError, match="dtype"):
        m.triangle_list(raw, T, Of.int(), W)
    with pytest.raises(ValueError, match="dtype"):
        m.triangle_list(raw, T, Of, W.long())
    with pytest.raises(ValueError, match="shape"):
        m.triangle_list(raw, T, torch.zeros(4, dtype=torch.int64), W)
    with pytest.raises(ValueError, match="shape"):
        m.triangle_list(raw, torch.zeros((4, 3, 3)), Of, W)
    with pytest.raises(ValueError, match="cuda"):
        m.triangle_list(raw, T, Of, W)
    with pytest.raises(ValueError, match="cuda"):
        m.triangle_lists(raw, T, sort=True)
    with pytest.raises(ValueError, match="the scene has 4 triangles"):
        m.scene_triangle_rows(raw, first=2, count=3)
    with pytest.raises(ValueError, match="the scene has 4 triangles"):
        m.scene_triangle_rows(raw, first=-1)
    v = torch.arange(18, dtype=torch.float64).reshape(2, 3, 3)
    rows = m.pack_triangles(v)
    assert rows.shape == (2, 9) and rows.dtype == torch.float32 and rows.is_contiguous() and rows[1].tolist() == list(range(9, 18))
    assert torch.equal(m.pack_triangles(rows), rows) and m.pack_triangles(np.zeros((0, 9))).shape == (0, 9)
    with pytest.raises(ValueError, match="shape"):
        m.pack_triangles(torch.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="shape"):
        m.pack_triangles(torch.zeros(9))


# ---- code generation ----------------------------------------------------------------------------------------------------------------
PINNED = (96, 5)      # (VGPRs, waves per SIMD) the compiler reported for every instance


def test_kernel_codegen_has_no_vgpr_spill_and_one_scratch_store():
    """overlap_tris.hip compiled for gfx950, from the compiler's report: three kernels -- count, any, fill --, none with a VGPR
    spill or an AGPR, each with the 20-entry LDS stack per lane of a 256-thread block, the private segment of trace_rays_kernel (the
    stack's spill array and nothing else) and exactly one scratch store, the push of a stack entry beyond the LDS part."""
    res, asm = _resource_usage("overlap_tris.hip")
    assert len(res) == 3 and len([k for k in res if "overlap_tris_kernel" in k]) == 2 and len([k for k in res if "triangle_list_kernel" in k]) == 1, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    for k, r in res.items():
        print(k, r)
        assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, (k, r)
        assert {r["ScratchSize [bytes/lane]"]} == private, (k, r)
        assert r["VGPRs"] <= PINNED[0] and r["Occupancy [waves/SIMD]"] >= PINNED[1], (k, r)
        assert len([t for t in _kernel_body(asm, k) if t.startswith("scratch_store")]) == 1, k


# ---- hand-made rows: the counts written out by hand ----------------------------------------------------------------------------------
# Sphere 0: centre (0, 0, -10), radius 2.  Triangle 0: (0, 0, 0) (4, 0, 0) (0, 4, 0), in z = 0.  Plane 0: z = -16.  Every coordinate
# is dyadic, so every operation of the tests is exact.
HAND = """png 8 8 hand.png
sphere 0 0 -10 2
xyz 0 0 0
xyz 4 0 0
xyz 0 4 0
tri 1 2 3
plane 0 0 1 16
"""
# (a, b, c, the count, the kind admitted)
HAND_ROWS = [
    ((1, 1, 0), (3, 1, 0), (1, 3, 0), 1, 2),               # 0: coplanar and overlapping
    ((3, 3, 0), (5, 3, 0), (3, 5, 0), 0, 0),               # 1: coplanar and disjoint (beyond x + y = 4), the bounds meeting: only the in-plane axes separate
    ((0, 0, 0), (-2, 0, 1), (0, -2, 1), 1, 2),             # 2: a shared vertex
    ((0, 0, 0), (4, 0, 0), (2, 0, 3), 1, 2),               # 3: a shared edge
    ((1, 1, -1), (1, 1, 1), (2, 1, 1), 1, 2),              # 4: piercing: the edge a-b goes through (1, 1, 0)
    ((1, 1, -1), (3, 1, -1), (2, 1, 1), 1, 2),             # 5: parallel edges (a-b and the triangle's along x: a zero axis), crossing it
    ((3, 3, -1), (5, 3, -1), (4, 3, 1), 0, 0),             # 6: parallel edges, the bounds meeting, disjoint (it crosses z = 0 at x >= 3.5, y = 3)
    ((1, 1, 0), (1, 1, 2), (2, 1, 2), 1, 2),               # 7: a vertex touching the face
    ((0, 0, -10), (0.5, 0, -10), (0, 0.5, -10), 0, 0),     # 8: inside the sphere: no touch
    ((0, 0, -10), (3, 0, -10), (0, 3, -10), 1, 1),         # 9: crossing the sphere's surface
    ((-1, -1, -8), (1, -1, -8), (0, 1, -8), 1, 1),         # 10: outside and tangent at the pole (0, 0, -8): dn == rs
    ((-1, -1, -7), (1, -1, -7), (0, 1, -7), 0, 0),         # 11: outside
    ((0, 0, -17), (1, 0, -15), (0, 1, -15), 1, 3),         # 12: straddling the plane
    ((0, 0, -16), (1, 0, -15), (0, 1, -15), 1, 3),         # 13: touching the plane with one vertex
    ((0, 0, -15.5), (1, 0, -15), (0, 1, -15), 0, 0),       # 14: on one side of it
    ((1, 1, 2), (0, 0, -10), (2, 1, 2), 2, 0),             # 15: a long one: b at the sphere's centre, the edge a-b through triangle 0 at (5/6, 5/6, 0)
    ((NAN, 1, 0), (3, 1, 0), (1, 3, 0), 0, 0),             # 16: dead: a NaN (row 0 otherwise)
    ((1, 1, 0), (3, INF, 0), (1, 3, 0), 0, 0),             # 17: dead: an infinity
    ((1, 1, 0), (2, 1, 0), (3, 1, 0), 0, 0),               # 18: dead: no area (collinear, lying across triangle 0)
    ((1, 1, 0), (1, 1, 0), (1, 1, 0), 0, 0),               # 19: dead: a point on triangle 0
]


def hand_rows():
    return np.array([[*a, *b, *c] for a, b, c, _, _ in HAND_ROWS], f32)


def _arrays(text):
    return pyscene.parse_lines(text.split("\n")).arrays()


def test_the_hand_made_rows_have_the_counts_written_by_hand():
    arrays, rows = _arrays(HAND), hand_rows()
    ps, pt, pp = otr.passes(arrays, rows)
    got = otr.counts(arrays, rows)
    assert got.tolist() == [r[3] for r in HAND_ROWS]
    for i, (_, _, _, count, kind) in enumerate(HAND_ROWS):
        if kind:
            assert count == 1 and [ps[i, 0], pt[i, 0], pp[i, 0]] == [kind == 1, kind == 2, kind == 3], i
    assert ps[15, 0] and pt[15, 0] and not pp[15, 0]
    assert otr.live_rows(rows).tolist() == [True] * 16 + [False] * 4


def test_only_the_in_plane_axes_separate_the_coplanar_disjoint_pair():
    arrays, rows = _arrays(HAND), hand_rows()
    a, b, c, ub, uc, lo, hi = otr.row_quantities(rows[1:2])
    T = arrays["triangles"]
    near, area, sep = otr.triangle_clauses(lo, hi, a, ub, uc, T["p0"], T["p1"], T["p2"])
    assert near.tolist() == [True] and area.tolist() == [True]
    assert not sep[:11].any() and sep[11:].any()      # the first eleven alone would admit it
    assert otr.passes(arrays, rows[1:2], axes=11)[1].tolist() == [[True]] and otr.passes(arrays, rows[1:2])[1].tolist() == [[False]]
    # parallel edges make a zero axis, which separates nothing: row 5's a-b against the triangle's p-q
    a, b, c, ub, uc, lo, hi = otr.row_quantities(rows[5:6])
    axes = otr.triangle_axes(ub, uc, T["p0"] - a, T["p1"] - a, T["p2"] - a)
    assert not axes[2].any() and not otr.triangle_clauses(lo, hi, a, ub, uc, T["p0"], T["p1"], T["p2"])[2][2].any()


# ---- the inputs (the GPU tests use the same) -----------------------------------------------------------------------------------------
def triangles_about(arrays, n, seed, pad=0.3, smin=0.05, smax=1.5):
    """n triangles: a uniform in the box of the scene's points grown by `pad`, b and c at log-uniform distances smin..smax from it."""
    pts = [arrays["spheres"]["c"]] + [arrays["triangles"][k] for k in ("p0", "p1", "p2")]
    pts = np.concatenate([p.reshape(-1, 3) for p in pts] + [np.zeros((1, 3))]).astype(np.float64)
    rng = np.random.default_rng(seed)
    a = rng.uniform(pts.min(axis=0) - pad, pts.max(axis=0) + pad, (n, 3))
    out = [a]
    for _ in range(2):
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        out.append(a + d * np.exp(rng.uniform(np.log(smin), np.log(smax), (n, 1))))
    return np.concatenate(out, axis=1).astype(f32)


def dead_rows():
    return hand_rows()[16:]


@functools.lru_cache(maxsize=None)
def dense_case():
    """(text, rows): the dense scene (300 spheres, 200 triangles, 2 planes) and 2004 shuffled rows: 1400 triangles of size 0.05 to
    1.5, 400 larger ones (1 to 4: more than eight surfaces), the scene's own 200 triangles, the dead rows."""
    text = dense_scene_text()
    arrays = _arrays(text)
    rows = np.concatenate([triangles_about(arrays, 1400, 71), triangles_about(arrays, 400, 72, smin=1.0, smax=4.0), otr.scene_rows(arrays), dead_rows()])
    assert rows.shape == (2004, 9)
    return text, np.ascontiguousarray(rows[np.random.default_rng(3).permutation(len(rows))])


@functools.lru_cache(maxsize=None)
def far_case():
    """(text, rows): far_from_origin at 1e5 (300 spheres, a plane) with 60 triangles of its own size there, 600 rows about it and
    those 60 triangles as rows."""
    rng = np.random.default_rng(81)
    lines = [edge_scenes.far_from_origin(offset=100000.0)]
    for _ in range(60):
        v = rng.uniform(-1, 1, 3) + rng.uniform(-0.4, 0.4, (3, 3))
        lines += ["xyz %.4f %.4f %.4f\n" % (100000.0 + p[0], p[1], p[2]) for p in v] + ["tri -3 -2 -1\n"]
    text = "".join(lines)
    arrays = _arrays(text)
    assert len(arrays["triangles"]) == 60
    rows = triangles_about(arrays, 600, 82, pad=0.1, smin=0.05, smax=0.6)
    rows[:, 0::3] += f32(100000.0) - rows[:, 0:1]      # (the box of the points includes the origin: put every row at the scene)
    rows[:, 0::3] += rng.uniform(-1, 1, (600, 1)).astype(f32)
    return text, np.concatenate([rows, otr.scene_rows(arrays)]).astype(f32)


@functools.lru_cache(maxsize=None)
def deep_case():
    """(text, rows): deep_stack(600) -- concentric spheres of radius 0.5 to 0.9 about (0, 0, -3) -- and 120 rows with a near the
    centre: those that reach beyond 0.9 cross every shell."""
    text = edge_scenes.deep_stack(600)
    rng = np.random.default_rng(91)
    a = np.array([0, 0, -3.0]) + rng.uniform(-0.2, 0.2, (120, 3))
    d = rng.standard_normal((2, 120, 3))
    d /= np.linalg.norm(d, axis=2)[..., None]
    reach = rng.uniform(0.3, 2.0, (2, 120, 1))
    return text, np.concatenate([a, a + d[0] * reach[0], a + d[1] * reach[1]], axis=1).astype(f32)


def mesh_text(k=5, seed=17):
    """A k x k grid of quads over [0, k]^2, each split in two, with random heights: 2 k^2 triangles that share vertices bit for
    bit (the file names each vertex once)."""
    rng = np.random.default_rng(seed)
    lines = ["png 8 8 mesh.png\n"]
    for y in range(k + 1):
        for x in range(k + 1):
            lines.append("xyz %.4f %.4f %.4f\n" % (x + rng.uniform(-0.2, 0.2), y + rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5)))
    at = lambda x, y: y * (k + 1) + x + 1
    for y in range(k):
        for x in range(k):
            lines.append("tri %d %d %d\n" % (at(x, y), at(x + 1, y), at(x, y + 1)))
            lines.append("tri %d %d %d\n" % (at(x + 1, y), at(x + 1, y + 1), at(x, y + 1)))
    return "".join(lines)


@functools.lru_cache(maxsize=None)
def mesh_case():
    text = mesh_text()
    return text, otr.scene_rows(_arrays(text))


MOVED_TRI = np.array([[0.5, 0.5, -3.0, 2.5, 0.5, -2.0, 0.5, 2.5, -2.5]], f32)      # what triangle 0 of the moved case becomes


@functools.lru_cache(maxsize=None)
def moved_case():
    """(text after the update, rows): the well-shaped scene with its triangle 0 moved to MOVED_TRI, and 500 rows."""
    text = _well_shaped_scene()
    lines = text.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith("xyz")][:3]
    for i, v in zip(at, MOVED_TRI.reshape(3, 3)):
        lines[i] = "xyz %.4f %.4f %.4f" % tuple(v)
    moved = "\n".join(lines)
    arrays = _arrays(moved)
    assert np.array_equal(otr.scene_rows(arrays)[0], MOVED_TRI[0])
    return moved, np.concatenate([triangles_about(arrays, 500, 95, smin=0.2, smax=2.0), MOVED_TRI])


def small_case(name):
    text = edge_scenes.ALL[name]()
    rng = np.random.default_rng(5)
    a = rng.uniform(-3, 3, (100, 3))
    a[:, 2] -= 2
    return text, np.concatenate([a, a + rng.uniform(-2, 2, (100, 3)), a + rng.uniform(-2, 2, (100, 3))], axis=1).astype(f32)


CASES = {"hand": lambda: (HAND, hand_rows()), "dense": dense_case, "far_1e5": far_case, "deep_stack": deep_case, "mesh": mesh_case, "moved": moved_case,
         **{name: functools.partial(small_case, name) for name in ("empty", "plane_only", "single_triangle")}}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(counts uint32 [n], offsets int64 [n + 1], words uint32) of a case by the brute force, in the oracle tree's leaf order: what
    the GPU tests compare against."""
    text, rows = CASES[name]()
    arrays, _, refs = _oracle_tree(text)
    adm = otr.admitted(arrays, rows)
    offsets, words = otr.lists(arrays, rows, refs, adm=adm)
    counts = otr.counts(arrays, rows, adm=adm)
    assert np.array_equal(np.diff(offsets), counts.astype(np.int64))
    for a in (counts, offsets, words):
        a.setflags(write=False)
    return counts, offsets, words


def test_the_dense_case_meets_its_conditions():
    counts, offsets, words = reference("dense")
    kind, _ = olr.unpack(words)
    print(f"dense: non-empty {np.mean(counts > 0):.3f}, more than 8: {np.mean(counts > 8):.3f}, max {counts.max()}, kinds {np.bincount(kind)[1:]}")
    assert np.mean(counts > 0) >= 0.10 and set(kind.tolist()) == {1, 2, 3} and np.mean(counts > 8) > 0.02
    _, rows = CASES["dense"]()
    assert np.all(counts[~otr.live_rows(rows)] == 0) and (~otr.live_rows(rows)).sum() == 4


def test_the_other_cases_have_what_their_tests_need():
    counts, _, words = reference("deep_stack")
    assert counts.max() == 600 and np.mean(counts > 500) > 0.2
    counts, _, words = reference("far_1e5")
    assert set(olr.unpack(words)[0].tolist()) == {1, 2, 3} and 0.1 < np.mean(counts > 0)
    assert reference("empty")[0].max() == 0 and set(olr.unpack(reference("plane_only")[2])[0].tolist()) == {3}
    assert set(olr.unpack(reference("single_triangle")[2])[0].tolist()) == {2}
    counts, _, _ = reference("hand")
    assert counts.tolist() == [r[3] for r in HAND_ROWS]


def test_triangles_that_share_a_vertex_or_an_edge_always_touch():
    """The header's PROPERTY on a mesh: every row of the scene's own triangles admits itself and every triangle that shares a vertex
    with it, bit for bit -- and the mesh, a height field, meets itself nowhere else."""
    text, rows = CASES["mesh"]()
    arrays = _arrays(text)
    _, pt, _ = otr.passes(arrays, rows)
    v = rows.reshape(-1, 3, 3)
    shares = np.array([[any(np.array_equal(p, q) for p in v[i] for q in v[j]) for j in range(len(v))] for i in range(len(v))])
    assert shares.sum() > 6 * len(v) and np.all(np.diag(shares))
    assert np.array_equal(pt, shares)
    # ... and so at 1e5, where a coordinate's ulp is 0.008: each row touches itself
    text, rows = CASES["far_1e5"]()
    _, pt, _ = otr.passes(_arrays(text), rows[-60:])
    assert np.all(np.diag(pt))


# ---- the restatement against float64 -------------------------------------------------------------------------------------------------
def _closest_f64(a, b, c, q):
    """The closest point of triangle (a, b, c) to q in float64, by other means than the header's: the projection onto the plane if
    it falls inside, else the nearest point of the three edges."""
    n = np.cross(b - a, c - a)
    p = q - n * ((q - a) @ n) / (n @ n)
    inside = all(np.cross(v - u, p - u) @ n >= 0 for u, v in ((a, b), (b, c), (c, a)))
    if inside:
        return p
    best = None
    for u, v in ((a, b), (b, c), (c, a)):
        t = min(1.0, max(0.0, ((q - u) @ (v - u)) / ((v - u) @ (v - u))))
        x = u + t * (v - u)
        if best is None or np.linalg.norm(q - x) < np.linalg.norm(q - best):
            best = x
    return best


def _sat_f64(r, s):
    """(the largest normalised gap over the seventeen axes -- above 0: separated by that distance; below: every axis overlaps by
    at least that much --, the same over the well-conditioned axes only) of triangles r and s ([3, 3] each) in float64."""
    e = [r[1] - r[0], r[2] - r[1], r[0] - r[2]]
    f = [s[1] - s[0], s[2] - s[1], s[0] - s[2]]
    n1, n2 = np.cross(e[0], e[1]), np.cross(f[0], f[1])
    axes = [(n1, 1.0), (n2, 1.0)]
    for x in e:
        for y in f:
            L = np.cross(x, y)
            axes.append((L, np.linalg.norm(L) / (np.linalg.norm(x) * np.linalg.norm(y))))
    axes += [(np.cross(n1, x), 1.0) for x in e] + [(np.cross(n2, y), 1.0) for y in f]
    every, good = -np.inf, -np.inf
    for L, sine in axes:
        ln = np.linalg.norm(L)
        if ln < 1e-12:
            continue
        pr, ps = r @ (L / ln), s @ (L / ln)
        gap = max(pr.min() - ps.max(), ps.min() - pr.max())
        every = max(every, gap)
        if sine > 1e-2:
            good = max(good, gap)
    return every, good


@pytest.mark.parametrize("seed", [5, 6])
def test_restatement_agrees_with_float64_on_random_scenes(seed):
    """300 random triangles (sizes 0.2 to 2) against the 40 spheres, 40 well-shaped triangles and 2 planes of section 6o's scene, in
    float64: a triangle pair by the separating axes, normalised -- clearly apart when an axis whose edges are not nearly parallel
    (sine above 0.01: its float32 direction is the float64 one to 1e-5) leaves a gap above EPS, clearly through each other when every
    axis overlaps by more than EPS; a sphere by the closest point found by projection and the farthest vertex, both clear of rs by
    EPS; a plane by the signed distances, the least and the largest clear of 0 by EPS.  EPS = 1e-5 of the pair's scale, a hundred
    float32 roundings.  Every clear pair must agree.  The pairs left out as grazing are at most 2 % of the near pairs -- those whose
    bounds meet (every plane pair is one)."""
    arrays = _arrays(_well_shaped_scene(seed=seed))
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    rows = triangles_about(arrays, 300, 60 + seed, smin=0.2, smax=2.0)
    ps, pt, pp = otr.passes(arrays, rows)
    assert ps.shape == (300, 40) and pt.shape == (300, 40) and pp.shape == (300, 2)
    R = rows.astype(np.float64).reshape(-1, 3, 3)
    lo, hi = R.min(axis=1), R.max(axis=1)
    near = grazing = checked = 0
    admitted = np.zeros(3, np.int64)
    for i in range(len(R)):
        scale = np.abs(R[i]).max() + (hi[i] - lo[i]).max()
        for j in range(len(T)):
            s = np.stack([T[k][j].astype(np.float64) for k in ("p0", "p1", "p2")])
            if not (np.all(s.min(axis=0) <= hi[i]) and np.all(s.max(axis=0) >= lo[i])):
                assert not pt[i, j]      # (clause (i) is exact)
                continue
            near += 1
            eps = 1e-5 * (scale + np.abs(s).max())
            every, good = _sat_f64(R[i], s)
            if good > eps:
                want = False
            elif every < -eps:
                want = True
            else:
                grazing += 1
                continue
            checked += 1
            admitted[1] += want
            assert pt[i, j] == want, (i, j, every, good)
        for j in range(len(S)):
            c, r = S["c"][j].astype(np.float64), float(S["r"][j])
            if not (np.all(c - r <= hi[i]) and np.all(c + r >= lo[i])):
                continue      # (the float32 box may differ in its last bit: such a pair is neither near nor checked)
            near += 1
            eps = 1e-5 * (scale + np.abs(c).max() + r)
            dn = np.linalg.norm(c - _closest_f64(*R[i], c))
            df = np.linalg.norm(R[i] - c, axis=1).max()
            if abs(dn - r) < eps or abs(df - r) < eps:
                grazing += 1
                continue
            checked += 1
            admitted[0] += dn <= r <= df
            assert ps[i, j] == (dn <= r <= df), (i, j, dn, df, r)
        for j in range(len(Pl)):
            nor, point = Pl["nor"][j].astype(np.float64), Pl["point"][j].astype(np.float64)
            sd = (R[i] - point) @ (nor / np.linalg.norm(nor))
            near += 1
            eps = 1e-5 * (scale + np.abs(point).max())
            if abs(sd.min()) < eps or abs(sd.max()) < eps:
                grazing += 1
                continue
            checked += 1
            admitted[2] += sd.min() <= 0 <= sd.max()
            assert pp[i, j] == (sd.min() <= 0 <= sd.max()), (i, j, sd)
    print(f"seed {seed}: near pairs {near}, checked {checked}, grazing {grazing} ({grazing / near:.4f}); admitted spheres, triangles, planes {admitted}")
    assert grazing <= 0.02 * near and checked > 1000 and np.all(admitted > 20)


# ---- the reference against itself over the oracle's tree --------------------------------------------------------------------------------
def _walk(arrays, rows, nodes, refs, adm, slack=2.0 ** -18, left_first=True):
    """The header's pruning rule as a walk (overlap_list_ref.walk_words' loop with the row's vertex bounds for the box): the words
    of every row."""
    _, _, _, _, _, lo, hi = otr.row_quantities(rows)
    live = otr.live_rows(rows)
    ns, nt, npl = len(arrays["spheres"]), len(arrays["triangles"]), len(arrays["planes"])
    Cm = f32(0.0) if len(nodes) <= 1 else f32(max(abs(float(nodes[0][f])) for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")))
    with np.errstate(all="ignore"):
        sigma = (np.fmax(np.abs(lo).max(axis=1), np.abs(hi).max(axis=1)) + Cm) * f32(slack)
        los, his = lo - sigma[:, None], hi + sigma[:, None]
        meets = np.ones((len(rows), len(nodes)), bool)
        for axis, (fmin, fmax) in enumerate((("xmin", "xmax"), ("ymin", "ymax"), ("zmin", "zmax"))):
            if len(nodes):
                meets &= ~(nodes[fmin][None, :] > his[:, axis:axis + 1]) & ~(nodes[fmax][None, :] < los[:, axis:axis + 1])
    left, right, count, off = (nodes[f].tolist() for f in ("left", "right", "count", "prim_offset")) if len(nodes) else ([], [], [], [])
    ty, pid = np.asarray(refs["type"]).tolist(), np.asarray(refs["id"]).tolist()
    out = []
    for i in range(len(rows)):
        got = []
        if live[i]:
            got += [int(olr.word(3, j)) for j in range(npl) if adm[i, ns + nt + j]]
            if len(nodes):
                stack, cur = [], 0
                while True:
                    if count[cur] > 0:
                        r = off[cur]
                        if adm[i, (ns + pid[r]) if ty[r] else pid[r]]:
                            got.append(int(olr.word(2 if ty[r] else 1, pid[r])))
                        pop = True
                    else:
                        x, y = (left[cur], right[cur]) if left_first else (right[cur], left[cur])
                        hx, hy = meets[i, x], meets[i, y]
                        if hx and hy:
                            stack.append(y)
                        cur = x if hx else y
                        pop = not (hx or hy)
                    if pop:
                        if not stack:
                            break
                        cur = stack.pop()
        out.append(np.array(got, u32))
    return out


@pytest.mark.parametrize("name", ["hand", "dense", "far_1e5", "mesh", "single_triangle", "plane_only", "empty"])
def test_the_pruned_left_first_walk_emits_the_brute_force(name):
    """With the header's sigma, and with none: clauses (0) and (i) are exact bounds tests, so no slack is needed."""
    text, rows = CASES[name]()
    arrays, nodes, refs = _oracle_tree(text)
    adm = otr.admitted(arrays, rows)
    counts, offsets, words = reference(name)
    for slack in (2.0 ** -18, 0.0):
        walked = _walk(arrays, rows, nodes, refs, adm, slack=slack)
        assert [len(w) for w in walked] == counts.tolist()
        assert np.array_equal(np.concatenate(walked) if len(rows) else np.zeros(0, u32), words), slack
    if name == "dense":
        other = _walk(arrays, rows, nodes, refs, adm, left_first=False)
        assert all(np.array_equal(np.sort(x), np.sort(y)) for x, y in zip(walked, other)) and any(not np.array_equal(x, y) for x, y in zip(walked, other))

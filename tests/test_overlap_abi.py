"""Box overlap queries (include_ext/mirt_overlap.h: mirt_overlap_boxes): what the header's text says, the wrappers' checks, the
kernel's code generation, and the numpy restatement of the header (tests/overlap_ref.py) against float64 by other methods and
against itself over the oracle's tree: on the inputs the GPU tests use, the pruned walk gives the brute force's bits on every row in
either child order, the any-overlap walk agrees on "non-empty", the counts are bracketed by the contact query's, and the records,
counts and order have the properties the header states.  The header against overlap.py's signature table and the built library is
a row of tests/test_extension_abi.py.  No GPU needed."""
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
import light_scenes
import overlap_ref as ovr
import pyscene
from codegen_lib import _kernel_body, _resource_usage
from test_closest_abi import _oracle_tree, _points_about, _well_shaped_scene
from test_multihit_abi import dense_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "mirt_overlap.h")
f32 = np.float32
u32 = np.uint32
u64 = np.uint64
INF = float("inf")
NAN = float("nan")


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_spells_out_the_tests_and_states_the_rules():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert "never by the tree" in text and "(dist, kind, id)" in text and "mirt_closest.h's, word for word" in text
    assert "dmin2 <= rr && dmax2 >= rr" in text and "fabsf(s) <= e" in text and "mn <= rr && mx >= -rr" in text and "mn <= h[k] && mx >= -h[k]" in text
    assert "a NaN never admits a candidate" in text and "It may lie outside the box" in text
    assert "sigma = 2^-18" in text and "There is no shrinking bound" in text and "A box without volume" in text


def test_no_other_header_of_the_folder_names_the_entry_point_in_its_comments_either():
    """(test_extension_abi.py lets a newer header speak of an older entry point in its comments; the two newer ones here do not)"""
    folder = os.path.join(ROOT, "include_ext")
    others = [name for name in os.listdir(folder) if name != "mirt_overlap.h"]
    assert len(others) >= 4
    for name in others:
        assert "mirt_overlap_boxes" not in open(os.path.join(folder, name)).read(), name


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    Bx, Hh, Cn, F = torch.zeros((4, 8)), torch.zeros((4, 3, 6), dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros((4, 3, 8))
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_boxes(raw, Bx.double(), Hh)
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_boxes(raw, Bx, Hh.to(torch.int16))
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_boxes(raw, Bx, Hh, Cn.float())
    with pytest.raises(ValueError, match="dtype"):
        m.overlap_boxes(raw, Bx, Hh, Cn, F.double())
    with pytest.raises(ValueError, match="dtype"):
        m.count_overlaps(raw, Bx.double())
    with pytest.raises(ValueError, match="dtype"):
        m.count_overlaps(raw, Bx, Cn.float())
    with pytest.raises(ValueError, match="shape"):
        m.overlap_boxes(raw, torch.zeros((4, 4)), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.overlap_boxes(raw, Bx, torch.zeros((4, 18), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.overlap_boxes(raw, Bx, torch.zeros((5, 3, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape.*at most 8"):
        m.overlap_boxes(raw, Bx, torch.zeros((4, 9, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.overlap_boxes(raw, Bx, Hh, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.overlap_boxes(raw, Bx, Hh, Cn, torch.zeros((4, 2, 8)))      # (the features' k is the records')
    with pytest.raises(ValueError, match="shape"):
        m.count_overlaps(raw, torch.zeros(32))
    with pytest.raises(ValueError, match="shape"):
        m.count_overlaps(raw, Bx, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="d_counts"):
        m.overlap_boxes(raw, Bx, None)
    with pytest.raises(ValueError, match="d_counts"):
        m.overlap_boxes(raw, Bx, torch.zeros((4, 0, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="any_overlap"):
        m.overlap_boxes(raw, Bx, Hh, Cn, any_overlap=True)
    with pytest.raises(ValueError, match="contiguous"):
        m.overlap_boxes(raw, torch.zeros((4, 16))[:, ::2], Hh)
    with pytest.raises(ValueError, match="contiguous"):
        m.overlap_boxes(raw, Bx, Hh, torch.zeros(8, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.overlap_boxes(raw, Bx, Hh, Cn, F)
    with pytest.raises(ValueError, match="cuda"):
        m.count_overlaps(raw, Bx, any_overlap=True)
    # pack_boxes makes the rows; voxel_rows a grid's, x fastest, neighbours sharing a face's one bit pattern
    lo, hi = torch.tensor([[0.0, 1, 2], [3, 4, 5]]), torch.tensor([[1.0, 2, 3], [4, 5, 6]])
    rows = m.pack_boxes(lo, hi)
    assert rows.shape == (2, 8) and torch.equal(rows[:, 0:3], lo) and torch.equal(rows[:, 4:7], hi) and bool(torch.all(rows[:, 3] == 0))
    assert torch.equal(m.pack_boxes([0.0, 0, 0], hi)[:, 0:3], torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="shape"):
        m.pack_boxes(torch.zeros((3, 3)), hi)
    v = m.voxel_rows((0.1, -1.0, 0.3), (0.7, 1.0, 2.9), (3, 2, 5)).numpy()
    assert v.shape == (30, 8) and np.all(v[:, 3] == 0) and np.all(v[:, 7] == 0)
    g = v.reshape(5, 2, 3, 8)
    assert np.array_equal(g[:, :, 1:, 0].view(u32), g[:, :, :-1, 4].view(u32))      # x: a voxel's lo is its neighbour's hi, bit for bit
    assert np.array_equal(g[:, 1:, :, 1].view(u32), g[:, :-1, :, 5].view(u32)) and np.array_equal(g[1:, :, :, 2].view(u32), g[:-1, :, :, 6].view(u32))
    assert np.all(g[..., 0] < g[..., 4]) and np.all(g[..., 1] < g[..., 5]) and np.all(g[..., 2] < g[..., 6])
    assert g[0, 0, 0, 0] == f32(0.1) and g[0, 0, 2, 4] == f32(0.7) and g[4, 1, 2, 6] == f32(2.9) and g[0, 0, 1, 0] != g[0, 0, 0, 0]      # x fastest
    with pytest.raises(ValueError, match="shape"):
        m.voxel_rows((0, 0, 0), (1, 1, 1), (4, 4))
    with pytest.raises(ValueError, match="lo <= hi"):
        m.voxel_rows((0, 0, 2), (1, 1, 1), (4, 4, 4))


# ---- code generation ----------------------------------------------------------------------------------------------------------------
# (capacity, any): (VGPRs, waves per SIMD) the compiler reported
PINNED = {(0, False): (80, 6), (0, True): (80, 6), (1, False): (94, 5), (4, False): (104, 4), (8, False): (113, 4)}


def test_overlap_kernel_codegen_has_no_vgpr_spill_and_keeps_the_list_in_registers():
    """overlap.hip compiled for gfx950, from the compiler's report: five instances -- count, any, capacity 1, 4, 8 --, none with a
    VGPR spill or an AGPR, each with the 20-entry LDS stack per lane of a 256-thread block, the private segment of
    trace_rays_kernel (the stack's spill array and nothing else: a list indexed at run time, or a spilled register, would add to it)
    and exactly one scratch store, the push of a stack entry beyond the LDS part.  Registers and waves per SIMD as pinned above."""
    res, asm = _resource_usage("overlap.hip")
    by = {(int(mm.group(1)), mm.group(2) == "1"): k for k in res for mm in [re.search(r"overlap_kernelILi(\d+)ELb([01])E", k)]}
    assert sorted(by) == sorted(PINNED) and len(res) == 5, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    for inst, name in by.items():
        r = res[name]
        print(inst, r)
        assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, (inst, r)
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, (inst, r)
        assert {r["ScratchSize [bytes/lane]"]} == private, (inst, r)
        assert r["VGPRs"] <= PINNED[inst][0] and r["Occupancy [waves/SIMD]"] >= PINNED[inst][1], (inst, r)
        body = _kernel_body(asm, name)
        assert len([t for t in body if t.startswith("scratch_store")]) == 1, inst


# ---- the inputs (the GPU tests use the same) -----------------------------------------------------------------------------------------
def _arrays(text):
    return pyscene.parse_lines(text.split("\n")).arrays()


def pack(lo, hi):
    rows = np.zeros((len(lo), 8), f32)
    rows[:, 0:3] = lo
    rows[:, 4:7] = hi
    return rows


def boxes_about(arrays, n, seed, pad=0.5, hmin=0.02, hmax=0.7):
    """n boxes: centres uniform in the scene's box grown by `pad`, half extents log-uniform in hmin..hmax per axis; every eighth box
    has no extent on one axis, every sixteenth on two, every thirty-second is a point."""
    c = _points_about(arrays, n, seed, pad).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    h = np.exp(rng.uniform(np.log(hmin), np.log(hmax), (n, 3)))
    i = np.arange(n)
    h[i % 8 == 7, 0] = 0
    h[i % 16 == 15, 1] = 0
    h[i % 32 == 31, 2] = 0
    lo, hi = (c - h).astype(f32), (c + h).astype(f32)
    return pack(lo, np.maximum(lo, hi))


def shuffled(rows, seed=1):
    return np.ascontiguousarray(rows[np.random.default_rng(seed).permutation(len(rows))])


DEAD = [((1, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, -1, 1)), ((0, 0, 2), (1, 1, 1)), ((NAN, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, NAN, 1)),
        ((-INF, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, INF)), ((-INF, -INF, -INF), (INF, INF, INF))]


def dead_rows():
    """Rows that are not live: lo > hi on an axis, a NaN, an infinity."""
    return pack(np.array([d[0] for d in DEAD], f32), np.array([d[1] for d in DEAD], f32))


@functools.lru_cache(maxsize=None)
def dense_case():
    """(text, rows): the dense scene (300 spheres, 200 triangles, 2 planes) and 2000 shuffled rows: 1500 boxes with half extents
    0.02 to 0.7, 492 larger ones (0.5 to 1.5: more than eight surfaces), the dead rows."""
    text = dense_scene_text()
    arrays = _arrays(text)
    rows = np.concatenate([boxes_about(arrays, 1500, 51), boxes_about(arrays, 492, 52, hmin=0.5, hmax=1.5), dead_rows()])
    rows[::7, 3], rows[::5, 7] = 123.0, NAN       # (the pad words are ignored)
    assert rows.shape == (2000, 8)
    return text, shuffled(rows.astype(f32))


def touching_rows(arrays, seed):
    """Per sphere four boxes that span the centre on two axes and on the third have a face exactly on a plane of the sphere's
    float32 box (c -+ r, rounded), outside it -- the box touches the sphere to rounding, and its leaf's box exactly -- or one
    float32 step beyond that plane: clear of the leaf's box, and still touching wherever the sphere's own test rounds that way."""
    S = arrays["spheres"]
    rng = np.random.default_rng(seed)
    n = len(S)
    c, r = S["c"].astype(f32), S["r"].astype(f32)
    axis = rng.integers(0, 3, n)
    lo = (c - f32(0.25) * r[:, None]).astype(f32)
    hi = (c + f32(0.25) * r[:, None]).astype(f32)
    out = []
    i = np.arange(n)
    for side in (-1, 1):
        for beyond in (False, True):
            l, h = lo.copy(), hi.copy()
            if side > 0:
                face = (c[i, axis] + r).astype(f32)
                face = np.nextafter(face, f32(np.inf)) if beyond else face
                l[i, axis], h[i, axis] = face, (face + r).astype(f32)
            else:
                face = (c[i, axis] - r).astype(f32)
                face = np.nextafter(face, f32(-np.inf)) if beyond else face
                l[i, axis], h[i, axis] = (face - r).astype(f32), face
            out.append(pack(l, h))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def far_case(offset):
    """(text, rows): far_from_origin, 400 boxes about it and the 1200 touching rows of its spheres."""
    text = edge_scenes.far_from_origin(offset=offset)
    arrays = _arrays(text)
    rows = np.concatenate([boxes_about(arrays, 400, 31, hmin=0.01, hmax=0.3), touching_rows(arrays, 32)])
    return text, shuffled(rows.astype(f32))


@functools.lru_cache(maxsize=None)
def deep_case():
    """(text, rows): deep_stack(600) and 250 boxes, inside the nest and across it."""
    text = edge_scenes.deep_stack(600)
    return text, boxes_about(_arrays(text), 250, 44, pad=0.5, hmin=0.05, hmax=1.5)


CHOSEN = """png 8 8 chosen.png
sphere 0 0 -4 1
sphere 8 0 0 0.5
xyz 0 0 3
xyz 1 0 3
xyz 0 1 3
tri 1 2 3
tri 1 2 3
xyz 4 0 0
xyz 6 0 0
tri 4 5 5
xyz 4 4 0
xyz 6 4 0
tri 6 6 7
plane 0 0 1 16
"""
# (lo, hi, the count): every coordinate is dyadic, so every operation of the tests is exact
CHOSEN_ROWS = [
    ((-1, -1, 2.5), (0, 0, 3.5), 2),             # 0: the box's edge x = 0, y = 0 on the twins' vertex a
    ((-1, 0.25, 2.5), (0, 0.75, 3.5), 2),        # 1: the face x = 0 on their edge a-c
    ((0.25, 0.25, 3), (0.5, 0.5, 4), 2),         # 2: the face z = 3 in their plane
    ((-0.25, -0.25, -3), (0.25, 0.25, -2), 1),   # 3: the face z = -3 on sphere 0's pole
    ((-1, -1, -17), (1, 1, -16), 1),             # 4: the face z = -16 on the plane
    ((-1, -1, -16), (1, 1, -15), 1),             # 5: ... from the other side
    ((-0.25, -0.25, -4.25), (0.25, 0.25, -3.75), 0),      # 6: strictly inside sphere 0: not counted
    ((7, -1, -1), (9, 1, 1), 1),                 # 7: holds sphere 1: counted
    ((-1, -1, 2), (2, 2, 4), 2),                 # 8: encloses the twins whole
    ((0.25, 0.25, 3), (0.25, 0.25, 3), 2),       # 9: a point on the twins
    ((0, 0, -3), (0, 0, -3), 1),                 # 10: a point on sphere 0's pole
    ((0, 0, -16), (0, 0, -16), 1),               # 11: a point on the plane
    ((4.5, -0.5, -0.5), (5.5, 0.5, 0.5), 1),     # 12: the triangle without area (b == c) met as the segment (4, 0, 0)-(6, 0, 0)
    ((6, -0.5, -0.5), (7, 0.5, 0.5), 1),         # 13: ... touched at its end
    ((6.125, -0.5, -0.5), (7, 0.5, 0.5), 0),     # 14: ... and missed
    ((4.5, 3.5, -0.5), (5.5, 4.5, 0.5), 0),      # 15: a == b: every axis passes, dist at m is 0 / 0, not admitted
    ((3.5, 3.5, -0.5), (4.5, 4.5, 0.5), 1),      # 16: ... where the vertex region answers, dist is a number: admitted
    ((-9, -9, -20), (9, 9, 9), 7),               # 17: everything, the a == b triangle too: from this centre its vertex region answers
    ((2, 2, 2), (2.5, 2.5, 2.5), 0),             # 18: nothing
]


@functools.lru_cache(maxsize=None)
def chosen_case():
    lo = np.array([r[0] for r in CHOSEN_ROWS], f32)
    hi = np.array([r[1] for r in CHOSEN_ROWS], f32)
    return CHOSEN, np.concatenate([pack(lo, hi), dead_rows()])


VOXEL_SCENE = """png 8 8 voxels.png
sphere 0.3 -0.4 -0.9 0.7
xyz -1.25 -0.75 0.5
xyz 1 -0.5 0.5
xyz -0.25 1.25 0.5
tri 1 2 3
xyz -1.6 0.1 -1.7
xyz -0.2 1.3 -0.4
xyz -1.1 1.7 1.2
tri 4 5 6
plane 0 1 0 1.5
"""
VOXEL_BOX = ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (16, 16, 16))      # voxels of 0.25: the first triangle (z = 0.5) and the plane (y = -1.5) lie on voxel faces


@functools.lru_cache(maxsize=None)
def voxel_case():
    return VOXEL_SCENE, m.voxel_rows(*VOXEL_BOX).numpy()


@functools.lru_cache(maxsize=None)
def mixed_case():
    """(text, rows): the scene and the 4096 rows of the row-count test."""
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    return text, boxes_about(_arrays(text), 4096, 45, pad=1.0, hmin=0.02, hmax=1.0)


def small_case(name):
    text = edge_scenes.ALL[name]()
    c = np.random.default_rng(5).uniform(-3, 3, (100, 3))
    c[:, 2] -= 2
    h = np.exp(np.random.default_rng(6).uniform(np.log(0.05), np.log(1.5), (100, 3)))
    return text, pack((c - h).astype(f32), (c + h).astype(f32))


MOVED = ("sphere 0.9 -0.2 -2.6 0.6", "sphere 0.3 0.4 -2.4 0.7")


@functools.lru_cache(maxsize=None)
def moved_case():
    """(text after the update, rows): the scene of the update test with its second sphere moved."""
    text = light_scenes.scene("spheres_planes", 3, "mixed")
    moved = text.replace(*MOVED)
    assert moved != text
    return moved, boxes_about(_arrays(moved), 600, 48, pad=1.0, hmin=0.05, hmax=1.0)


CASES = {"dense": dense_case, "far_1e3": lambda: far_case(1000.0), "far_1e5": lambda: far_case(100000.0), "deep_stack": deep_case,
         "chosen": chosen_case, "voxels": voxel_case, "mixed": mixed_case, "moved": moved_case,
         **{name: functools.partial(small_case, name) for name in ("single_sphere", "single_triangle", "empty", "plane_only")}}


@functools.lru_cache(maxsize=None)
def case_keys(name):
    """(arrays, rows, the key of every candidate for every row): computed once per case."""
    text, rows = CASES[name]()
    arrays = _arrays(text)
    return arrays, rows, ovr.keys(arrays, rows)[0]


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """(hits, counts, features) of a case by the brute force: what the GPU tests compare against."""
    arrays, rows, key = case_keys(name)
    return ovr.brute_force(arrays, rows, k, key=key)


# ---- the restatement against float64 by other methods ------------------------------------------------------------------------------
def _clip_leaves_something(tri, lo, hi):
    """Sutherland-Hodgman in float64: the triangle clipped against the box's six closed half spaces; is anything left?"""
    poly = [tri[0], tri[1], tri[2]]
    for axis in range(3):
        for sign, bound in ((1.0, hi[axis]), (-1.0, -lo[axis])):
            out = []
            for j in range(len(poly)):
                p, q = poly[j - 1], poly[j]
                dp, dq = sign * p[axis] - bound, sign * q[axis] - bound
                if dq <= 0:
                    if dp > 0:
                        out.append(p + (q - p) * (dp / (dp - dq)))
                    out.append(q)
                elif dp <= 0:
                    out.append(p + (q - p) * (dp / (dp - dq)))
            poly = out
            if not poly:
                return False
    return True


def _nearest_axis_margin(mm, hh, a, b, c):
    """The least |gap| over the thirteen axes in float64, each axis normalised (a gap is how far the triangle's interval ends from
    the box's, a length): how near the pair is to the bound of some axis."""
    v = [a - mm, b - mm, c - mm]
    f = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    axes = [np.eye(3)[k] for k in range(3)] + [np.cross(f[0], f[1])] + [np.cross(np.eye(3)[k], e) for e in f for k in range(3)]
    least = np.inf
    for ax in axes:
        ln = np.linalg.norm(ax)
        if ln < 1e-12:
            continue
        ax = ax / ln
        p = [x @ ax for x in v]
        r = hh @ np.abs(ax)
        least = min(least, abs(min(p) - r), abs(max(p) + r))
    return least


def test_restatement_agrees_with_float64_by_other_methods():
    """300 boxes (half extents 0.02 to 0.7; the scene's scale is 1, its triangles' shortest edge) against the 40 spheres, 40
    well-shaped triangles and 2 planes of section 6o's scene: 24 600 candidate/row pairs.  In float64, a triangle by clipping it
    against the box's six half spaces, a sphere by the closed-form nearest and farthest points of the box, a plane by the signed
    distances of the eight corners.  A pair is set aside when an axis passes or fails by less than 1e-5 (|m| + |h| + |p|); at most
    1 % may be.  On the kept pairs the admitted sets are equal."""
    arrays = _arrays(_well_shaped_scene())
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    rng = np.random.default_rng(61)
    n = 300
    c = rng.uniform(-2.5, 2.5, (n, 3))
    h = np.exp(rng.uniform(np.log(0.02), np.log(0.7), (n, 3)))
    rows = pack((c - h).astype(f32), (c + h).astype(f32))
    key, kinds, ids = ovr.keys(arrays, rows)
    got = key != u64(ovr.KEY_NONE)
    assert got.shape == (n, 82) and got.size >= 20000
    lo, hi = rows[:, 0:3].astype(np.float64), rows[:, 4:7].astype(np.float64)
    mm, hh = (lo + hi) / 2, (hi - lo) / 2
    want = np.zeros_like(got)
    near = np.zeros_like(got)
    REL = 1e-5
    for j in range(len(S)):
        cc, r = S["c"][j].astype(np.float64), float(S["r"][j])
        dmin = np.linalg.norm(np.maximum(np.maximum(lo - cc, cc - hi), 0), axis=1)
        dmax = np.linalg.norm(np.maximum(np.abs(cc - lo), np.abs(hi - cc)), axis=1)
        want[:, j] = (dmin <= r) & (r <= dmax)
        scale = np.abs(mm).max(axis=1) + np.abs(hh).max(axis=1) + np.abs(cc).max() + r
        near[:, j] = (np.abs(dmin - r) < REL * scale) | (np.abs(dmax - r) < REL * scale)
    corners = np.array([[(i >> a) & 1 for a in range(3)] for i in range(8)], np.float64)
    for j in range(len(Pl)):
        col = len(S) + len(T) + j
        nor, point = Pl["nor"][j].astype(np.float64), Pl["point"][j].astype(np.float64)
        N = nor / np.linalg.norm(nor)
        sd = ((lo[:, None, :] + corners[None] * (hi - lo)[:, None, :]) - point) @ N      # [n, 8]
        want[:, col] = (sd.min(axis=1) <= 0) & (sd.max(axis=1) >= 0)
        scale = np.abs(mm).max(axis=1) + np.abs(hh).max(axis=1) + np.abs(point).max()
        near[:, col] = (np.abs(sd.min(axis=1)) < REL * scale) | (np.abs(sd.max(axis=1)) < REL * scale)
    for j in range(len(T)):
        col = len(S) + j
        tri = [T[k][j].astype(np.float64) for k in ("p0", "p1", "p2")]
        pmax = max(np.abs(p).max() for p in tri)
        for i in range(n):
            want[i, col] = _clip_leaves_something(tri, lo[i], hi[i])
            near[i, col] = _nearest_axis_margin(mm[i], hh[i], *tri) < REL * (np.abs(mm[i]).max() + np.abs(hh[i]).max() + pmax)
    kept = ~near
    print(f"pairs {got.size}, set aside {near.sum()} ({near.mean():.5f}), admitted {want.mean():.4f}: spheres {want[:, :40].mean():.4f}, "
          f"triangles {want[:, 40:80].mean():.4f}, planes {want[:, 80:].mean():.4f}; differing among all pairs {(got != want).sum()}")
    assert near.mean() <= 0.01
    assert np.array_equal(got[kept], want[kept])
    for sel in (slice(0, 40), slice(40, 80), slice(80, 82)):
        assert want[:, sel].sum() > 20 and (~want[:, sel]).sum() > 20      # every kind is admitted and refused


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pruned_walk_in_either_child_order_equals_the_brute_force_bit_for_bit(name):
    arrays, rows, key = case_keys(name)
    text, _ = CASES[name]()
    _, nodes, refs = _oracle_tree(text)
    k = 8
    want_hits, want_counts, want_feat = reference(name, k)
    for left_first in (True, False):
        hits, counts, feat, visited = ovr.pruned_walk(arrays, rows, nodes, refs, k, left_first=left_first, key=key)
        assert np.array_equal(hits, want_hits) and np.array_equal(feat.view(u32), want_feat.view(u32)), left_first
        assert np.array_equal(counts, want_counts), left_first
        _, some, _, seen = ovr.pruned_walk(arrays, rows, nodes, refs, 0, left_first=left_first, any_overlap=True, key=key)
        assert np.array_equal(some, (want_counts > 0).astype(u32)), left_first
        assert np.all(seen <= visited)
        print(f"{name}: left first {left_first}: {visited.mean():.1f} of {len(refs)} leaves visited per row; any: {seen.mean():.1f}")
    if len(refs) > 100 and name != "deep_stack":
        assert visited.mean() < 0.5 * len(refs)      # (it does prune)


@pytest.mark.parametrize("name", ["far_1e3", "far_1e5"])
def test_the_walk_without_the_slack_on_the_far_and_touching_rows(name):
    """The negative control: sigma = 0 away from the origin.  Rows whose face lies exactly on a plane of a sphere's float32 box are
    visited without a slack (the compare is negated); of the rows one float32 step beyond that plane some still pass the sphere's
    own test -- lo - c rounds to r, the squares agree -- and those the walk without the slack loses: 17 of 1600 rows at 1e3 and 17
    at 1e5.  With the header's sigma the walk equals the brute force."""
    arrays, rows, key = case_keys(name)
    text, _ = CASES[name]()
    _, nodes, refs = _oracle_tree(text)
    want_hits, want_counts, _ = reference(name, 8)
    hits, counts, _, _ = ovr.pruned_walk(arrays, rows, nodes, refs, 8, key=key)
    assert np.array_equal(hits, want_hits) and np.array_equal(counts, want_counts)
    hits0, counts0, _, _ = ovr.pruned_walk(arrays, rows, nodes, refs, 8, slack=0.0, key=key)
    lost = (counts0 != want_counts) | np.any(hits0.reshape(len(rows), -1) != want_hits.reshape(len(rows), -1), axis=1)
    touching = want_counts > 0
    print(f"{name}: {int(lost.sum())} of {len(rows)} rows differ without the slack ({int(touching.sum())} rows touch something)")
    assert np.all(counts0 <= want_counts) and lost.sum() >= 1      # (a walk can only lose candidates)


@pytest.mark.parametrize("name", ["dense", "deep_stack", "mixed", "far_1e3"])
def test_counts_are_bracketed_by_the_contact_query(name):
    """For every live row with min(h) > 0: the ball of radius 0.999 min(h) about m lies in the box, the ball of radius 1.001 |h|
    holds it, so count_within of the first <= the overlap count <= count_within of the second."""
    arrays, rows, _ = case_keys(name)
    _, counts, _ = reference(name, 0)
    _, _, mm, hh = ovr.box_quantities(rows)
    sel = ovr.live_rows(rows) & (hh.min(axis=1) > 0)
    assert sel.sum() > 0.7 * len(rows)
    inner = np.concatenate([mm, (f32(0.999) * hh.min(axis=1))[:, None]], axis=1).astype(f32)[sel]
    outer = np.concatenate([mm, (f32(1.001) * cr._length(hh))[:, None]], axis=1).astype(f32)[sel]
    _, cin, _ = kr.brute_force(arrays, inner, 0)
    _, cout, _ = kr.brute_force(arrays, outer, 0)
    print(f"{name}: inner {cin.mean():.2f} <= overlap {counts[sel].mean():.2f} <= outer {cout.mean():.2f}; strictly between on "
          f"{np.mean((cin < counts[sel]) | (counts[sel] < cout)):.3f} of the rows")
    assert np.all(cin <= counts[sel]) and np.all(counts[sel] <= cout)
    assert np.any(cin < counts[sel]) and np.any(counts[sel] < cout)


@pytest.mark.parametrize("name", ["dense", "deep_stack", "chosen", "far_1e5"])
def test_records_counts_and_order(name):
    arrays, rows, _ = case_keys(name)
    h8, c8, f8 = reference(name, 8)
    h4, c4, f4 = reference(name, 4)
    h1, c1, f1 = reference(name, 1)
    h0, c0, f0 = reference(name, 0)
    n = len(rows)
    assert h8.shape == (n, 8, 6) and f8.shape == (n, 8, 8) and h0.shape == (n, 0, 6)
    assert np.array_equal(h4, h8[:, :4]) and np.array_equal(f4.view(u32), f8[:, :4].view(u32)) and np.array_equal(h1, h8[:, :1])
    assert np.array_equal(c4, c8) and np.array_equal(c1, c8) and np.array_equal(c0, c8)            # the counts do not depend on k
    past = np.arange(8)[None, :] >= c8[:, None]
    assert np.all(h8[past] == ovr.MISS) and np.all(f8[past] == 0) and np.all(h8[~past][:, 1] != 0) and np.all(f8[~past][:, 3] == 1)
    t = h8[:, :, 0].view(f32)
    both = ~past[:, 1:]
    assert np.all((t[:, 1:] >= t[:, :-1])[both]) and np.all(t[~past] >= 0)                           # t is non-decreasing along a row
    tie = (t[:, 1:] == t[:, :-1]) & both
    order = h8[:, :, 1].astype(np.int64) * (1 << 32) + h8[:, :, 2]
    assert np.all((order[:, 1:] > order[:, :-1])[tie])                                             # ties are in (kind, id) order
    dead = ~ovr.live_rows(rows)
    assert np.all(c8[dead] == 0) and np.all(h8[dead] == ovr.MISS)
    # every record is mirt_closest_points' record of that candidate at the box's centre: the nearest record is its answer whenever
    # the nearest surface of all touches the box
    near_hits, near_feat = cr.brute_force(arrays, ovr.centre_rows(rows))
    same = (c8 > 0) & (h8[:, 0, 0] == near_hits[:, 0])
    assert np.array_equal(h8[same, 0], near_hits[same]) and np.array_equal(f8[same, 0].view(u32), near_feat[same].view(u32))
    assert same.sum() > 0


def test_the_dense_rows_fill_truncate_and_empty_the_list():
    _, c, _ = reference("dense", 0)
    print(f"dense: more than 8: {np.mean(c > 8):.3f}, 1 to 8: {np.mean((c >= 1) & (c <= 8)):.3f}, none: {np.mean(c == 0):.3f}, max {c.max()}")
    assert np.mean(c > 8) > 0.10 and np.mean((c >= 1) & (c <= 8)) > 0.30 and np.mean(c == 0) > 0.01
    h8, _, _ = reference("dense", 8)
    assert set(h8[:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}


def test_the_chosen_rows_have_the_counts_the_header_gives_them():
    arrays, rows, _ = case_keys("chosen")
    h8, c8, f8 = reference("chosen", 8)
    n = len(CHOSEN_ROWS)
    assert c8[:n].tolist() == [r[2] for r in CHOSEN_ROWS] and np.all(c8[n:] == 0)
    # two identical primitives both appear, the lower id first, with the same record but for the id
    for r in (0, 1, 2, 8, 9):
        assert [tuple(x) for x in h8[r, :2, 1:3].tolist()] == [(2, 0), (2, 1)] and np.array_equal(h8[r, 0, 3:6], h8[r, 1, 3:6]) and h8[r, 0, 0] == h8[r, 1, 0]
    assert tuple(h8[3, 0, 1:3].tolist()) == (1, 0) and tuple(h8[7, 0, 1:3].tolist()) == (1, 1) and tuple(h8[4, 0, 1:3].tolist()) == (3, 0)
    assert tuple(h8[12, 0, 1:3].tolist()) == (2, 2) and h8[12, 0, 0].view(f32) == 0 and tuple(h8[16, 0, 1:3].tolist()) == (2, 3)
    assert sorted(tuple(x) for x in h8[17, :7, 1:3].tolist()) == [(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0)]
    # P is the surface point nearest the centre: for the box that touches the twins at a vertex it is that vertex, on the box; for
    # the box on sphere 0's pole it is the pole, and the normal points at the centre
    assert np.array_equal(f8[0, 0, 0:4], np.array([0, 0, 3, 1], f32)) and np.array_equal(f8[9, 0, 0:3], rows[9, 0:3])
    assert np.array_equal(f8[3, 0, 0:3], np.array([0, 0, -3], f32)) and np.array_equal(f8[3, 0, 4:7], np.array([0, 0, 1], f32))


def test_a_surface_on_a_shared_voxel_face_marks_both_neighbours():
    arrays, rows, _ = case_keys("voxels")
    _, c, _ = reference("voxels", 0)
    grid = (c > 0).reshape(16, 16, 16)      # [z, y, x]
    # the triangle in z = 0.5, the face between layers 9 and 10: at its centroid's column both are marked, the layers beyond are not
    x, y = int((-0.1667 + 2) / 0.25), int((0.0 + 2) / 0.25)
    assert grid[9, y, x] and grid[10, y, x]
    # the plane y = -1.5, the face between rows 1 and 2: both rows are marked everywhere, row 0 nowhere a primitive reaches it
    assert np.all(grid[:, 1, :]) and np.all(grid[:, 2, :]) and not np.any(grid[:, 0, :])
    assert 0.05 < grid.mean() < 0.5

"""Every record the traversal kernels read from a built scene (mirt_get_records), recomputed in numpy from the tree in the
reference's numbering (mirt_get_tree), the scene's own arrays and the layout facts of csrc/scene_dev.h -- never from another
device result of the same kind.

  tree          every node but the root has one parent, every leaf is reached from node 0, every primitive sits in one leaf, a
                node's box is the fminf / fmaxf union of its children's, a leaf's box is its primitive's, tree_depth is the
                longest path in internal nodes
  exact records the twelve floats are the two children's boxes, the references name them, NODE_SWAP_PURE is set where both
                subtrees hold spheres only, NODE_SWAP_ANY always
  32-byte       the six words bound each child's box from outside by less than three grid steps (exact arithmetic, the form of
                qbox_ref.check_words) and equal the float32 restatement; words 6, 7 are the references; REF_QPURE in word 6 only
  wide          the grandchildren in the reference's visiting order, a leaf child standing for itself; absent slots inverted
  primitives    sorted order at unit j + 2 tris_before[j], the scene's own bits, unit_prim on every unit, tri_boxes
  scalars       qparams, grid_ok, coord_max, the root references, bounds_as_shipped offering no quantised records
"""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
import edge_scenes
import qbox_ref as Q

pytestmark = pytest.mark.gpu

F = np.float32
REF_LEAF, REF_TRI, REF_QPURE, REF_NONE, QBOX_NONE = 0x80000000, 0x40000000, 0x20000000, 0xf0000000, 0x0000ffff
NODE_SWAP_PURE, NODE_SWAP_ANY = 1, 2
SCENES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes")
LIT = edge_scenes.HEADER + "color 1 1 1\nsun 1 1 1\n"
TRI = "xyz -1 -1 -2\nxyz 1 -1 -2.5\nxyz 0 1 -2\ntri -3 -2 -1\n"      # (a negative index counts back from the last vertex)
FLAT_TRI = "xyz -1 0.25 -3\nxyz 1 0.25 -3\nxyz 0 0.25 -4\ntri -3 -2 -1\n"      # thin in y: its leaf box is padded by 0.01

TEXTS = {
    "identical64": LIT + "sphere 0.5 0.25 -3 0.5\n" * 64,                       # every Morton code equal: the index tie-break orders the leaves
    "n2_spheres": LIT + "sphere -1 0 -3 0.5\nsphere 1 0.5 -4 0.75\n",
    "n3_spheres": LIT + "sphere -1 0 -3 0.5\nsphere 1 0.5 -4 0.75\nsphere 0 2 -3.5 0.25\n",
    "n2_mixed": LIT + "sphere -1 0 -3 0.5\n" + TRI,
    "n3_mixed": LIT + TRI + "sphere -1 0 -3 0.5\n" + FLAT_TRI,
    "n1_sphere": edge_scenes.single_sphere(),
    "n1_triangle": edge_scenes.single_triangle(),
    "empty": edge_scenes.empty(),
    "far_from_origin": edge_scenes.far_from_origin(),
}

# (spheres, triangles): mixed primitives, duplicate Morton codes.  A block is 256 threads and the sort and placement-scan tiles are
# 2048 items: 257, 2048 and 2049 primitives are the smallest scenes with a second block, a full tile, and a second workgroup whose
# offsets and carry come from the first while its own tile is partly filled.
SYNTHETIC = {"synthetic": (1500, 1500), "synthetic_257": (128, 129), "synthetic_2048": (1024, 1024), "synthetic_2049": (1024, 1025)}


def load(name):
    if name in ("tri", "redchair", "spiral"):
        return m.parseInput(os.path.join(SCENES, name + ".txt"))
    if name in SYNTHETIC:
        return m.syntheticScene(*SYNTHETIC[name])
    return m.parseText(TEXTS[name])


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def prim_boxes(refs, spheres, tris):
    """[n, 6] (xmin, xmax, ymin, ymax, zmin, zmax): the leaf box of every primitive reference, float32 operation for operation."""
    out = np.zeros((len(refs), 6), F)
    for i, (t, k) in enumerate(zip(refs["type"], refs["id"])):
        if t == 0:
            c, r = spheres["c"][k].astype(F), F(spheres["r"][k])
            a, b = c - r, c + r
            lo, hi = np.where(a <= b, a, b), np.where(a <= b, b, a)
        else:
            p = np.stack([tris["p0"][k], tris["p1"][k], tris["p2"][k]]).astype(F)
            lo, hi = np.fmin(np.fmin(p[0], p[1]), p[2]), np.fmax(np.fmax(p[0], p[1]), p[2])
            thin = (hi - lo) < F(0.01)
            lo, hi = np.where(thin, lo - F(0.01), lo), np.where(thin, hi + F(0.01), hi)
        out[i, 0::2], out[i, 1::2] = lo, hi
    return out


def words_bound(x, smin, step, q, upper):
    """qbox_ref.check_words on arrays: float64 decides what it can decide, Fractions the rest."""
    u = (x.astype(np.float64) - smin.astype(np.float64)) / step.astype(np.float64)
    q = q.astype(np.float64)
    if upper:
        top = q == 65535
        slack = np.where(top, 65535 + 1 / 16 - u, np.minimum(q - u, 3 - (q - u)))
    else:
        slack = np.where(q == 0, u - q, np.minimum(u - q, 3 - (u - q)))
    assert np.all(slack > -1e-6), (upper, np.argwhere(slack <= -1e-6)[:5])
    for idx in np.argwhere(slack < 1e-6):
        i = tuple(idx)
        ue = (Fraction(float(x[i])) - Fraction(float(smin[i]))) / Fraction(float(step[i]))
        qi = int(q[i])
        if upper:
            assert (ue - 65535 < Fraction(1, 16)) if qi == 65535 else (qi >= ue and qi - ue < 3), ("q_hi", i, qi, float(ue))
        else:
            assert qi <= ue and (qi == 0 or ue - qi < 3), ("q_lo", i, qi, float(ue))


def check_box_words(words, boxes, smin, smax, grid_ok):
    """words [n, 3] against boxes [n, 6]: the restatement's bits always; the bounds in exact arithmetic where the grid resolves
    the scene."""
    step, _ = Q.grid_of(smin, smax)
    lo, hi = boxes[:, 0::2], boxes[:, 1::2]
    s, st = np.broadcast_to(smin, lo.shape), np.broadcast_to(step, lo.shape)
    assert np.array_equal(words & 0xffff, Q.q_lo(lo, s, st)) and np.array_equal(words >> 16, Q.q_hi(hi, s, st))
    if grid_ok:
        words_bound(lo, s, st, words & 0xffff, False)
        words_bound(hi, s, st, words >> 16, True)


def check_scene(stl, raw, spheres=None, shipped=False):
    spheres = stl.array("spheres") if spheres is None else spheres
    tris = stl.array("triangles")
    n, ns, nt = stl.num_prims, stl.num_spheres, stl.num_triangles
    tree, codes, refs, bounds = raw.tree()
    rec = raw.records()
    info = rec["info"]
    assert (info.num_nodes, info.prim_units, info.num_tri_boxes) == (max(n - 1, 0), ns + 3 * nt, nt)
    assert info.num_tris_before == (n + 1 if n else 0) and info.prim_base16 == 4 * max(n - 1, 0)
    assert [len(rec[k]) for k in ("nodes", "qnodes", "wnodes", "prims", "unit_prim", "tris_before", "tri_boxes", "qparams")] == \
        [info.num_nodes, info.num_qnodes, info.num_wnodes, info.prim_units, info.prim_units, info.num_tris_before, info.num_tri_boxes, info.num_qparams]
    if n == 0:
        assert info.root_ref == info.root_ref_q == info.root_ref_w == REF_NONE and info.num_qparams == 0 and info.tree_depth == 0
        return info

    # ---- the sorted leaves: every primitive once, in code order, where the primitive records go ----
    assert sorted(map(tuple, refs.tolist())) == sorted(map(tuple, stl.array("prim_refs").tolist())) and len(set(map(tuple, refs.tolist()))) == n
    assert np.all(codes[:-1] <= codes[1:])
    is_tri = refs["type"] != 0
    tb = np.concatenate([[0], np.cumsum(is_tri)]).astype(np.uint32)
    assert np.array_equal(rec["tris_before"], tb) and tb[n] == nt
    unit = np.arange(n, dtype=np.uint32) + 2 * tb[:n]
    leaf_ref = (REF_LEAF | np.where(is_tri, REF_TRI, 0) | (info.prim_base16 + unit)).astype(np.uint32)
    box = np.stack([tree[k] for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")], axis=1)
    assert np.array_equal(bits(box[n - 1:]), bits(prim_boxes(refs, spheres, tris)))
    leaves = tree[n - 1:]
    assert np.array_equal(leaves["prim_offset"], np.arange(n)) and np.all(leaves["count"] == 1)

    # ---- the primitive region ----
    want = np.zeros((ns + 3 * nt, 4), F)
    want_up = np.zeros(ns + 3 * nt, np.uint32)
    covered = np.zeros(ns + 3 * nt, np.int32)
    for j in range(n):
        k, u = refs["id"][j], unit[j]
        if is_tri[j]:
            t = tris[k]
            want[u:u + 3] = np.concatenate([t["p0"], t["nor"], t["e1"], t["e2"]]).reshape(3, 4)
            want_up[u:u + 3] = 0x80000000 | k
            covered[u:u + 3] += 1
        else:
            want[u] = (*spheres["c"][k], spheres["r"][k])
            want_up[u] = k
            covered[u] += 1
    assert np.all(covered == 1)
    assert np.array_equal(bits(rec["prims"]), bits(want)) and np.array_equal(rec["unit_prim"], want_up)
    if nt:
        tri_leaf = np.zeros((nt, 8), F)
        tri_leaf[refs["id"][is_tri], :6] = box[n - 1:][is_tri]
        assert np.array_equal(bits(rec["tri_boxes"]), bits(tri_leaf))

    if n == 1:
        assert info.root_ref == leaf_ref[0] and info.root_ref_q == info.root_ref_w == REF_NONE
        assert (info.grid_ok, info.tree_depth, info.coord_max, info.num_qparams) == (0, 0, 0.0, 0)
        return info

    # ---- the tree ----
    left, right = tree["left"][:n - 1].astype(np.int64), tree["right"][:n - 1].astype(np.int64)
    kids = np.stack([left, right], axis=1)
    assert kids.min() >= 1 and kids.max() <= 2 * n - 2
    parents = np.bincount(kids.ravel(), minlength=2 * n - 1)
    assert parents[0] == 0 and np.all(parents[1:] == 1)
    depth = np.zeros(2 * n - 1, np.int64)      # internal nodes on the path from the root, the node itself included
    order, stack = [], [0]
    depth[0] = 1
    while stack:
        i = stack.pop()
        order.append(i)
        for c in kids[i]:
            depth[c] = depth[i] + (1 if c < n - 1 else 0)
            if c < n - 1:
                stack.append(c)
            else:
                order.append(c)
    assert len(order) == 2 * n - 1 and len(set(order)) == 2 * n - 1      # every leaf is reached from node 0
    assert info.tree_depth == depth[n - 1:].max() == raw.get_option("tree_depth")
    lb, rb = box[left], box[right]
    union = np.where(np.arange(6) % 2 == 0, np.fmin(lb, rb), np.fmax(lb, rb))
    assert np.array_equal(bits(box[:n - 1]), bits(union))
    tri_count = np.zeros(2 * n - 1, np.int64)
    tri_count[n - 1:] = is_tri
    for i in reversed([i for i in order if i < n - 1]):
        tri_count[i] = tri_count[left[i]] + tri_count[right[i]]
    pure = tri_count == 0
    if not shipped:
        assert np.array_equal(bits(bounds), bits(np.concatenate([box[0, 0::2], box[0, 1::2]])))

    def ref_of(node, base16, per_node):
        node = np.asarray(node)
        return np.where(node >= n - 1, leaf_ref[np.maximum(node - (n - 1), 0)], base16 + per_node * node).astype(np.uint32)

    # ---- exact records ----
    nodes = rec["nodes"]
    assert np.array_equal(bits(nodes[:, :6]), bits(lb)) and np.array_equal(bits(nodes[:, 6:12]), bits(rb))
    w = bits(nodes)
    assert np.array_equal(w[:, 12], ref_of(left, 0, 4)) and np.array_equal(w[:, 13], ref_of(right, 0, 4))
    assert np.array_equal(w[:, 14], NODE_SWAP_ANY | np.where(pure[left] & pure[right], NODE_SWAP_PURE, 0)) and not w[:, 15].any()
    assert info.root_ref == 0

    # ---- what the host decided from the root's two child boxes ----
    both = np.concatenate([lb[0], rb[0]])
    assert info.coord_max == np.abs(both).max()
    lo, hi = np.fmin(lb[0, 0::2], rb[0, 0::2]), np.fmax(lb[0, 1::2], rb[0, 1::2])
    assert info.grid_ok == int(np.all(np.fmax(np.abs(lo), np.abs(hi)) <= F(64.0) * (hi - lo)))

    if shipped:      # no quantised records are offered
        assert info.root_ref_q == info.root_ref_w == REF_NONE and (info.num_qnodes, info.num_wnodes, info.num_qparams) == (0, 0, 0)
        return info
    smin, smax = bounds[:3], bounds[3:]
    step, lim = Q.grid_of(smin, smax)
    assert info.num_qparams == 9 and np.array_equal(bits(rec["qparams"]), bits(np.concatenate([smin, step, lim])))

    if nt == 0:      # ---- 32-byte records ----
        q = rec["qnodes"]
        assert info.num_wnodes == 0 and info.root_ref_w == REF_NONE and len(q) == n - 1
        assert info.qnode_base16 * 16 >= 16 * (info.prim_base16 + info.prim_units) and info.root_ref_q == info.qnode_base16
        check_box_words(q[:, 0:3], lb, smin, smax, info.grid_ok)
        check_box_words(q[:, 3:6], rb, smin, smax, info.grid_ok)
        assert np.array_equal(q[:, 6], ref_of(left, info.qnode_base16, 2) | REF_QPURE)      # (a sphere-only scene: every subtree is)
        assert np.array_equal(q[:, 7], ref_of(right, info.qnode_base16, 2)) and not (q[:, 7] & REF_QPURE).any()
    else:            # ---- wide records ----
        wn = rec["wnodes"]
        assert info.num_qnodes == 0 and info.root_ref_q == REF_NONE and len(wn) == n - 1
        assert (info.wnode_base16 * 16) % 128 == 0 and info.wnode_base16 >= info.prim_base16 + info.prim_units and info.root_ref_w == info.wnode_base16
        grand = np.full((n - 1, 4), -1, np.int64)
        for p in range(n - 1):
            g = []
            for c in kids[p]:
                g += [c] if c >= n - 1 else [left[c], right[c]]
            grand[p, :len(g)] = g
        for s in range(4):
            have = grand[:, s] >= 0
            check_box_words(wn[have, 3 * s:3 * s + 3], box[grand[have, s]], smin, smax, info.grid_ok)
            assert np.array_equal(wn[have, 12 + s], ref_of(grand[have, s], info.wnode_base16, 4))
            assert np.all(wn[~have, 3 * s:3 * s + 3] == QBOX_NONE) and np.all(wn[~have, 12 + s] == REF_NONE)
    return info


@pytest.mark.parametrize("name", ["tri", "redchair", "spiral"] + list(SYNTHETIC) + sorted(TEXTS))
def test_every_record_is_what_the_tree_says(name):
    stl = load(name)
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        with pytest.raises(m.MirtError) as e:
            raw.records()
        assert e.value.status == 6      # not built
        m.build_lbvh_karas(raw)
        info = check_scene(stl, raw)
        if name == "far_from_origin":
            assert info.grid_ok == 0 and info.num_qnodes == stl.num_prims - 1
        elif stl.num_prims > 1 and name not in SYNTHETIC:
            assert info.grid_ok == 1
        assert (info.num_qnodes > 0) == (stl.num_triangles == 0 and stl.num_prims > 1)
        assert (info.num_wnodes > 0) == (stl.num_triangles > 0 and stl.num_prims > 1)
    finally:
        raw.close()


@pytest.mark.parametrize("name", ["n3_mixed", "identical64", "tri"])
def test_bounds_as_shipped_offers_no_quantised_records(name):
    stl = load(name)
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        raw.set_option("bounds_as_shipped", 1)
        m.build_lbvh_karas(raw)
        check_scene(stl, raw, shipped=True)
        raw.set_option("bounds_as_shipped", 0)      # and a rebuild offers them again, with nothing of the other tree left
        m.build_lbvh_karas(raw)
        check_scene(stl, raw)
    finally:
        raw.close()


def test_nothing_stale_survives_an_update_and_a_rebuild():
    stl = m.parseText(edge_scenes.far_camera(300))
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        m.build_lbvh_karas(raw)
        check_scene(stl, raw)
        rng = np.random.default_rng(5)
        moved = stl.array("spheres")
        moved["c"] = rng.uniform(-3, 2, (len(moved), 3)).astype(F)
        moved["r"] = rng.uniform(0.02, 0.3, len(moved)).astype(F)
        xyzr = torch.from_numpy(np.concatenate([moved["c"], moved["r"][:, None]], axis=1)).to("cuda:0")
        m.update_spheres(raw, xyzr)
        with pytest.raises(m.MirtError) as e:
            raw.records()
        assert e.value.status == 6      # updated, not rebuilt
        m.build_lbvh_karas(raw)
        check_scene(stl, raw, spheres=moved)
    finally:
        raw.close()


def test_a_null_scene_is_an_argument_error():
    assert m.lib().mirt_get_records(None, None, None, None, None, None, None, None, None, None) == 3
    assert "mirt_get_records: null scene" in m.lib().mirt_last_error().decode()

"""Closest-point queries (include/mirt_closest.h: mirt_closest_points): what only this header says, the wrappers' checks, the
kernel's code generation, the numpy restatement of the header (tests/closest_ref.py) against a float64 brute force that shares no
code with it, and the header's pruning rule -- the slack -- checked on the CPU over the oracle's tree: with it the pruned walk
gives the brute force's bits, without it it loses answers.  The header against closest.py's signature table and the built
library: tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import closest_ref as cr
import edge_scenes
import light_scenes
import oracle_lib as ol
import pyscene
from codegen_lib import _kernel_body, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24      # float32's unit roundoff


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_says_that_the_arrays_define_the_answer_and_states_the_slack():
    text = open(os.path.join(ROOT, "include", "mirt_closest.h")).read()
    assert "not by the tree" in text and "sigma = 2^-18" in text and "(dist, kind, id)" in text


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    P, Hh, F = torch.zeros((4, 4)), torch.zeros((4, 6), dtype=torch.int32), torch.zeros((4, 8))
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points(raw, P.double(), Hh)
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points(raw, P, Hh.to(torch.int16))
    with pytest.raises(ValueError, match="dtype"):
        m.closest_points(raw, P, Hh, F.double())
    with pytest.raises(ValueError, match="shape"):
        m.closest_points(raw, torch.zeros((4, 3)), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.closest_points(raw, torch.zeros(16), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.closest_points(raw, P, torch.zeros((5, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.closest_points(raw, P, Hh, torch.zeros((4, 7)))
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points(raw, torch.zeros((4, 8))[:, ::2], Hh)
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points(raw, P, torch.zeros((4, 12), dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.closest_points(raw, P, Hh, torch.zeros((4, 16))[:, ::2])
    with pytest.raises(ValueError, match="cuda"):
        m.closest_points(raw, P, Hh, F)
    # pack_points
    xyz = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    rows = m.pack_points(xyz)
    assert rows.shape == (4, 4) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows[:, 0:3], xyz.float()) and bool(torch.all(torch.isinf(rows[:, 3])))
    assert torch.equal(m.pack_points(xyz, 0.5)[:, 3], torch.full((4,), 0.5))
    assert torch.equal(m.pack_points(xyz.numpy(), [1, 2, 3, 4], "cpu")[:, 3], torch.tensor([1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(ValueError, match="shape"):
        m.pack_points(torch.zeros((4, 2)))
    with pytest.raises(ValueError, match="radius"):
        m.pack_points(xyz, [1.0, 2.0])


# ---- code generation ----------------------------------------------------------------------------------------------------------------
def test_closest_kernel_codegen_runs_8_waves_per_simd_with_scratch_only_for_the_stack():
    """closest.hip compiled for gfx950, from the compiler's report: one kernel, within the 64 VGPRs of 8 waves per SIMD (54 when
    this was written), no AGPRs, a 20-entry LDS stack per lane of a 256-thread block, no register spills, the private segment of
    the query kernels, and one scratch store: the push of a stack entry beyond the LDS part."""
    res, asm = _resource_usage("closest.hip")
    assert len(res) == 1 and "closest_points_kernel" in list(res)[0], list(res)
    name, r = list(res.items())[0]
    print(r)
    assert r["Occupancy [waves/SIMD]"] == 8, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
    query, _ = _resource_usage("query.hip")
    assert {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k} == {r["ScratchSize [bytes/lane]"]}
    body = _kernel_body(asm, name)
    assert len([t for t in body if t.startswith("scratch_store")]) == 1


# ---- the restatement against float64 ---------------------------------------------------------------------------------------------------
def _well_shaped_scene(seed=5, ns=40, nt=40):
    """Spheres, triangles and two planes in [-2, 2]^3.  The triangles are well-shaped: edges between 1 and 2, every angle at least
    45 degrees -- the family the rounding bound below is derived for."""
    rng = np.random.default_rng(seed)
    lines = ["png 8 8 closest.png\n", "plane 0 1 0 2.25\n", "plane 1 0.5 0.25 2.5\n"]
    for _ in range(ns):
        c = rng.uniform(-2, 2, 3)
        lines.append("sphere %.5f %.5f %.5f %.5f\n" % (c[0], c[1], c[2], rng.uniform(0.15, 0.5)))
    made = 0
    while made < nt:
        a = rng.uniform(-1.5, 1.5, 3)
        b = a + _unit(rng) * rng.uniform(1, 2)
        c = a + _unit(rng) * rng.uniform(1, 2)
        e = [np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)]
        cosines = [np.dot(b - a, c - a) / (e[0] * e[1]), np.dot(a - b, c - b) / (e[0] * e[2]), np.dot(a - c, b - c) / (e[1] * e[2])]
        if min(e) < 1 or max(e) > 2 or max(cosines) > np.cos(np.radians(45)):
            continue
        for v in (a, b, c):
            lines.append("xyz %.5f %.5f %.5f\n" % tuple(v))
        lines.append("tri -3 -2 -1\n")
        made += 1
    return "".join(lines)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _f64_candidates(arrays, q):
    """Distances [n, candidates] in float64 and a bound on the float32 restatement's rounding error for each, by methods of their
    own: a sphere by the norm, a plane by its unit normal, a triangle by the projection onto its plane where that falls inside and
    the nearest of its three edge segments where it does not.  Columns: spheres, triangles, planes; `kinds`, `ids` name them."""
    q = q.astype(np.float64)
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    cols, tols, kinds, ids = [], [], [], []
    qn = np.abs(q).max(axis=1)
    for j in range(len(S)):
        c, r = S["c"][j].astype(np.float64), float(S["r"][j])
        l = np.linalg.norm(q - c, axis=1)
        cols.append(np.abs(l - r))
        # v = q - c has a relative error U per component; two products, two sums and the root make l's 3.5 U; l - r one more
        tols.append(5 * U * (l + r))
        kinds.append(1), ids.append(j)
    for j in range(len(T)):
        a, b, c = (T[k][j].astype(np.float64) for k in ("p0", "p1", "p2"))
        ab, ac = b - a, c - a
        nrm = np.cross(ab, ac)
        S2 = float(nrm @ nrm)
        ap = q - a
        # projection: barycentric coordinates from the normal equations
        m00, m01, m11 = ab @ ab, ab @ ac, ac @ ac
        r0, r1 = ap @ ab, ap @ ac
        det = m00 * m11 - m01 * m01
        v, w = (m11 * r0 - m01 * r1) / det, (m00 * r1 - m01 * r0) / det
        inside = (v >= 0) & (w >= 0) & (v + w <= 1)
        face = np.abs(ap @ (nrm / np.sqrt(S2)))

        def segment(p0, p1):
            d = p1 - p0
            t = np.clip(((q - p0) @ d) / (d @ d), 0, 1)
            return np.linalg.norm(q - (p0 + t[:, None] * d), axis=1)
        edges = np.minimum(np.minimum(segment(a, b), segment(a, c)), segment(b, c))
        cols.append(np.where(inside, face, edges))
        # L the longest edge, D the largest distance from q to a vertex: every d_k is a dot product of magnitude <= L D with an
        # error of 5 U L D (two differences, three products, two sums); a product of two of them errs by 11 U L^2 D^2, va, vb, vc by
        # 23 U L^2 D^2, a barycentric coordinate -- a quotient by (va + vb) + vc = |ab x ac|^2 = S2 -- by 4 x 23 U L^2 D^2 / S2, P by
        # 2 L times that, rounded to 200 U L^3 D^2 / S2; the edge regions' quotients err by less.  Then P's own three operations,
        # q - P and the length: 8 U (D + |a| + L).
        L = max(np.linalg.norm(ab), np.linalg.norm(ac), np.linalg.norm(c - b))
        D = np.maximum(np.maximum(np.linalg.norm(ap, axis=1), np.linalg.norm(q - b, axis=1)), np.linalg.norm(q - c, axis=1))
        tols.append(U * (200 * L ** 3 * D ** 2 / S2 + 8 * (D + np.abs(a).max() + L)))
        kinds.append(2), ids.append(j)
    for j in range(len(Pl)):
        nor, point = Pl["nor"][j].astype(np.float64), Pl["point"][j].astype(np.float64)
        N = nor / np.linalg.norm(nor)
        cols.append(np.abs((q - point) @ N))
        # N's components 3.5 U each, the difference U, the dot product's three products and two sums: below 16 U |q - point|
        tols.append(16 * U * np.linalg.norm(q - point, axis=1))
        kinds.append(3), ids.append(j)
    return np.stack(cols, axis=1), np.stack(tols, axis=1), np.array(kinds), np.array(ids)


def test_restatement_agrees_with_a_float64_brute_force():
    """2000 points in [-2.5, 2.5]^3 against 40 spheres, 40 well-shaped triangles and 2 planes, R = inf and R = 0.3.  A row is clear
    when the float64 winner's distance plus its rounding bound lies below every other candidate's distance minus its bound (and,
    with a radius, clear of the radius on the same terms).  On clear rows the restatement names the float64 winner and its
    distance is within the winner's bound; the feature row's point is that far from q and its normal faces q.  At most 5 % of the
    rows may be unclear."""
    arrays = pyscene.parse_lines(_well_shaped_scene().split("\n")).arrays()
    rng = np.random.default_rng(21)
    q = rng.uniform(-2.5, 2.5, (2000, 3)).astype(f32)
    d64, tol, kinds, ids = _f64_candidates(arrays, q)
    assert tol.max() < 0.05, tol.max()
    for R in (np.inf, 0.3):
        rows = np.concatenate([q, np.full((len(q), 1), R, f32)], axis=1)
        hits, feat = cr.brute_force(arrays, rows)
        t, kind, pid = hits[:, 0].view(f32), hits[:, 1], hits[:, 2]
        order = np.argsort(d64, axis=1)
        i = np.arange(len(q))
        w = order[:, 0]
        lower = np.where(np.arange(d64.shape[1])[None, :] == w[:, None], np.inf, d64 - tol).min(axis=1)
        upper = d64[i, w] + tol[i, w]
        clear = upper < lower
        admitted = d64[i, w] < R
        if np.isfinite(R):
            clear &= (upper < R) | ((d64 - tol).min(axis=1) > R)
        print(f"R {R}: clear {clear.mean():.4f}, hits {np.mean(kind != 0):.3f}, worst distance error / bound "
              f"{np.max((np.abs(t - d64[i, w]) / tol[i, w])[clear & admitted]):.3g}")
        assert clear.mean() >= 0.95
        hit = clear & admitted
        assert np.array_equal(kind[hit], kinds[w[hit]]) and np.array_equal(pid[hit], ids[w[hit]])
        assert np.all(kind[clear & ~admitted] == 0)
        assert np.all(np.abs(t[hit].astype(np.float64) - d64[i, w][hit]) <= tol[i, w][hit])
        assert len(set(kind[hit].tolist())) == 3 and hit.sum() > (100 if np.isfinite(R) else 1800)
        P, nn = feat[hit, 0:3].astype(np.float64), feat[hit, 4:7].astype(np.float64)
        qq = q[hit].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(qq - P, axis=1) - t[hit]) <= tol[i, w][hit] + 8 * U * 8)
        assert np.all(((qq - P) * nn).sum(axis=1) >= -1e-5) and np.all(np.abs(np.linalg.norm(nn, axis=1) - 1) < 1e-5)
        assert np.all(feat[hit, 3] == 1) and np.all(feat[kind == 0] == 0) and np.all(hits[kind == 0, 0] == f32(-1).view(np.uint32))


# ---- the slack: the pruned walk over the oracle's tree -----------------------------------------------------------------------------
def _oracle_tree(text):
    sc = pyscene.parse_lines(text.split("\n"))
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        return sc.arrays(), o.nodes(), o.refs()
    finally:
        o.close()


def _points_about(arrays, n, seed, pad=0.5):
    """n points, uniform in the box of the spheres' centres and the triangles' vertices grown by `pad`."""
    pts = [arrays["spheres"]["c"]] + [arrays["triangles"][k] for k in ("p0", "p1", "p2")]
    pts = np.concatenate([p.reshape(-1, 3) for p in pts]).astype(np.float64)
    lo, hi = pts.min(axis=0) - pad, pts.max(axis=0) + pad
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32)


def with_tight_radii(arrays, q):
    """Rows (q, inf), and for every q with an answer at distance d the rows (q, d) -- a miss -- and (q, nextafter(d, inf)) -- that
    same record: the radius at which the winner's own boxes have to be visited on the strength of the slack alone."""
    inf_rows = np.concatenate([q, np.full((len(q), 1), np.inf, f32)], axis=1)
    hits, _ = cr.brute_force(arrays, inf_rows)
    d = hits[:, 0].view(f32)
    has = hits[:, 1] != 0
    at = np.concatenate([q[has], d[has, None]], axis=1)
    above = np.concatenate([q[has], np.nextafter(d[has], f32(np.inf))[:, None]], axis=1)
    return np.ascontiguousarray(np.concatenate([inf_rows, at, above]), f32), int(has.sum())


SLACK_SCENES = {
    "far_1e3": lambda: (edge_scenes.far_from_origin(offset=1000.0), 600, 0.5),
    "far_1e5": lambda: (edge_scenes.far_from_origin(offset=100000.0), 300, 0.5),
    "deep_stack": lambda: (edge_scenes.deep_stack(600), 60, 1.5),      # (points inside every box of the nest, and outside)
    "mixed_planes": lambda: (light_scenes.scene("mixed_planes", 3, "mixed"), 600, 0.5),
}


@functools.lru_cache(maxsize=None)
def _slack_case(name):
    text, npoints, pad = SLACK_SCENES[name]()
    arrays, nodes, refs = _oracle_tree(text)
    q = _points_about(arrays, npoints, 31, pad)
    if name.startswith("far"):
        # points straight off a sphere along an axis, where the box's face is as near as the sphere itself: the box bound and the
        # distance then differ by their roundings alone
        S = arrays["spheres"]
        rng = np.random.default_rng(32)
        off = np.zeros((len(S), 3))
        off[np.arange(len(S)), rng.integers(0, 3, len(S))] = (S["r"] + rng.uniform(0.001, 0.05, len(S))) * rng.choice([-1, 1], len(S))
        q = np.concatenate([q, (S["c"].astype(np.float64) + off).astype(f32)])
    rows, nhas = with_tight_radii(arrays, q)
    return arrays, nodes, refs, rows, nhas


@pytest.mark.parametrize("name", list(SLACK_SCENES))
def test_pruned_walk_with_the_slack_equals_the_brute_force_bit_for_bit(name):
    arrays, nodes, refs, rows, nhas = _slack_case(name)
    n = (len(rows) - 2 * nhas)
    want_hits, want_feat = cr.brute_force(arrays, rows)
    # the radius rule: R = d misses, R = nextafter(d) finds the record found without a radius
    assert nhas > 0.9 * n and np.all(want_hits[n:n + nhas, 1] == 0)
    assert np.array_equal(want_hits[n + nhas:], want_hits[:n][want_hits[:n, 1] != 0])
    for near_first in (True, False):
        hits, feat, visited = cr.pruned_walk(arrays, rows, nodes, refs, near_first=near_first)
        assert np.array_equal(hits, want_hits) and np.array_equal(feat.view(np.uint32), want_feat.view(np.uint32)), near_first
    leaves = len(refs)
    print(f"{name}: {leaves} leaves, visited per row: R = inf {visited[:n].mean():.1f}, R = d {visited[n:n + nhas].mean():.1f}")
    assert visited[n:].mean() < (1.0 if name == "deep_stack" else 0.5) * leaves      # (it does prune; inside the nest nothing can be)


@pytest.mark.parametrize("name", ["far_1e3", "far_1e5"])
def test_without_the_slack_the_pruned_walk_loses_answers(name):
    """The negative control: sigma = 0 on a scene away from the origin.  A sphere's float32 box does not bound its float32
    distance, so with R one step above the answer the walk prunes the winner's own box on some rows."""
    arrays, nodes, refs, rows, nhas = _slack_case(name)
    want_hits, _ = cr.brute_force(arrays, rows)
    hits, _, _ = cr.pruned_walk(arrays, rows, nodes, refs, slack=0.0)
    differ = np.any(hits != want_hits, axis=1)
    print(f"{name}: {int(differ.sum())} of {len(rows)} rows differ without the slack")
    assert differ.sum() >= 1

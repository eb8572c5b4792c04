"""Sphere casts (include_ext/mirt_spherecast.h: mirt_cast_spheres): what the header's text says, the wrappers' checks, the kernel's code
generation from the compiler's report, the numpy restatement of the header (tests/spherecast_ref.py) against a float64 brute force
that shares no code with it, and the header's pruning rule checked on the CPU over the oracle's tree: on every input the GPU tests
use the pruned walk gives the brute force's bits.  The header against spherecast.py's signature table and the built library is a row
of tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import re
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import edge_scenes
import light_scenes
import pyscene
import spherecast_ref as sr
from codegen_lib import _resource_usage
from test_closest_abi import _oracle_tree, _points_about, _well_shaped_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include_ext", "mirt_spherecast.h")
f32 = np.float32
u32 = np.uint32
INF = float("inf")
NAN = float("nan")


# ---- header, wrappers ----------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_definition_and_the_pruning_rule():
    text = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert "never by the tree" in text and "(t, kind, id)" in text and "0 <= t < tmax" in text
    assert "tie at t = 0" in text and "mirt_closest_points_multi" in text
    assert "closest-approach form" in text and "Pruning (informative" in text and "sigma = 2^-18" in text and "tau = 2^-20" in text
    assert sr.SLACK == f32(2.0 ** -18) and sr.TAU == f32(2.0 ** -20)


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    Cs, Hh, F = torch.zeros((4, 8)), torch.zeros((4, 6), dtype=torch.int32), torch.zeros((4, 8))
    with pytest.raises(ValueError, match="dtype"):
        m.cast_spheres(raw, Cs.double(), Hh)
    with pytest.raises(ValueError, match="dtype"):
        m.cast_spheres(raw, Cs, Hh.to(torch.int16))
    with pytest.raises(ValueError, match="dtype"):
        m.cast_spheres(raw, Cs, Hh, F.double())
    with pytest.raises(ValueError, match="shape"):
        m.cast_spheres(raw, torch.zeros((4, 4)), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.cast_spheres(raw, torch.zeros(32), Hh)
    with pytest.raises(ValueError, match="shape"):
        m.cast_spheres(raw, Cs, torch.zeros((5, 6), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        m.cast_spheres(raw, Cs, Hh, torch.zeros((4, 7)))
    with pytest.raises(ValueError, match="contiguous"):
        m.cast_spheres(raw, torch.zeros((4, 16))[:, ::2], Hh)
    with pytest.raises(ValueError, match="contiguous"):
        m.cast_spheres(raw, Cs, torch.zeros((4, 12), dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.cast_spheres(raw, Cs, Hh, torch.zeros((4, 16))[:, ::2], any_hit=True)
    with pytest.raises(ValueError, match="cuda"):
        m.cast_spheres(raw, Cs, Hh, F)
    # pack_casts
    o = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    d = torch.ones((4, 3), dtype=torch.float64)
    rows = m.pack_casts(o, d)
    assert rows.shape == (4, 8) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows[:, 0:3], o.float()) and torch.equal(rows[:, 4:7], d.float())
    assert bool(torch.all(torch.isinf(rows[:, 3]))) and bool(torch.all(rows[:, 7] == 0))
    rows = m.pack_casts([1.0, 2.0, 3.0], d.numpy(), 5.0, [0.1, 0.2, 0.3, 0.4])
    assert torch.equal(rows[:, 0:3], torch.tensor([[1.0, 2.0, 3.0]] * 4)) and torch.equal(rows[:, 3], torch.full((4,), 5.0))
    assert torch.equal(rows[:, 7], torch.tensor([0.1, 0.2, 0.3, 0.4]))
    with pytest.raises(ValueError, match="shape"):
        m.pack_casts(o, torch.zeros((4, 2)))
    with pytest.raises(ValueError, match="shape"):
        m.pack_casts(torch.zeros((3, 3)), d)
    with pytest.raises(ValueError, match="tmax"):
        m.pack_casts(o, d, [1.0, 2.0])
    with pytest.raises(ValueError, match="r has shape"):
        m.pack_casts(o, d, 1.0, [1.0, 2.0])


# ---- code generation ----------------------------------------------------------------------------------------------------------------
PINNED = (96, 5)      # (VGPRs, waves per SIMD) the compiler reported for both instances


def test_sphere_cast_kernel_codegen_spills_no_register():
    """spherecast.hip compiled for gfx950, from the compiler's report alone: two kernels (first contact, any contact), no VGPR or
    SGPR spill, no AGPR, the 20-entry LDS stack per lane of a 256-thread block, the private segment of trace_rays_kernel (the
    stack's spill array and nothing else), and the registers and waves per SIMD pinned above: 96 VGPRs at 5 waves -- at 6 waves
    (80 VGPRs) the compiler spills 11 and 12 registers, at 8 waves about 30."""
    res, _ = _resource_usage("spherecast.hip")
    by_any = {int(re.search(r"sphere_cast_kernelILb(\d)E", k).group(1)): k for k in res}
    assert sorted(by_any) == [0, 1] and len(res) == 2, list(res)
    query, _ = _resource_usage("query.hip")
    private = {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k}
    assert len(private) == 1
    for any_hit, name in by_any.items():
        r = res[name]
        print(any_hit, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (any_hit, r)
        assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, (any_hit, r)
        assert {r["ScratchSize [bytes/lane]"]} == private, (any_hit, r)
        assert r["VGPRs"] == PINNED[0] and r["Occupancy [waves/SIMD]"] == PINNED[1], (any_hit, r)


# ---- the restatement against float64 ---------------------------------------------------------------------------------------------------
def _f64_triangle_distance(q, a, b, c):
    """(distance, closest point) of the points q [..., 3] to the triangle (a, b, c) in float64: the projection onto the plane where
    it falls inside, else the nearest of the three edge segments."""
    ab, ac = b - a, c - a
    nrm = np.cross(ab, ac)
    nrm = nrm / np.linalg.norm(nrm)
    ap = q - a
    m00, m01, m11 = ab @ ab, ab @ ac, ac @ ac
    r0, r1 = ap @ ab, ap @ ac
    det = m00 * m11 - m01 * m01
    v, w = (m11 * r0 - m01 * r1) / det, (m00 * r1 - m01 * r0) / det
    inside = (v >= 0) & (w >= 0) & (v + w <= 1)
    best_p = q - (ap @ nrm)[..., None] * nrm
    best_d = np.where(inside, np.abs(ap @ nrm), np.inf)
    for p0, p1 in ((a, b), (a, c), (b, c)):
        e = p1 - p0
        s = np.clip(((q - p0) @ e) / (e @ e), 0, 1)
        p = p0 + s[..., None] * e
        dist = np.linalg.norm(q - p, axis=-1)
        closer = dist < best_d
        best_p = np.where(closer[..., None], p, best_p)
        best_d = np.where(closer, dist, best_d)
    return best_d, best_p


def _f64_first_contacts(arrays, rows):
    """For every row and candidate, in float64 and by methods of their own: t of the first contact (inf: none), the contact point,
    and the grazing measure h2 / R^2 with the parameter of the closest approach.  A sphere and a plane in closed form (the
    quadratic's discriminant, which float64 can afford); a triangle by its distance function along the path, which is convex:
    a golden-section search for the closest approach, then a bisection for the first t at which the distance is r.  Columns:
    spheres, triangles, planes; `kinds`, `ids` name them."""
    rows = rows.astype(np.float64)
    o, r = rows[:, 0:3], rows[:, 7]
    d = rows[:, 4:7] / np.linalg.norm(rows[:, 4:7], axis=1)[:, None]
    S, T, Pl = arrays["spheres"], arrays["triangles"], arrays["planes"]
    ts, Ps, grazes, approaches, kinds, ids = [], [], [], [], [], []
    for j in range(len(S)):
        c, rs = S["c"][j].astype(np.float64), float(S["r"][j])
        oc = o - c
        l = np.linalg.norm(oc, axis=1)
        b = (oc * d).sum(axis=1)
        outside = l > rs
        R = np.where(outside, rs + r, rs - r)
        disc = b * b - (l * l - R * R)
        root = np.sqrt(np.maximum(disc, 0))
        t = np.where(outside, -b - root, -b + root)
        t = np.where((disc < 0) | (t < 0), np.inf, t)
        t = np.where(np.abs(l - rs) <= r, 0.0, t)
        Cw = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
        u = (Cw - c) / np.linalg.norm(Cw - c, axis=1)[:, None]
        ts.append(t), Ps.append(c + u * rs), grazes.append(disc / (R * R)), approaches.append(-b)
        kinds.append(1), ids.append(j)
    for j in range(len(T)):
        a, b, c = (T[k][j].astype(np.float64) for k in ("p0", "p1", "p2"))
        L = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
        dist = lambda t: _f64_triangle_distance(o + d * t[:, None], a, b, c)[0]
        lo, hi = np.zeros(len(o)), np.linalg.norm(o - a, axis=1) + 2 * L + r
        g = (np.sqrt(5.0) - 1) / 2
        for _ in range(90):
            x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
            left = dist(x1) < dist(x2)
            lo, hi = np.where(left, lo, x1), np.where(left, x2, hi)
        tmin = 0.5 * (lo + hi)
        dmin = dist(tmin)
        lo, hi = np.zeros(len(o)), tmin.copy()
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            above = dist(mid) > r
            lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
        t = np.where(dmin <= r, hi, np.inf)
        t = np.where(dist(np.zeros(len(o))) <= r, 0.0, t)
        Cw = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
        ts.append(t), Ps.append(_f64_triangle_distance(Cw, a, b, c)[1]), grazes.append((r * r - dmin * dmin) / (r * r)), approaches.append(tmin)
        kinds.append(2), ids.append(j)
    for j in range(len(Pl)):
        nor, point = Pl["nor"][j].astype(np.float64), Pl["point"][j].astype(np.float64)
        N = nor / np.linalg.norm(nor)
        s = (o - point) @ N
        dn = d @ N
        with np.errstate(all="ignore"):
            t = (np.sign(s) * r - s) / dn
        t = np.where(s * dn < 0, t, np.inf)
        t = np.where(np.abs(s) <= r, 0.0, t)
        Cw = o + d * np.where(np.isfinite(t), t, 0.0)[:, None]
        ts.append(t), Ps.append(Cw - ((Cw - point) @ N)[:, None] * N), grazes.append(np.full(len(o), np.inf)), approaches.append(np.full(len(o), np.inf))
        kinds.append(3), ids.append(j)
    return np.stack(ts, axis=1), np.stack(Ps, axis=1), np.stack(grazes, axis=1), np.stack(approaches, axis=1), np.array(kinds), np.array(ids)


T_MEASURED, P_MEASURED = 5.6e-6, 4.6e-6      # the largest errors of t and of a coordinate of P, each divided by max(t, 1)


def test_restatement_agrees_with_a_float64_brute_force():
    """1500 casts in [-2.5, 2.5]^3 against 40 spheres, 40 well-shaped triangles and 2 planes, radii 0.02 to 0.15, tmax = inf.
    Rows are set aside as ill-conditioned when a candidate that could be the answer grazes (|h2| below 1e-3 R^2 in float64, its
    closest approach no later than the winner's contact) or when two candidates' float64 t lie within 1e-4 relative (t2 - t1 <= 1e-4 t2; two
    overlaps at the start, both at 0, are such a pair).  At most 5 % of the rows may be set aside (2.4 % are, all of them close pairs).  On the kept rows the restatement names
    the float64 winner.  The tolerances are 4 x the largest float32-vs-float64 errors measured on the kept rows of these seeds,
    relative to max(t, 1) because a far plane met at a shallow angle has an error that grows with t: 5.53e-6 for t and 4.52e-6
    for a coordinate of P (T_MEASURED, P_MEASURED above, rounded up)."""
    arrays = pyscene.parse_lines(_well_shaped_scene().split("\n")).arrays()
    rng = np.random.default_rng(61)
    n = 1500
    o = rng.uniform(-2.5, 2.5, (n, 3))
    d = rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0, (n, 1))
    rows = np.concatenate([o, np.full((n, 1), np.inf), d, rng.uniform(0.02, 0.15, (n, 1))], axis=1).astype(f32)
    t64, P64, graze, approach, kinds, ids = _f64_first_contacts(arrays, rows)
    order = np.argsort(t64, axis=1, kind="stable")
    i = np.arange(n)
    w, second = order[:, 0], order[:, 1]
    tw, t2 = t64[i, w], t64[i, second]
    has = np.isfinite(tw)
    close = has & np.isfinite(t2) & (t2 - tw <= 1e-4 * t2)
    limit = np.where(has, tw, np.inf)[:, None]
    grazing = np.any((np.abs(graze) < 1e-3) & (approach >= 0) & (approach <= limit * (1 + 1e-4) + 1e-4), axis=1)
    kept = ~(close | grazing)
    hits, feat = sr.brute_force(arrays, rows)
    t, kind, pid = hits[:, 0].view(f32), hits[:, 1], hits[:, 2]
    hit = kept & has
    scale = np.maximum(tw[hit], 1.0)      # (a far plane met at a shallow angle: the error grows with t)
    t_err = (np.abs(t[hit].astype(np.float64) - tw[hit]) / scale).max()
    p_err = (np.abs(feat[hit, 0:3].astype(np.float64) - P64[i, w][hit]).max(axis=1) / scale).max()
    print(f"set aside {1 - kept.mean():.4f} (close {close.mean():.4f}, grazing {grazing.mean():.4f}); hits {has.mean():.3f}; "
          f"largest error on the kept rows: t {t_err:.3g}, P {p_err:.3g}; kinds {sorted(set(kind[hit].tolist()))}, t = 0 on {np.mean(tw[hit] == 0):.3f}")
    assert kept.mean() >= 0.95
    assert np.array_equal(kind[hit], kinds[w[hit]]) and np.array_equal(pid[hit], ids[w[hit]])
    assert np.all(kind[kept & ~has] == 0)
    assert t_err <= 4 * T_MEASURED and p_err <= 4 * P_MEASURED
    assert len(set(kind[hit].tolist())) == 3 and hit.sum() > 1000 and 0.02 < np.mean(tw[hit] == 0) < 0.5
    # the record: the normal is the unit vector from P to the centre at contact, which is r from P
    Cw = rows[hit, 0:3].astype(np.float64) + (rows[hit, 4:7] / np.linalg.norm(rows[hit, 4:7].astype(np.float64), axis=1)[:, None]) * tw[hit][:, None]
    away = Cw - feat[hit, 0:3]
    moving = tw[hit] > 0
    assert np.all((np.abs(np.linalg.norm(away, axis=1) - rows[hit, 7]) / scale)[moving] <= 2 * 4 * P_MEASURED)
    nn = feat[hit, 4:7].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(nn, axis=1) - 1) < 1e-5) and np.all((away * nn).sum(axis=1)[moving] > 0.9 * rows[hit, 7][moving])
    assert np.all(feat[hit, 3] == 1) and np.all(feat[kind == 0] == 0) and np.all(hits[kind == 0, 0] == f32(-1).view(u32))


# ---- the inputs (the GPU tests use the same) -----------------------------------------------------------------------------------------
def _arrays(text):
    return pyscene.parse_lines(text.split("\n")).arrays()


def shuffled(rows, seed=1):
    """(so that rows with and without a bound, tight and loose, sit in the same wave)"""
    return np.ascontiguousarray(rows[np.random.default_rng(seed).permutation(len(rows))])


def casts_about(arrays, n, seed, pad, rmax, zero_share=0.15):
    """n rows with tmax = inf: origins uniform in the box of the primitives grown by `pad` (_points_about), directions of any
    length, half of them all around and half towards a point of the primitives' box, radii uniform in 0..rmax with a share of
    exact zeros."""
    rng = np.random.default_rng(seed + 1000)
    o = _points_about(arrays, n, seed, pad)
    d = rng.normal(size=(n, 3))
    d[::2] = _points_about(arrays, n, seed + 2000, 0.0)[::2].astype(np.float64) - o[::2]
    d = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.2, 4.0, (n, 1))
    r = rng.uniform(0.0, rmax, (n, 1)) * (rng.random((n, 1)) >= zero_share)
    return np.ascontiguousarray(np.concatenate([o, np.full((n, 1), np.inf), d, r], axis=1), f32)


def with_tight_tmax(arrays, rows):
    """The rows, and for every row with an answer at t the same cast with tmax = t -- a miss -- and tmax = nextafter(t, inf) --
    that same record: the bound at which the winner's own boxes have to be visited on the strength of the slacks alone."""
    hits, _ = sr.brute_force(arrays, rows)
    t = hits[:, 0].view(f32)
    has = hits[:, 1] != 0
    at, above = rows[has].copy(), rows[has].copy()
    at[:, 3] = t[has]
    above[:, 3] = np.nextafter(t[has], f32(np.inf))
    return np.ascontiguousarray(np.concatenate([rows, at, above]), f32), int(has.sum())


def _mixed_case(geometry):
    text = light_scenes.scene(geometry, 3, "mixed")
    arrays = _arrays(text)
    rows, _ = with_tight_tmax(arrays, casts_about(arrays, 300 if geometry.endswith("_planes") else 450, 71, 1.0, 0.7))
    loose = casts_about(arrays, 200, 72, 1.0, 0.7)
    loose[:, 3] = np.random.default_rng(73).uniform(0.2, 4.0, 200).astype(f32)
    return text, shuffled(np.concatenate([rows, loose]))


def _smallest_case(name):
    text = edge_scenes.ALL[name]()
    rng = np.random.default_rng(5)
    o = rng.uniform(-3, 3, (150, 3))
    o[:, 2] -= 2
    d = rng.normal(size=(150, 3))
    d[:75] = (np.array([0.0, 0.0, -2.0]) + rng.uniform(-1, 1, (75, 3))) - o[:75]      # (half of them towards the primitive)
    rows = np.concatenate([o, np.full((150, 1), np.inf), d, rng.uniform(0, 0.5, (150, 1)) * (rng.random((150, 1)) > 0.2)], axis=1).astype(f32)
    rows, _ = with_tight_tmax(_arrays(text), rows)
    return text, shuffled(np.ascontiguousarray(rows[:300]))


def _deep_case():
    text = edge_scenes.deep_stack()
    arrays = _arrays(text)
    rows, _ = with_tight_tmax(arrays, casts_about(arrays, 80, 44, 0.6, 0.2, zero_share=0.6))      # (most origins within the nest, most balls a point)
    return text, shuffled(rows)


def _far_case(offset):
    """far_from_origin: casts about the cluster, and casts straight at a sphere along an axis from just off it, where the box's face
    is as near as the sphere itself: the slab parameter and the candidate's t then differ by their roundings alone."""
    text = edge_scenes.far_from_origin(offset=offset)
    arrays = _arrays(text)
    rows = casts_about(arrays, 250, 31, 0.5, 0.1)
    S = arrays["spheres"]
    rng = np.random.default_rng(32)
    axis = rng.integers(0, 3, len(S))
    sign = rng.choice([-1.0, 1.0], len(S))
    r = rng.uniform(0.0, 0.05, len(S)) * (rng.random(len(S)) > 0.3)
    off = np.zeros((len(S), 3))
    off[np.arange(len(S)), axis] = (S["r"] + r + rng.uniform(0.001, 0.3, len(S))) * sign
    d = np.zeros((len(S), 3))
    d[np.arange(len(S)), axis] = -sign
    straight = np.concatenate([S["c"].astype(np.float64) + off, np.full((len(S), 1), np.inf), d, r[:, None]], axis=1).astype(f32)
    rows, _ = with_tight_tmax(arrays, np.concatenate([rows, straight]))
    return text, shuffled(rows)


def _row_count_case():
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    arrays = _arrays(text)
    rows = casts_about(arrays, 4096, 45, 1.0, 0.6)
    rows[:, 3] = np.random.default_rng(46).choice([0.5, 2.0, np.inf], 4096).astype(f32)
    return text, rows


CHOSEN = """png 8 8 chosen.png
plane 0 1 0 50
xyz 0 0 0
xyz 2 0 0
xyz 0 2 0
tri 1 2 3
sphere 10 0 0 1
sphere 10 0 0 1
sphere 0 20 0 4
sphere 30 0 0 1
xyz 29 -4 2
xyz 29 4 2
xyz 29 0 -6
tri 4 5 6
xyz 40 0 0
xyz 41 0 0
xyz 42 0 0
tri 7 8 9
xyz 40 1 0
xyz 42 1 0
xyz 41 3 0
tri 10 11 12
sphere 62 0 0 1
sphere 60 2 0 1
sphere 60 0 2 1
sphere 58 0 0 1
sphere 60 -2 0 1
sphere 60 0 -2 1
xyz 80 0 0
xyz 80.0009 0 0
xyz 80 0.0009 0
tri 13 14 15
"""
# the rows of the chosen scene, group by group: (name, rows); the GPU test reads its expectations by these names
H = 0.5


def chosen_groups():
    down, up = (0, 0, -1), (0, 0, 1)
    row = lambda o, d, r, tmax=INF: tuple(o) + (tmax,) + tuple(d) + (r,)
    groups = []
    # a ball of radius 0.5 dropped along -z from z = 3 onto the first triangle: its face, its three edges, its three vertices
    groups.append(("face", [row((0.5, 0.5, 3), down, H)]))
    groups.append(("edges", [row((1, -0.25, 3), down, H), row((-0.25, 1, 3), down, H), row((1.25, 1.25, 3), down, H)]))
    groups.append(("vertices", [row((-0.25, -0.25, 3), down, H), row((2.25, -0.25, 3), down, H), row((-0.25, 2.25, 3), down, H)]))
    # the big sphere (0, 20, 0) of radius 4: from inside moving out, from outside moving in, a near-tangent pass, a clear pass
    groups.append(("big_sphere", [row((0, 20, 0), (1, 0, 0), H), row((0, 21, 0), (0, -2, 0), 1.0), row((0, 30, 0), (0, -1, 0), H),
                                  row((-10, 24.4375, 0), (1, 0, 0), H), row((-10, 24.5625, 0), (1, 0, 0), H)]))
    # the plane y = -50 from above, from below, parallel to it, moving away
    groups.append(("plane", [row((100, -40, 0), (0, -1, 0), 1.0), row((100, -60, 0), (0, 3, 0), 1.0), row((100, -40, 0), (1, 0, 0), 1.0),
                             row((100, -40, 0), (0, 1, 0), 1.0), row((100, -60, 0), (0.6, -0.8, 0), 1.0, 1000.0)]))
    # overlap at the start with each kind: t = 0
    groups.append(("overlap", [row((0.5, 0.5, 0.25), up, H), row((10, 1.25, 0), (0, 1, 0), H), row((100, -49.75, 0), (0, 1, 0), H),
                               row((0, 16.25, 0), (1, 0, 0), H), row((0.5, 0.5, 0.5), up, H)]))
    # twin spheres: the id tie; sphere 3 and triangle 1 first touched at the same t: the kind tie
    groups.append(("twins", [row((10, 5, 0), (0, -1, 0), H), row((13, 0, 0), (-1, 0, 0), 0.25)]))
    groups.append(("kind_tie", [row((25, 0, 0), (1, 0, 0), H), row((25, 0, 0), (1, 0, 0), 0.0)]))
    # six equal spheres about (60, 0, 0), whose sorted-leaf order is not file order: a ball that touches all six at the start,
    # then smaller ones towards one of them
    groups.append(("six", [row((60, 0, 0), (0, 1, 0), 1.0), row((60, 0, 0), (0, 1, 0), H), row((60, 0, 0), (0, -1, 0), H, 0.75),
                           row((60, 0, 0), (1, 0, 0), 0.0)]))
    # the triangle without area beside a real one
    groups.append(("no_area", [row((40.5, -3, 0), (0, 1, 0), H), row((41, 0.5, 3), down, 0.25), row((39, 0, 3), down, H), row((44, 0, 0), (-1, 0, 0), H),
                               row((41, -3, 0), (0, 1, 0), 0.0)]))
    # a small triangle of positive area whose record normal is (0, 0, 0) (its cross product is shorter than 1e-6): a ball far above
    # it passing by, a ray pointing away from it, a ball dropped onto it (met by its edges, 2e-7 past the face), a ray through it
    groups.append(("small", [row((80.0002, 0.0002, 5), (1, 0, 0), 0.1), row((80.0002, 0.0002, 5), up, 0.0), row((80.0002, 0.0002, 3), down, 0.1),
                             row((80.0002, 0.0002, 3), down, 0.0, 10.0)]))
    # tmax just below and just above the contact at t = 2.5
    groups.append(("tmax", [row((0.5, 0.5, 3), down, H, 2.5), row((0.5, 0.5, 3), down, H, float(np.nextafter(f32(2.5), f32(3)))),
                            row((0.5, 0.5, 3), down, H, float(np.nextafter(f32(2.5), f32(2))))]))
    # r = 0: a ray
    groups.append(("ray", [row((0.5, 0.5, 3), down, 0.0), row((0, 30, 0), (0, -1, 0), 0.0), row((3, 3, 3), down, 0.0, 10.0)]))
    # dead rows
    groups.append(("dead", [row((0.5, 0.5, 3), down, H, 0.0), row((0.5, 0.5, 3), down, H, -1.0), row((0.5, 0.5, 3), down, H, NAN),
                            row((0.5, 0.5, 3), down, -1.0), row((0.5, 0.5, 3), down, NAN), row((0.5, 0.5, 3), down, INF),
                            row((NAN, 0.5, 3), down, H), row((0.5, INF, 3), down, H), row((0.5, 0.5, -INF), down, H),
                            row((0.5, 0.5, 3), (0, 0, 0), H), row((0.5, 0.5, 3), (0, NAN, -1), H), row((0.5, 0.5, 3), (0, 0, -1e-7), H)]))
    return groups


def _chosen_case():
    return CHOSEN, np.array([r for _, rows in chosen_groups() for r in rows], f32)


def _along_edges_case():
    """Casts aimed along the edges of the mixed scene's triangles, from beyond an end point: exactly along the edge and turned off
    it by 1e-7 to 0.1, the path on the edge's line and up to 0.4 beside it, radii 0 to 0.3 -- the regime in which an edge piece's
    A = |d^ - e (d^ . e) / (e . e)|^2 is small or zero and its t ill-conditioned."""
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    arrays = _arrays(text)
    T = arrays["triangles"]
    rng = np.random.default_rng(81)
    rows = []
    for j in range(len(T)):
        v = [T[k][j].astype(np.float64) for k in ("p0", "p1", "p2")]
        for p, q in ((v[0], v[1]), (v[0], v[2]), (v[1], v[2]), (v[1], v[0]), (v[2], v[0]), (v[2], v[1])):
            e = (q - p) / np.linalg.norm(q - p)
            for turn in (0.0, 1e-7, 1e-5, 1e-3, 1e-2, 0.1):
                for beside in (0.0, 0.05, 0.4):
                    for r in (0.0, 0.01, 0.1, 0.3):
                        side = np.cross(e, rng.normal(size=3))
                        side /= np.linalg.norm(side)
                        off = np.cross(e, rng.normal(size=3))
                        off /= np.linalg.norm(off)
                        o = p - e * rng.uniform(0.5, 2.0) + side * beside
                        rows.append(np.concatenate([o, [np.inf], (e + off * turn) * rng.uniform(0.5, 2.0), [r]]))
    rows, _ = with_tight_tmax(arrays, np.array(rows, f32))
    return text, shuffled(rows)


UPDATE_MOVED = ("sphere 0.9 -0.2 -2.6 0.6", "sphere 0.3 0.4 -2.4 0.7")


def _update_case():
    text = light_scenes.scene("spheres_planes", 3, "mixed").replace(*UPDATE_MOVED)
    return text, casts_about(_arrays(text), 600, 48, 1.0, 0.5)


def _visibility_case():
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    rows = casts_about(_arrays(text), 500, 47, 1.0, 0.4)
    rows[:, 3] = 3.0
    return text, rows


CASES = {"mixed": lambda: _mixed_case("mixed"), "mixed_planes": lambda: _mixed_case("mixed_planes"),
         "single_sphere": lambda: _smallest_case("single_sphere"), "single_triangle": lambda: _smallest_case("single_triangle"),
         "empty": lambda: _smallest_case("empty"), "plane_only": lambda: _smallest_case("plane_only"),
         "deep_stack": _deep_case, "far_1e3": lambda: _far_case(1000.0), "far_1e5": lambda: _far_case(100000.0),
         "row_counts": _row_count_case, "chosen": _chosen_case, "along_edges": _along_edges_case, "update": _update_case, "visibility": _visibility_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, arrays, rows) of a case."""
    text, rows = CASES[name]()
    return text, _arrays(text), rows


@functools.lru_cache(maxsize=None)
def reference(name):
    """(hits, features, candidates) of a case by the brute force: what the GPU tests compare against."""
    _, arrays, rows = case(name)
    cands = sr.candidates(arrays, rows)
    return sr.brute_force(arrays, rows, cands) + (cands,)


# ---- the reference against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pruned_walk_equals_the_brute_force_bit_for_bit(name):
    text, arrays, rows = case(name)
    _, nodes, refs = _oracle_tree(text)
    want_hits, want_feat = reference(name)[:2]
    for near_first in (True, False):
        hits, feat, visited = sr.pruned_walk(arrays, rows, nodes, refs, near_first=near_first)
        assert np.array_equal(hits, want_hits) and np.array_equal(feat.view(u32), want_feat.view(u32)), near_first
        if near_first and len(refs) > 100:
            print(f"{name}: {len(refs)} leaves, visited per row {visited.mean():.1f}")
            assert visited.mean() < (1.0 if name == "deep_stack" else 0.5) * len(refs)      # (it does prune; inside the nest nothing can be)
    hits, feat, _ = sr.pruned_walk(arrays, rows, nodes, refs, any_hit=True)
    assert len(sr.any_hit_is_valid(arrays, rows, hits, feat)) == 0


def test_the_cases_reach_every_kind_of_answer():
    for name in ("mixed", "mixed_planes"):
        hits, feat, _ = reference(name)
        t, kind = hits[:, 0].view(f32), hits[:, 1]
        want = {0, 1, 2, 3} if name == "mixed_planes" else {0, 1, 2}
        assert set(kind.tolist()) == want and set(kind[t == 0].tolist()) == want - {0} and set(kind[t > 0].tolist()) == want - {0}, name
        _, _, rows = case(name)
        assert 900 <= len(rows) <= 1100 and np.mean(rows[:, 7] == 0) > 0.05 and np.mean(np.isinf(rows[:, 3])) > 0.2
    for name, kinds in (("single_sphere", {0, 1}), ("single_triangle", {0, 2}), ("empty", {0}), ("plane_only", {0, 3})):
        assert set(reference(name)[0][:, 1].tolist()) == kinds and len(case(name)[2]) <= 300, name
    assert len(set(reference("deep_stack")[0][:, 2].tolist())) > 10
    for name in ("far_1e3", "far_1e5"):
        kind = reference(name)[0][:, 1]
        assert np.count_nonzero(kind == 1) > 500 and np.count_nonzero(kind == 0) > 300, name


@pytest.mark.parametrize("name", ["far_1e3", "far_1e5"])
def test_without_the_slacks_the_pruned_walk_loses_answers(name):
    """The negative control: sigma = 0 and tau = 0 on a scene away from the origin.  A sphere's float32 box does not bound its
    float32 contact, so with tmax one step above the answer the walk prunes the winner's own box on some rows: 61 of 1562 at an
    offset of 1e3 and 60 at 1e5 when this was written.  (With sigma alone none is lost on these rows, with tau alone 35 and 34:
    tau rests on the count of DESIGN.md section 6v alone.)"""
    text, arrays, rows = case(name)
    _, nodes, refs = _oracle_tree(text)
    want_hits = reference(name)[0]
    hits, _, _ = sr.pruned_walk(arrays, rows, nodes, refs, slack=0.0, tau=0.0)
    differ = np.any(hits != want_hits, axis=1)
    print(f"{name}: {int(differ.sum())} of {len(rows)} rows differ without the slacks")
    assert differ.sum() >= 1

"""Closest-point queries on the GPU (include/mirt_closest.h: mirt_closest_points; closest.closest_points).  The yardstick is
tests/closest_ref.py, the numpy restatement of the header as a brute force over every candidate: hits and feature rows are compared
on bit patterns, whatever the scene's tree makes the kernel visit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import closest
import closest_ref as cr
import edge_scenes
import light_scenes
import pyscene
from test_closest_abi import _points_about, with_tight_radii
from test_gpu_visibility import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
INF = float("inf")
NAN = float("nan")


def _scene(text, **options):
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _arrays(text):
    return pyscene.parse_lines(text.split("\n")).arrays()


def _query(raw, rows, want_features=True, stream=None):
    """mirt_closest_points on the rows (numpy [n, 4]): (hits uint32 [n, 6], features float32 [n, 8] or None); the row after the
    last keeps its sentinel."""
    n = len(rows)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    hits = torch.full((n + 1, 6), -7, dtype=torch.int32, device=DEV)
    feat = torch.full((n + 1, 8), -7.0, dtype=torch.float32, device=DEV) if want_features else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.closest_points(raw, d_rows, hits[:n], feat[:n] if want_features else None, stream=stream)
    torch.cuda.synchronize()
    assert bool(torch.all(hits[n] == -7)) and (feat is None or bool(torch.all(feat[n] == -7.0)))
    return hits[:n].cpu().numpy().view(np.uint32), (feat[:n].cpu().numpy() if want_features else None)


def _hit_bits(h):
    """MirtHit words with the float columns' NaNs folded."""
    out = h.copy()
    out[:, 0] = bits(h[:, 0].view(f32))
    out[:, 3:6] = bits(h[:, 3:6].view(f32))
    return out


def _assert_equals_brute_force(raw, arrays, rows):
    want_hits, want_feat = cr.brute_force(arrays, rows)
    hits, feat = _query(raw, rows)
    bad = np.flatnonzero(np.any(_hit_bits(hits) != _hit_bits(want_hits), axis=1) | np.any(bits(feat) != bits(want_feat), axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:5]], hits[bad[:5]], want_hits[bad[:5]])
    only_hits, none = _query(raw, rows, want_features=False)      # d_features == NULL: the same hits
    assert none is None and np.array_equal(only_hits, hits)
    return hits, feat


def _shuffled(rows, seed=1):
    """(so that rows with and without a radius, tight and loose, sit in the same wave)"""
    return np.ascontiguousarray(rows[np.random.default_rng(seed).permutation(len(rows))])


# ---- 1. scenes against the brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["mixed", "mixed_planes"])
def test_mixed_scenes_equal_the_brute_force(geometry):
    text = light_scenes.scene(geometry, 3, "mixed")
    arrays = _arrays(text)
    rows, nhas = with_tight_radii(arrays, _points_about(arrays, 700, 41, 1.0))
    some = _points_about(arrays, 300, 42, 1.0)
    rows = _shuffled(np.concatenate([rows, np.concatenate([some, np.random.default_rng(43).uniform(0.05, 1.5, (300, 1)).astype(f32)], axis=1)]))
    raw = _scene(text)
    try:
        hits, feat = _assert_equals_brute_force(raw, arrays, rows)
    finally:
        raw.close()
    kinds = set(hits[:, 1].tolist())
    assert kinds == ({0, 1, 2, 3} if geometry.endswith("_planes") else {0, 1, 2}), kinds
    hit = hits[:, 1] != 0
    assert np.all(feat[hit, 3] == 1) and np.all(feat[~hit] == 0) and np.all(hits[~hit, 0] == f32(-1).view(np.uint32))
    # api.unpack_hits reads the records unchanged
    t, kind, pid, nn = m.unpack_hits(torch.from_numpy(hits.view(np.int32)))
    assert np.array_equal(t.numpy().view(np.uint32), hits[:, 0]) and np.array_equal(kind.numpy().view(np.uint32), hits[:, 1])
    assert np.array_equal(nn.numpy(), feat[:, 4:7])


@pytest.mark.parametrize("name", ["single_sphere", "single_triangle", "empty", "plane_only"])
def test_smallest_scenes(name):
    text = edge_scenes.ALL[name]()
    arrays = _arrays(text)
    q = np.random.default_rng(5).uniform(-3, 3, (300, 3)).astype(f32)
    q[:, 2] -= 2
    rows, nhas = with_tight_radii(arrays, q)
    raw = _scene(text)
    try:
        hits, _ = _assert_equals_brute_force(raw, arrays, _shuffled(rows))
    finally:
        raw.close()
    assert set(hits[:, 1].tolist()) == {"single_sphere": {0, 1}, "single_triangle": {0, 2}, "empty": {0}, "plane_only": {0, 3}}[name]


@functools.lru_cache(maxsize=None)
def _deep_stack_case():
    text = edge_scenes.deep_stack()
    arrays = _arrays(text)
    rows, _ = with_tight_radii(arrays, _points_about(arrays, 250, 44, 1.5))
    rows = _shuffled(rows)
    return text, arrays, rows, cr.brute_force(arrays, rows)


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, arrays, rows, (want_hits, want_feat) = _deep_stack_case()
    raw = _scene(text)
    try:
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            raw.set_option("stack_lds_depth", depth)
        hits, feat = _query(raw, rows)
    finally:
        raw.close()
    assert np.array_equal(_hit_bits(hits), _hit_bits(want_hits)) and np.array_equal(bits(feat), bits(want_feat))
    assert len(set(hits[:, 2].tolist())) > 10      # (outside the nest the largest few spheres, inside it any of them)


@pytest.mark.parametrize("offset", [1000.0, 100000.0])
def test_far_from_origin_where_the_boxes_do_not_bound_the_distances(offset):
    """The scenes of the CPU slack test (tests/test_closest_abi.py): a kernel that pruned at its best distance without the
    header's slack would lose rows here."""
    text = edge_scenes.far_from_origin(offset=offset)
    arrays = _arrays(text)
    q = _points_about(arrays, 500, 31, 0.5)
    S = arrays["spheres"]
    rng = np.random.default_rng(32)
    off = np.zeros((len(S), 3))
    off[np.arange(len(S)), rng.integers(0, 3, len(S))] = (S["r"] + rng.uniform(0.001, 0.05, len(S))) * rng.choice([-1, 1], len(S))
    q = np.concatenate([q, (S["c"].astype(np.float64) + off).astype(f32)])
    rows, nhas = with_tight_radii(arrays, q)
    raw = _scene(text)
    try:
        hits, _ = _assert_equals_brute_force(raw, arrays, _shuffled(rows))
    finally:
        raw.close()
    assert np.count_nonzero(hits[:, 1] == 1) > 800 and np.count_nonzero(hits[:, 1] == 0) > 700


# ---- 2. row counts ------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_a_wave_a_block_and_a_grid():
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    arrays = _arrays(text)
    base = np.concatenate([_points_about(arrays, 4096, 45, 1.0), np.random.default_rng(46).choice([0.2, 0.8, np.inf], (4096, 1)).astype(f32)], axis=1)
    want_hits, want_feat = cr.brute_force(arrays, base)
    assert set(want_hits[:257, 1].tolist()) == {0, 1, 2, 3}
    raw = _scene(text)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257):
            hits, feat = _query(raw, base[:n])
            assert np.array_equal(hits, want_hits[:n]) and np.array_equal(bits(feat), bits(want_feat[:n])), n
        # more rows than a grid's worth of lanes: every lane takes a second row
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37
        reps = -(-n // 4096)
        hits, feat = _query(raw, np.tile(base, (reps, 1))[:n])
        assert np.array_equal(hits, np.tile(want_hits, (reps, 1))[:n]) and np.array_equal(bits(feat), bits(np.tile(want_feat, (reps, 1))[:n]))
    finally:
        raw.close()


# ---- 3. chosen rows -------------------------------------------------------------------------------------------------------------------
CHOSEN = """png 8 8 chosen.png
xyz 0 0 0
xyz 2 0 0
xyz 0 2 0
tri 1 2 3
sphere 5 0 0 1
sphere 5 0 0 1
sphere 0 10 0 1
sphere 10 0 0 1
xyz 13 -4 -4
xyz 13 4 -4
xyz 13 0 6
tri 4 5 6
xyz 20 0 0
xyz 21 0 0
xyz 22 0 0
tri 7 8 9
xyz 20 1 0
xyz 22 1 0
xyz 21 3 0
tri 10 11 12
"""


def test_chosen_rows():
    arrays = _arrays(CHOSEN)
    R = 1.0      # (keeps the other primitives out of the first triangle's rows)
    tri_regions = [(-0.5, -0.5, 0.5), (2.5, -0.25, 0.5), (1.0, -0.5, 0.5), (-0.25, 2.5, 0.5), (-0.5, 1.0, 0.5), (1.5, 1.5, 0.5), (0.5, 0.5, 0.5)]
    rows = [p + (R,) for p in tri_regions]                                               # vertex a, b, edge ab, c, edge ac, edge bc, the face
    rows += [(0, 0, 0, R), (2, 0, 0, R), (1, 0, 0, R), (1, 1, 0, R), (0.5, 0.5, 0, R), (0.5, 0.5, -0.25, R)]      # on a vertex, an edge, the face; below it
    rows += [(0, 10, 0, INF), (0, 10.5, 0, INF), (0, 11, 0, INF), (0, 12, 0, 1.5), (0, 10, 1e-7, 2.0)]   # at a sphere's centre, inside it, on it, outside
    rows += [(5, 3, 0, INF), (5, 0, 0.5, INF), (7, 0, 0, INF)]                                            # two identical spheres: the id tie
    rows += [(12, 0, 0, INF), (12, 0, 0, 1.0), (12, 0, 0, np.nextafter(f32(1), f32(2)))]               # sphere 3 and triangle 1 both at 1: the kind tie
    rows += [(20.5, -0.25, 0, INF), (21, 0.5, 0, INF), (19, 0, 0, INF), (21.5, 0.25, 0.5, INF), (23, -1, 0, 2.0)]   # the triangle without area beside a real one
    ndead = 6
    rows += [(1, 1, 1, 0.0), (1, 1, 1, -1.0), (1, 1, 1, NAN), (NAN, 1, 1, INF), (1, INF, 1, INF), (1, 1, -INF, 5.0)]
    rows = np.array(rows, f32)
    raw = _scene(CHOSEN)
    try:
        hits, feat = _assert_equals_brute_force(raw, arrays, rows)
    finally:
        raw.close()
    t, kind, pid = hits[:, 0].view(f32), hits[:, 1].tolist(), hits[:, 2].tolist()
    assert kind[:13] == [2] * 13 and pid[:13] == [0] * 13
    P = feat[:, 0:3]
    assert np.array_equal(P[:7], np.array([(0, 0, 0), (2, 0, 0), (1, 0, 0), (0, 2, 0), (0, 1, 0), (1, 1, 0), (0.5, 0.5, 0)], f32))
    assert np.all(t[7:12] == 0) and t[12] == 0.25 and np.array_equal(feat[12, 4:7], np.array([0, 0, -1], f32)) and feat[6, 6] == 1
    assert kind[13:18] == [1] * 5 and pid[13:18] == [2] * 5
    assert t[13] == 1 and np.all(feat[13, 4:7] == 0) and np.array_equal(P[13], np.array([0, 10, 0], f32))      # the centre: u = 0, P = c
    assert t[14] == 0.5 and np.array_equal(feat[14, 4:7], np.array([0, -1, 0], f32)) and t[15] == 0 and t[16] == 1
    assert np.all(feat[17, 4:7] == 0) and np.array_equal(P[17], np.array([0, 10, 0], f32))                      # within 1e-6 of the centre
    assert kind[18:21] == [1] * 3 and pid[18:21] == [0] * 3                                                      # the lower id of the twins
    assert (kind[21], pid[21], t[21]) == (1, 3, 1.0) and kind[22] == 0 and (kind[23], pid[23]) == (1, 3)       # the sphere before the triangle
    assert set(zip(kind[24:29], pid[24:29])) <= {(2, 2), (2, 3)} and (2, 2) in set(zip(kind[24:29], pid[24:29]))
    assert kind[-ndead:] == [0] * ndead and np.all(feat[-ndead:] == 0)


# ---- 4. into the surface-point queries -----------------------------------------------------------------------------------------------
def test_feature_rows_feed_hemisphere_visibility():
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    arrays = _arrays(text)
    rows = np.concatenate([_points_about(arrays, 500, 47, 1.0), np.full((500, 1), 0.4, f32)], axis=1)
    _, want_feat = cr.brute_force(arrays, rows)
    raw = _scene(text)
    try:
        d_rows = torch.from_numpy(rows).to(DEV)
        hits = torch.empty((500, 6), dtype=torch.int32, device=DEV)
        feat = torch.empty((500, 8), dtype=torch.float32, device=DEV)
        m.closest_points(raw, d_rows, hits, feat)
        # the rows packed by hand: the restatement's points, the hit records' normals and kinds
        t, kind, _, nn = m.unpack_hits(hits)
        by_hand = m.pack_features(torch.from_numpy(want_feat[:, 0:3].copy()).to(DEV), nn, kind)
        dirs = m.cosine_directions(16, DEV)
        out = [torch.empty((500, 4), dtype=torch.float32, device=DEV) for _ in range(2)]
        mask = [torch.empty(500, dtype=torch.int64, device=DEV) for _ in range(2)]
        m.hemisphere_visibility(raw, feat, dirs, out[0], mask[0], radius=2.0)
        m.hemisphere_visibility(raw, by_hand, dirs, out[1], mask[1], radius=2.0)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert torch.equal(feat, by_hand) and torch.equal(mask[0], mask[1]) and np.array_equal(bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy()))
    hit = kind.cpu().numpy() != 0
    assert 50 < hit.sum() < 500 and len(set(mask[0].cpu().numpy()[hit].tolist())) > 3 and bool(torch.all(out[0][torch.from_numpy(~hit).to(DEV)] == 0))


# ---- 5. after updates in place; another stream ------------------------------------------------------------------------------------------
def test_query_follows_geometry_updated_in_place_and_runs_on_another_stream():
    text = light_scenes.scene("spheres_planes", 3, "mixed")
    moved = text.replace("sphere 0.9 -0.2 -2.6 0.6", "sphere 0.3 0.4 -2.4 0.7")
    assert moved != text
    arrays = _arrays(moved)
    rows = np.concatenate([_points_about(arrays, 600, 48, 1.0), np.full((600, 1), INF, f32)], axis=1)
    raw = _scene(text)
    try:
        before, _ = _query(raw, rows)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.closest_points(raw, torch.from_numpy(rows).to(DEV), torch.empty((600, 6), dtype=torch.int32, device=DEV))
        assert e.value.status == 6 and b"mirt_closest_points" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        hits, feat = _assert_equals_brute_force(raw, arrays, rows)
        on_stream, feat_s = _query(raw, rows, stream=torch.cuda.Stream())
    finally:
        raw.close()
    fresh = _scene(moved)
    try:
        fresh_hits, fresh_feat = _query(fresh, rows)
    finally:
        fresh.close()
    assert np.array_equal(hits, fresh_hits) and np.array_equal(bits(feat), bits(fresh_feat)) and not np.array_equal(hits, before)
    assert np.array_equal(on_stream, hits) and np.array_equal(bits(feat_s), bits(feat))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n = 8
        Q = torch.zeros((4 * n, 4), dtype=torch.float32, device=DEV)
        Hh = torch.full((4 * n, 6), -7, dtype=torch.int32, device=DEV)
        F = torch.full((4 * n, 8), -7.0, dtype=torch.float32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.closest_points(raw, Q[:n], Hh[:n], F[:n])
        assert e.value.status == 6 and b"mirt_closest_points" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        L = closest.lib()
        pQ, pH, pF = Q.data_ptr(), Hh.data_ptr(), F.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(q=pQ, count=n, h=pH, f=pF, flags=0):
            return L.mirt_closest_points(raw._h, vp(q), count, vp(h), vp(f), flags, None)

        def refused(**kw):
            rc = call(**kw)
            return rc == 3 and b"mirt_closest_points" in m.lib().mirt_last_error()

        assert refused(count=-1)
        for flags in (1, 2, 0x80000000):
            assert refused(flags=flags)
        assert refused(q=0) and refused(h=0) and refused(q=0, h=0, f=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(h=pH + 2) and refused(f=pF + 8) and refused(f=pF + 4)
        assert refused(h=pQ) and refused(h=pQ + 16 * n - 4) and refused(q=pH + 24 * n - 16, h=pH)       # hits over the points
        assert refused(f=pQ) and refused(f=pQ + 16 * n - 16) and refused(q=pF + 32 * n - 16, f=pF)     # features over the points
        assert refused(f=pH) and refused(f=pH + 16) and refused(h=pF + 32 * n - 8)                     # features over the hits
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(F == -7.0))      # nothing ran
        assert call(count=0) == 0 and call(q=0, count=0, h=0, f=0) == 0
        m.closest_points(raw, Q[:0], Hh[:0], F[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(F == -7.0))
        # adjacent is not overlapping; the features are optional; d_hits needs 4-byte alignment only
        assert call(h=pQ + 16 * n) == 0 and call(f=pQ + 16 * n) == 0 and call(f=0) == 0 and call(h=pH + 4) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh[:n, 1] == 0)) and bool(torch.all(F[:n] == 0))      # rows of zeros have R = 0: misses
    finally:
        raw.close()

"""Box overlap queries on the GPU (include_ext/mirt_overlap.h: mirt_overlap_boxes; overlap.overlap_boxes, count_overlaps,
occupancy_grid).  The yardstick is tests/overlap_ref.py, the numpy restatement of the header as a brute force over every candidate:
records, counts and feature rows are compared on bit patterns on every row, whatever the scene's tree makes the kernel visit.  The
inputs are those tests/test_overlap_abi.py checks the restatement on."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import overlap
import overlap_ref as ovr
from test_gpu_contacts import _same, _scene      # (a built scene from its text; every row against a reference's records, counts, features)
from test_overlap_abi import CASES, CHOSEN_ROWS, MOVED, VOXEL_BOX, reference
from test_gpu_visibility import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32


def _query(raw, rows, k, want_counts=True, want_features=True, any_overlap=False, stream=None):
    """mirt_overlap_boxes on the rows (numpy [n, 8]): (hits uint32 [n, k, 6], counts uint32 [n] or None, features float32 [n, k, 8] or
    None); the row after the last of every output keeps its sentinel."""
    n = len(rows)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    hits = torch.full((n + 1, k, 6), -7, dtype=torch.int32, device=DEV) if k else None
    counts = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV) if want_counts else None
    feat = torch.full((n + 1, k, 8), -7.0, dtype=torch.float32, device=DEV) if want_features and k else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.overlap_boxes(raw, d_rows, hits[:n] if k else None, counts[:n] if want_counts else None, feat[:n] if feat is not None else None,
                    any_overlap=any_overlap, stream=stream)
    torch.cuda.synchronize()
    assert hits is None or bool(torch.all(hits[n] == -7))
    assert counts is None or int(counts[n]) == -7
    assert feat is None or bool(torch.all(feat[n] == -7.0))
    return (hits[:n].cpu().numpy().view(u32) if k else np.zeros((n, 0, 6), u32), counts[:n].cpu().numpy().view(u32) if want_counts else None,
            feat[:n].cpu().numpy() if feat is not None else None)


def _assert_equals_reference(raw, rows, k, want):
    """With counts and features, without counts, without features; with k = 0 the any flag against count > 0."""
    hits, counts, feat = _query(raw, rows, k)
    _same(hits, counts, feat, want, rows)
    if k:
        only, none, feat2 = _query(raw, rows, k, want_counts=False)
        assert none is None
        _same(only, None, feat2, want, rows)
        plain, counts2, none = _query(raw, rows, k, want_features=False)
        assert none is None and np.array_equal(plain, hits) and np.array_equal(counts2, counts)
        bare, _, _ = _query(raw, rows, k, want_counts=False, want_features=False)
        assert np.array_equal(bare, hits)
    else:
        _, some, _ = _query(raw, rows, 0, any_overlap=True)
        assert np.array_equal(some, (want[1] > 0).astype(u32))
    return hits, counts, feat


# ---- 1. scenes against the brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 4, 5, 8])
def test_dense_scene_equals_the_brute_force(k):
    text, rows = CASES["dense"]()
    raw = _scene(text)
    try:
        hits, counts, feat = _assert_equals_reference(raw, rows, k, reference("dense", k))
        if k == 0:
            d_rows = torch.from_numpy(rows).to(DEV)
            assert np.array_equal(m.count_overlaps(raw, d_rows).cpu().numpy().view(u32), counts)
            assert np.array_equal(m.count_overlaps(raw, d_rows, any_overlap=True).cpu().numpy().view(u32), (counts > 0).astype(u32))
    finally:
        raw.close()
    if k == 8:
        assert set(hits[:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3} and np.mean(counts > 8) > 0.1
        t, kind, pid, nn = m.unpack_hits(torch.from_numpy(hits.view(np.int32)).reshape(-1, 6))
        assert np.array_equal(t.numpy().view(u32), hits[:, :, 0].reshape(-1)) and np.array_equal(nn.numpy(), feat[:, :, 4:7].reshape(-1, 3))


@pytest.mark.parametrize("name", ["single_sphere", "single_triangle", "empty", "plane_only"])
def test_smallest_scenes(name):
    text, rows = CASES[name]()
    raw = _scene(text)
    try:
        for k in (0, 1, 4):
            hits, counts, _ = _assert_equals_reference(raw, rows, k, reference(name, k))
    finally:
        raw.close()
    assert set(hits[:, :, 1].reshape(-1).tolist()) == {"single_sphere": {0, 1}, "single_triangle": {0, 2}, "empty": {0}, "plane_only": {0, 3}}[name]
    assert set(counts.tolist()) == ({0} if name == "empty" else {0, 1})


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, rows = CASES["deep_stack"]()
    want = reference("deep_stack", 8)
    raw = _scene(text)
    try:
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            raw.set_option("stack_lds_depth", depth)
        hits, counts, feat = _query(raw, rows, 8)
        _same(hits, counts, feat, want, rows)
        _, only, _ = _query(raw, rows, 0)
        _, some, _ = _query(raw, rows, 0, any_overlap=True)
    finally:
        raw.close()
    assert counts.max() > 500 and np.array_equal(only, counts) and np.array_equal(some, (counts > 0).astype(u32))
    assert len(set(hits[:, :, 2].reshape(-1).tolist())) > 10


@pytest.mark.parametrize("offset", [1000.0, 100000.0])
def test_far_from_origin_and_touching_rows(offset):
    """Far from the origin, boxes whose face lies exactly on a plane of a sphere's float32 box and boxes one float32 step beyond it:
    the rows of which the CPU walk without the slack loses 17."""
    name = "far_1e3" if offset == 1000.0 else "far_1e5"
    text, rows = CASES[name]()
    raw = _scene(text)
    try:
        for k in (0, 4):
            hits, counts, _ = _assert_equals_reference(raw, rows, k, reference(name, k))
    finally:
        raw.close()
    assert np.count_nonzero(counts) > 300 and np.count_nonzero(counts == 0) > 300


# ---- 2. row counts ------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_a_wave_a_block_and_a_grid():
    text, base = CASES["mixed"]()
    want = reference("mixed", 4)
    assert set(want[0][:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}
    raw = _scene(text)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257):
            hits, counts, feat = _query(raw, base[:n], 4)
            _same(hits, counts, feat, tuple(w[:n] for w in want), base[:n])
        # more rows than a grid's worth of lanes: every lane takes a second row
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37
        reps = -(-n // 4096)
        tiled = tuple(np.tile(w, (reps,) + (1,) * (w.ndim - 1))[:n] for w in want)
        rows = np.tile(base, (reps, 1))[:n]
        hits, counts, feat = _query(raw, rows, 4)
        _same(hits, counts, feat, tiled)
        _, only, _ = _query(raw, rows, 0)
        _, some, _ = _query(raw, rows, 0, any_overlap=True)
        assert np.array_equal(only, tiled[1]) and np.array_equal(some, (tiled[1] > 0).astype(u32))
    finally:
        raw.close()


# ---- 3. chosen rows -------------------------------------------------------------------------------------------------------------------
def test_chosen_rows():
    """Dyadic coordinates: a box face exactly on a triangle's vertex, on its edge, in its plane, on a sphere's pole, on a plane; a
    box strictly inside a sphere (not counted) and one holding a sphere (counted); a box enclosing a whole triangle; point boxes on
    surfaces; a triangle without area met as a segment, and one whose dist is a NaN; rows with lo > hi, a NaN, an infinity."""
    text, rows = CASES["chosen"]()
    n = len(CHOSEN_ROWS)
    raw = _scene(text)
    try:
        for k in (8, 4, 2, 1, 0):
            hits, counts, feat = _assert_equals_reference(raw, rows, k, reference("chosen", k))
            assert counts[:n].tolist() == [r[2] for r in CHOSEN_ROWS] and np.all(counts[n:] == 0)
            if k == 8:
                h8, f8 = hits, feat
            if k == 1:
                assert tuple(hits[0, 0, 1:3].tolist()) == (2, 0)      # of the twins the lower id
    finally:
        raw.close()
    for r in (0, 1, 2, 8, 9):
        assert [tuple(x) for x in h8[r, :2, 1:3].tolist()] == [(2, 0), (2, 1)] and np.all(h8[r, 2:] == ovr.MISS)
    assert np.all(h8[6] == ovr.MISS) and np.all(f8[6] == 0) and np.all(h8[15] == ovr.MISS)
    assert np.all(h8[n:] == ovr.MISS) and np.all(f8[n:] == 0)
    assert np.array_equal(f8[3, 0], np.array([0, 0, -3, 1, 0, 0, 1, 0], f32))


# ---- 4. a voxel grid ------------------------------------------------------------------------------------------------------------------
def test_occupancy_grid_equals_the_reference_and_a_shared_face_marks_both_neighbours():
    text, rows = CASES["voxels"]()
    _, counts, _ = reference("voxels", 0)
    want = (counts > 0).reshape(16, 16, 16)
    raw = _scene(text)
    try:
        grid = m.occupancy_grid(raw, *VOXEL_BOX)
        assert grid.dtype == torch.bool and tuple(grid.shape) == (16, 16, 16) and grid.device.type == "cuda"
        assert np.array_equal(grid.cpu().numpy(), want)
        on_stream = m.occupancy_grid(raw, *VOXEL_BOX, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        assert np.array_equal(on_stream.cpu().numpy(), want)
        got, got_counts, _ = _query(raw, rows, 2)
        _same(got, got_counts, None, reference("voxels", 2), rows)
    finally:
        raw.close()
    assert want[9, 8, 7] and want[10, 8, 7]                                            # the triangle in z = 0.5, between layers 9 and 10
    assert np.all(want[:, 1, :]) and np.all(want[:, 2, :]) and not np.any(want[:, 0, :])      # the plane y = -1.5, between rows 1 and 2


# ---- 5. into the surface-point queries; after updates in place; another stream ---------------------------------------------------------
def test_feature_rows_feed_hemisphere_visibility_without_a_copy():
    text, rows = CASES["dense"]()
    n = len(rows)
    want_hits, _, want_feat = reference("dense", 1)
    raw = _scene(text)
    try:
        d_rows = torch.from_numpy(rows).to(DEV)
        h1 = torch.empty((n, 1, 6), dtype=torch.int32, device=DEV)
        f1 = torch.empty((n, 1, 8), dtype=torch.float32, device=DEV)
        m.overlap_boxes(raw, d_rows, h1, None, f1)
        dirs = m.cosine_directions(16, DEV)
        out = [torch.empty((n, 4), dtype=torch.float32, device=DEV) for _ in range(2)]
        mask = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(2)]
        m.hemisphere_visibility(raw, f1.view(n, 8), dirs, out[0], mask[0], radius=2.0)      # (a view: the rows as the query wrote them)
        m.hemisphere_visibility(raw, torch.from_numpy(np.ascontiguousarray(want_feat[:, 0])).to(DEV), dirs, out[1], mask[1], radius=2.0)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert f1.view(n, 8).data_ptr() == f1.data_ptr()
    assert np.array_equal(bits(f1.cpu().numpy()[:, 0]), bits(want_feat[:, 0])) and torch.equal(mask[0], mask[1])
    assert np.array_equal(bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy()))
    hit = want_hits[:, 0, 1] != 0
    assert 500 < hit.sum() < n and len(set(mask[0].cpu().numpy()[hit].tolist())) > 3


def test_query_follows_geometry_updated_in_place_and_runs_on_another_stream():
    moved, rows = CASES["moved"]()
    text = moved.replace(MOVED[1], MOVED[0])
    assert text != moved
    raw = _scene(text)
    try:
        before, _, _ = _query(raw, rows, 4)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.count_overlaps(raw, torch.from_numpy(rows).to(DEV))
        assert e.value.status == 6 and b"mirt_overlap_boxes" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        hits, counts, feat = _assert_equals_reference(raw, rows, 4, reference("moved", 4))
        _assert_equals_reference(raw, rows, 0, reference("moved", 0))
        on_stream, counts_s, feat_s = _query(raw, rows, 4, stream=torch.cuda.Stream())
    finally:
        raw.close()
    assert not np.array_equal(hits, before)
    assert np.array_equal(on_stream, hits) and np.array_equal(counts_s, counts) and np.array_equal(bits(feat_s), bits(feat))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    import light_scenes
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n, k = 8, 2
        Q = torch.zeros((16 * n, 8), dtype=torch.float32, device=DEV)
        Q[:, 0:3] = 1.0      # (lo > hi: rows that are not live)
        Hh = torch.full((4 * n, k, 6), -7, dtype=torch.int32, device=DEV)
        Cn = torch.full((16 * n,), -7, dtype=torch.int32, device=DEV)
        F = torch.full((4 * n, k, 8), -7.0, dtype=torch.float32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.overlap_boxes(raw, Q[:n], Hh[:n], Cn[:n], F[:n])
        assert e.value.status == 6 and b"mirt_overlap_boxes" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        L = overlap.lib()
        pQ, pH, pC, pF = Q.data_ptr(), Hh.data_ptr(), Cn.data_ptr(), F.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(q=pQ, count=n, kk=k, h=pH, c=pC, f=pF, flags=0):
            return L.mirt_overlap_boxes(raw._h, vp(q), count, kk, vp(h), vp(c), vp(f), flags, None)

        def refused(**kw):
            rc = call(**kw)
            return rc == 3 and b"mirt_overlap_boxes" in m.lib().mirt_last_error()

        assert refused(count=-1) and refused(kk=-1) and refused(kk=9)
        for flags in (2, 3, 0x80000000):
            assert refused(flags=flags) and refused(flags=flags, kk=0, h=0, f=0)
        assert refused(flags=1) and refused(flags=1, kk=1) and refused(flags=1, kk=0, h=0, f=0, c=0)      # the any flag: k == 0, counts
        assert refused(q=0) and refused(h=0) and refused(kk=0, h=0, c=0, f=0) and refused(q=0, h=0, c=0, f=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(h=pH + 2) and refused(c=pC + 2) and refused(f=pF + 8) and refused(f=pF + 4)
        nq, nh, nf = 32 * n, 24 * n * k, 32 * n * k
        assert refused(h=pQ) and refused(h=pQ + nq - 4) and refused(q=pH + nh - 16, h=pH)          # hits over the boxes
        assert refused(c=pQ) and refused(c=pQ + nq - 4) and refused(q=pC + 4 * n - 16, c=pC)       # counts over the boxes
        assert refused(f=pQ) and refused(f=pQ + nq - 16) and refused(q=pF + nf - 16, f=pF)         # features over the boxes
        assert refused(c=pH) and refused(c=pH + nh - 4) and refused(h=pC + 4 * n - 4)              # counts over the hits
        assert refused(f=pH) and refused(f=pH + 16) and refused(h=pF + nf - 8)                     # features over the hits
        assert refused(f=pC) and refused(c=pF + nf - 4) and refused(c=pF + 16)                     # features over the counts
        assert refused(kk=0, h=0, f=0, c=pQ + 16) and refused(flags=1, kk=0, h=0, f=0, c=pQ + 16)  # a count-only call's counts over the boxes
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(Cn == -7)) and bool(torch.all(F == -7.0))      # nothing ran
        assert call(count=0) == 0 and call(q=0, count=0, h=0, c=0, f=0) == 0 and call(count=0, kk=0, h=0) == 0 and call(count=0, kk=0, flags=1) == 0
        m.overlap_boxes(raw, Q[:0], Hh[:0], Cn[:0], F[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(Cn == -7)) and bool(torch.all(F == -7.0))
        # adjacent is not overlapping; counts and features are optional; with k = 0 the record and feature pointers are not ranges
        assert call(h=pQ + nq) == 0 and call(f=pQ + nq) == 0 and call(c=pQ + nq) == 0 and call(c=0) == 0 and call(f=0) == 0
        assert call(h=pH + 4) == 0 and call(kk=0, h=pQ, f=pQ) == 0 and call(kk=0, h=pQ, f=pQ, flags=1) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh[:n, :, 1] == 0)) and bool(torch.all(Cn[:n] == 0)) and bool(torch.all(F[:n] == 0))      # rows with lo > hi: misses
    finally:
        raw.close()

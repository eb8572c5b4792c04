"""Contact queries on the GPU (include_ext/mirt_contacts.h: mirt_closest_points_multi; contacts.closest_points_multi,
count_within).  The yardstick is tests/contacts_ref.py, the numpy restatement of the header as a brute force over every candidate:
records, counts and feature rows are compared on bit patterns on every row, whatever the scene's tree makes the kernel visit.  The
inputs are those tests/test_contacts_abi.py checks the restatement on."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import contacts
import contacts_ref as kr
import edge_scenes
import light_scenes
from test_closest_abi import _points_about, with_tight_radii
from test_contacts_abi import CASES, _arrays, reference, shuffled
from test_gpu_visibility import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32
INF = float("inf")
NAN = float("nan")


def _scene(text, **options):
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _query(raw, rows, k, want_counts=True, want_features=True, stream=None):
    """mirt_closest_points_multi on the rows (numpy [n, 4]): (hits uint32 [n, k, 6], counts uint32 [n] or None, features float32
    [n, k, 8] or None); the row after the last of every output keeps its sentinel."""
    n = len(rows)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    hits = torch.full((n + 1, k, 6), -7, dtype=torch.int32, device=DEV) if k else None
    counts = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV) if want_counts else None
    feat = torch.full((n + 1, k, 8), -7.0, dtype=torch.float32, device=DEV) if want_features and k else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.closest_points_multi(raw, d_rows, hits[:n] if k else None, counts[:n] if want_counts else None, feat[:n] if feat is not None else None, stream=stream)
    torch.cuda.synchronize()
    assert hits is None or bool(torch.all(hits[n] == -7))
    assert counts is None or int(counts[n]) == -7
    assert feat is None or bool(torch.all(feat[n] == -7.0))
    return (hits[:n].cpu().numpy().view(u32) if k else np.zeros((n, 0, 6), u32), counts[:n].cpu().numpy().view(u32) if want_counts else None,
            feat[:n].cpu().numpy() if feat is not None else None)


def _hit_bits(h):
    """MirtHit words with the float columns' NaNs folded."""
    out = h.copy()
    out[..., 0] = bits(h[..., 0].view(f32))
    out[..., 3:6] = bits(h[..., 3:6].view(f32))
    return out


def _same(hits, counts, feat, want, rows=None):
    """Every row against the reference's (hits, counts, features); counts / feat None: not asked for."""
    want_hits, want_counts, want_feat = want
    n = len(hits)
    bad = np.any((_hit_bits(hits) != _hit_bits(want_hits)).reshape(n, -1), axis=1)
    if counts is not None:
        bad |= counts != want_counts
    if feat is not None:
        bad |= np.any((bits(feat) != bits(want_feat)).reshape(n, -1), axis=1)
    bad = np.flatnonzero(bad)
    assert len(bad) == 0, (len(bad), bad[:5], None if rows is None else rows[bad[:5]], hits[bad[:3]], want_hits[bad[:3]],
                           None if counts is None else (counts[bad[:5]], want_counts[bad[:5]]))


def _assert_equals_reference(raw, rows, k, want):
    """With counts and features, without counts (the other bound rule: identical records), without features."""
    hits, counts, feat = _query(raw, rows, k)
    _same(hits, counts, feat, want, rows)
    if k:
        only, none, feat2 = _query(raw, rows, k, want_counts=False)
        assert none is None
        _same(only, None, feat2, want, rows)
        assert np.array_equal(only, hits)
        plain, counts2, none = _query(raw, rows, k, want_features=False)
        assert none is None and np.array_equal(plain, hits) and np.array_equal(counts2, counts)
        bare, _, _ = _query(raw, rows, k, want_counts=False, want_features=False)
        assert np.array_equal(bare, hits)
    return hits, counts, feat


# ---- 1. scenes against the brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 4, 5, 8])
def test_dense_scene_equals_the_brute_force(k):
    text, rows = CASES["dense"]()
    raw = _scene(text)
    try:
        hits, counts, feat = _assert_equals_reference(raw, rows, k, reference("dense", k))
        if k == 0:
            assert np.array_equal(m.count_within(raw, torch.from_numpy(rows).to(DEV)).cpu().numpy().view(u32), counts)
    finally:
        raw.close()
    if k == 8:
        assert set(hits[:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}
        # api.unpack_hits reads the records of every row, flattened
        t, kind, pid, nn = m.unpack_hits(torch.from_numpy(hits.view(np.int32)).reshape(-1, 6))
        assert np.array_equal(t.numpy().view(u32), hits[:, :, 0].reshape(-1)) and np.array_equal(nn.numpy(), feat[:, :, 4:7].reshape(-1, 3))


@pytest.mark.parametrize("name", ["single_sphere", "single_triangle", "empty", "plane_only"])
def test_smallest_scenes(name):
    text = edge_scenes.ALL[name]()
    arrays = _arrays(text)
    q = np.random.default_rng(5).uniform(-3, 3, (100, 3)).astype(f32)
    q[:, 2] -= 2
    rows, _ = with_tight_radii(arrays, q)
    rows = shuffled(rows)
    raw = _scene(text)
    try:
        for k in (0, 1, 4):
            hits, counts, _ = _assert_equals_reference(raw, rows, k, kr.brute_force(arrays, rows, k))
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
        only, _, _ = _query(raw, rows, 8, want_counts=False, want_features=False)
    finally:
        raw.close()
    assert np.all(counts == 600) and np.array_equal(only, hits)
    assert len(set(hits[:, :, 2].reshape(-1).tolist())) > 10


@pytest.mark.parametrize("offset", [1000.0, 100000.0])
def test_far_from_origin_where_the_boxes_do_not_bound_the_distances(offset):
    """The scenes of the CPU slack test: without counts the shrinking bound rests on the header's slack."""
    name = "far_1e3" if offset == 1000.0 else "far_1e5"
    text, rows = CASES[name]()
    want = reference(name, 4)
    raw = _scene(text)
    try:
        only, none, feat = _query(raw, rows, 4, want_counts=False)
        _same(only, None, feat, want, rows)
        hits, counts, feat = _query(raw, rows, 4)
        _same(hits, counts, feat, want, rows)
    finally:
        raw.close()
    assert np.count_nonzero(hits[:, 0, 1] == 1) > 800 and np.count_nonzero(hits[:, 0, 1] == 0) > 700


# ---- 2. row counts ------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_a_wave_a_block_and_a_grid():
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    arrays = _arrays(text)
    base = np.concatenate([_points_about(arrays, 4096, 45, 1.0), np.random.default_rng(46).choice([0.2, 0.8, np.inf], (4096, 1)).astype(f32)], axis=1)
    want = kr.brute_force(arrays, base, 4)
    assert set(want[0][:257, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}
    raw = _scene(text)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257):
            hits, counts, feat = _query(raw, base[:n], 4)
            _same(hits, counts, feat, tuple(w[:n] for w in want), base[:n])
        # more rows than a grid's worth of lanes: every lane takes a second row
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37
        reps = -(-n // 4096)
        hits, counts, feat = _query(raw, np.tile(base, (reps, 1))[:n], 4)
        _same(hits, counts, feat, tuple(np.tile(w, (reps,) + (1,) * (w.ndim - 1))[:n] for w in want))
    finally:
        raw.close()


# ---- 3. chosen rows -------------------------------------------------------------------------------------------------------------------
CHOSEN = """png 8 8 chosen.png
sphere 0 0 -4 1
sphere 0 0 -4 1
xyz 0 0 3
xyz 1 0 4
xyz 0 1 4
tri 1 2 3
tri 1 2 3
plane 0 0 1 3
plane 0 0 1 3
"""


def test_chosen_rows():
    """Two identical spheres, triangles and planes, all six at distance exactly 3 from the origin."""
    arrays = _arrays(CHOSEN)
    assert len(arrays["spheres"]) == 2 and len(arrays["triangles"]) == 2 and len(arrays["planes"]) == 2
    ndead = 6
    rows = [(0, 0, 0, 4.0), (0, 0, 0, 3.0), (0, 0, 0, np.nextafter(f32(3), f32(4))), (0, 0, 0, INF), (0, 0, -4, 1.5), (0.25, 0.25, 0, 3.2)]
    rows += [(1, 1, 1, 0.0), (1, 1, 1, -1.0), (1, 1, 1, NAN), (NAN, 1, 1, INF), (1, INF, 1, INF), (1, 1, -INF, 5.0)]
    rows = np.array(rows, f32)
    raw = _scene(CHOSEN)
    try:
        for k in (8, 4, 1, 0):
            hits, counts, feat = _assert_equals_reference(raw, rows, k, kr.brute_force(arrays, rows, k))
            if k == 8:
                h8, f8 = hits, feat
            if k == 4:
                assert [tuple(r) for r in hits[0, :, 1:3].tolist()] == [(1, 0), (1, 1), (2, 0), (2, 1)]      # the list's last slots at a six-way tie
            if k == 1:
                assert tuple(hits[0, 0, 1:3].tolist()) == (1, 0)
            assert counts[:4].tolist() == [6, 0, 6, 6] and counts[-ndead:].tolist() == [0] * ndead
    finally:
        raw.close()
    t = h8[:, :, 0].view(f32)
    six = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]
    for r in (0, 2, 3):
        assert [tuple(x) for x in h8[r, :6, 1:3].tolist()] == six and np.all(t[r, :6] == 3) and np.all(h8[r, 6:] == kr.MISS)
        assert np.array_equal(f8[r, :4, 0:4], np.array([(0, 0, -3, 1)] * 2 + [(0, 0, 3, 1)] * 2, f32))
        assert np.all(f8[r, 4:6, 0:2] == 0) and np.all(np.abs(f8[r, 4:6, 2]) == 3) and np.all(f8[r, 4:6, 3] == 1)
        assert np.array_equal(h8[r, 0], h8[r, 1]) is False and np.array_equal(h8[r, 0, 3:6], h8[r, 1, 3:6])      # twins: the same record but for the id
    assert np.all(h8[1] == kr.MISS) and np.all(f8[1] == 0)                                                         # R = 3: dist < R admits none
    # at the spheres' centre, one unit from the planes as well: a four-way tie across two kinds
    assert [tuple(x) for x in h8[4, :4, 1:3].tolist()] == [(1, 0), (1, 1), (3, 0), (3, 1)] and np.all(t[4, :4] == 1) and np.all(h8[4, 4:] == kr.MISS)
    assert np.all(h8[-ndead:] == kr.MISS) and np.all(f8[-ndead:] == 0)


SIX = "png 8 8 six.png\n" + "".join("sphere %d %d %d 1\n" % c for c in [(2, 0, 0), (0, 2, 0), (0, 0, 2), (-2, 0, 0), (0, -2, 0), (0, 0, -2), (5, 5, 5)])


def test_spheres_at_one_distance_come_in_id_order_whatever_their_leaf_order():
    """Six spheres at distance exactly 1 from the origin, listed so that the tree's sorted leaves (the negative octants first) are
    not in file order: the tie is broken by the ids, which the kernel's keys hold only at capacity 8."""
    arrays = _arrays(SIX)
    rows = np.array([(0, 0, 0, 1.5), (0, 0, 0, INF), (0, 0, 0, 1.0), (0.5, 0, 0, 2.0), (0, 0, 0, 2.0)], f32)
    raw = _scene(SIX)
    try:
        for k in (1, 2, 3, 4, 5, 6, 8):
            hits, counts, _ = _assert_equals_reference(raw, rows, k, kr.brute_force(arrays, rows, k))
            assert hits[0, :, 2].tolist() == list(range(min(k, 6))) + [0] * max(k - 6, 0) and np.all(hits[0, :min(k, 6), 0].view(f32) == 1)
            assert counts.tolist() == [6, 7, 0, 6, 6]
    finally:
        raw.close()


# ---- 4. against mirt_closest_points; into the surface-point queries ------------------------------------------------------------------
def test_k1_is_closest_points_on_every_row_and_its_feature_rows_feed_hemisphere_visibility():
    text, rows = CASES["dense"]()
    n = len(rows)
    d_rows = torch.from_numpy(rows).to(DEV)
    raw = _scene(text)
    try:
        hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
        feat = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        m.closest_points(raw, d_rows, hits, feat)
        for want_counts in (True, False):
            h1, _, f1 = _query(raw, rows, 1, want_counts=want_counts)
            assert np.array_equal(h1[:, 0], hits.cpu().numpy().view(u32)) and np.array_equal(f1[:, 0].view(u32), feat.cpu().numpy().view(u32))
        # row i * k + 0 of a k = 4 call gives hemisphere_visibility what closest_points' row gives it
        h4 = torch.empty((n, 4, 6), dtype=torch.int32, device=DEV)
        f4 = torch.empty((n, 4, 8), dtype=torch.float32, device=DEV)
        m.closest_points_multi(raw, d_rows, h4, None, f4)
        first = f4[:, 0].contiguous()
        dirs = m.cosine_directions(16, DEV)
        out = [torch.empty((n, 4), dtype=torch.float32, device=DEV) for _ in range(2)]
        mask = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(2)]
        m.hemisphere_visibility(raw, first, dirs, out[0], mask[0], radius=2.0)
        m.hemisphere_visibility(raw, feat, dirs, out[1], mask[1], radius=2.0)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert torch.equal(first.view(torch.int32), feat.view(torch.int32)) and torch.equal(mask[0], mask[1])
    assert np.array_equal(bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy()))
    hit = hits[:, 1].cpu().numpy() != 0
    assert 500 < hit.sum() < n and len(set(mask[0].cpu().numpy()[hit].tolist())) > 3


# ---- 5. after updates in place; another stream ------------------------------------------------------------------------------------------
def test_query_follows_geometry_updated_in_place_and_runs_on_another_stream():
    text = light_scenes.scene("spheres_planes", 3, "mixed")
    moved = text.replace("sphere 0.9 -0.2 -2.6 0.6", "sphere 0.3 0.4 -2.4 0.7")
    assert moved != text
    arrays = _arrays(moved)
    rows = np.concatenate([_points_about(arrays, 600, 48, 1.0), np.full((600, 1), 1.5, f32)], axis=1)
    raw = _scene(text)
    try:
        before, _, _ = _query(raw, rows, 4)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.closest_points_multi(raw, torch.from_numpy(rows).to(DEV), torch.empty((600, 4, 6), dtype=torch.int32, device=DEV))
        assert e.value.status == 6 and b"mirt_closest_points_multi" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        hits, counts, feat = _assert_equals_reference(raw, rows, 4, kr.brute_force(arrays, rows, 4))
        on_stream, counts_s, feat_s = _query(raw, rows, 4, stream=torch.cuda.Stream())
    finally:
        raw.close()
    assert not np.array_equal(hits, before)
    assert np.array_equal(on_stream, hits) and np.array_equal(counts_s, counts) and np.array_equal(bits(feat_s), bits(feat))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n, k = 8, 2
        Q = torch.zeros((16 * n, 4), dtype=torch.float32, device=DEV)
        Hh = torch.full((4 * n, k, 6), -7, dtype=torch.int32, device=DEV)
        Cn = torch.full((16 * n,), -7, dtype=torch.int32, device=DEV)
        F = torch.full((4 * n, k, 8), -7.0, dtype=torch.float32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.closest_points_multi(raw, Q[:n], Hh[:n], Cn[:n], F[:n])
        assert e.value.status == 6 and b"mirt_closest_points_multi" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        L = contacts.lib()
        pQ, pH, pC, pF = Q.data_ptr(), Hh.data_ptr(), Cn.data_ptr(), F.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(q=pQ, count=n, kk=k, h=pH, c=pC, f=pF, flags=0):
            return L.mirt_closest_points_multi(raw._h, vp(q), count, kk, vp(h), vp(c), vp(f), flags, None)

        def refused(**kw):
            rc = call(**kw)
            return rc == 3 and b"mirt_closest_points_multi" in m.lib().mirt_last_error()

        assert refused(count=-1) and refused(kk=-1) and refused(kk=9)
        for flags in (1, 2, 0x80000000):
            assert refused(flags=flags)
        assert refused(q=0) and refused(h=0) and refused(kk=0, h=0, c=0, f=0) and refused(q=0, h=0, c=0, f=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(h=pH + 2) and refused(c=pC + 2) and refused(f=pF + 8) and refused(f=pF + 4)
        nh, nf = 24 * n * k, 32 * n * k
        assert refused(h=pQ) and refused(h=pQ + 16 * n - 4) and refused(q=pH + nh - 16, h=pH)          # hits over the points
        assert refused(c=pQ) and refused(c=pQ + 16 * n - 4) and refused(q=pC + 4 * n - 16, c=pC)       # counts over the points
        assert refused(f=pQ) and refused(f=pQ + 16 * n - 16) and refused(q=pF + nf - 16, f=pF)         # features over the points
        assert refused(c=pH) and refused(c=pH + nh - 4) and refused(h=pC + 4 * n - 4)                  # counts over the hits
        assert refused(f=pH) and refused(f=pH + 16) and refused(h=pF + nf - 8)                         # features over the hits
        assert refused(f=pC) and refused(c=pF + nf - 4) and refused(c=pF + 16)                         # features over the counts
        assert refused(kk=0, h=0, f=0, c=pQ + 16)                                                      # a count-only call's counts over the points
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(Cn == -7)) and bool(torch.all(F == -7.0))      # nothing ran
        assert call(count=0) == 0 and call(q=0, count=0, h=0, c=0, f=0) == 0 and call(count=0, kk=0, h=0) == 0
        m.closest_points_multi(raw, Q[:0], Hh[:0], Cn[:0], F[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(Cn == -7)) and bool(torch.all(F == -7.0))
        # adjacent is not overlapping; counts and features are optional; with k = 0 the record and feature pointers are not ranges
        assert call(h=pQ + 16 * n) == 0 and call(f=pQ + 16 * n) == 0 and call(c=pQ + 16 * n) == 0 and call(c=0) == 0 and call(f=0) == 0
        assert call(h=pH + 4) == 0 and call(kk=0, h=pQ, f=pQ) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh[:n, :, 1] == 0)) and bool(torch.all(Cn[:n] == 0)) and bool(torch.all(F[:n] == 0))      # rows of zeros have R = 0: misses
    finally:
        raw.close()

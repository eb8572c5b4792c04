"""Sphere casts on the GPU (include_ext/mirt_spherecast.h: mirt_cast_spheres; spherecast.cast_spheres).  The yardstick is
tests/spherecast_ref.py, the numpy restatement of the header as a brute force over every candidate: hits and feature rows are
compared on bit patterns, whatever the scene's tree makes the kernel visit.  The inputs are those of tests/test_spherecast_abi.py,
on which the header's pruning rule is checked on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import spherecast
import light_scenes
import spherecast_ref as sr
from test_gpu_visibility import bits
from test_spherecast_abi import UPDATE_MOVED, case, chosen_groups, reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
u32 = np.uint32


def _scene(text, **options):
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _cast(raw, rows, want_features=True, any_hit=False, stream=None):
    """mirt_cast_spheres on the rows (numpy [n, 8]): (hits uint32 [n, 6], features float32 [n, 8] or None); the row after the last
    keeps its sentinel."""
    n = len(rows)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, f32)).to(DEV)
    hits = torch.full((n + 1, 6), -7, dtype=torch.int32, device=DEV)
    feat = torch.full((n + 1, 8), -7.0, dtype=torch.float32, device=DEV) if want_features else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.cast_spheres(raw, d_rows, hits[:n], feat[:n] if want_features else None, any_hit=any_hit, stream=stream)
    torch.cuda.synchronize()
    assert bool(torch.all(hits[n] == -7)) and (feat is None or bool(torch.all(feat[n] == -7.0)))
    return hits[:n].cpu().numpy().view(u32), (feat[:n].cpu().numpy() if want_features else None)


def _hit_bits(h):
    """MirtHit words with the float columns' NaNs folded."""
    out = h.copy()
    out[:, 0] = bits(h[:, 0].view(f32))
    out[:, 3:6] = bits(h[:, 3:6].view(f32))
    return out


def _assert_equals(hits, feat, want_hits, want_feat, rows):
    bad = np.flatnonzero(np.any(_hit_bits(hits) != _hit_bits(want_hits), axis=1) | np.any(bits(feat) != bits(want_feat), axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:5]], hits[bad[:5]], want_hits[bad[:5]])


def _assert_equals_brute_force(raw, name, rows=None):
    _, _, all_rows = case(name)
    want_hits, want_feat, _ = reference(name)
    rows = all_rows if rows is None else rows
    hits, feat = _cast(raw, rows)
    _assert_equals(hits, feat, want_hits[:len(rows)], want_feat[:len(rows)], rows)
    only_hits, none = _cast(raw, rows, want_features=False)      # d_features == NULL: the same hits
    assert none is None and np.array_equal(only_hits, hits)
    return hits, feat


# ---- 1. scenes against the brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_planes"])
def test_mixed_scenes_equal_the_brute_force(name):
    raw = _scene(case(name)[0])
    try:
        hits, feat = _assert_equals_brute_force(raw, name)
    finally:
        raw.close()
    t, kind = hits[:, 0].view(f32), hits[:, 1]
    want = {0, 1, 2, 3} if name.endswith("_planes") else {0, 1, 2}
    assert set(kind.tolist()) == want and set(kind[t == 0].tolist()) == want - {0} and set(kind[t > 0].tolist()) == want - {0}
    hit = kind != 0
    assert np.all(feat[hit, 3] == 1) and np.all(feat[~hit] == 0) and np.all(hits[~hit, 0] == f32(-1).view(u32))
    # api.unpack_hits reads the records unchanged
    tt, kk, pid, nn = m.unpack_hits(torch.from_numpy(hits.view(np.int32)))
    assert np.array_equal(tt.numpy().view(u32), hits[:, 0]) and np.array_equal(kk.numpy().view(u32), hits[:, 1])
    assert np.array_equal(bits(nn.numpy()), bits(feat[:, 4:7]))


@pytest.mark.parametrize("name", ["single_sphere", "single_triangle", "empty", "plane_only"])
def test_smallest_scenes(name):
    raw = _scene(case(name)[0])
    try:
        hits, _ = _assert_equals_brute_force(raw, name)
    finally:
        raw.close()
    assert set(hits[:, 1].tolist()) == {"single_sphere": {0, 1}, "single_triangle": {0, 2}, "empty": {0}, "plane_only": {0, 3}}[name]


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, _, rows = case("deep_stack")
    want_hits, want_feat, _ = reference("deep_stack")
    raw = _scene(text)
    try:
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            raw.set_option("stack_lds_depth", depth)
        hits, feat = _cast(raw, rows)
        any_hits, any_feat = _cast(raw, rows, any_hit=True)
    finally:
        raw.close()
    _assert_equals(hits, feat, want_hits, want_feat, rows)
    assert len(set(hits[:, 2].tolist())) > 10
    assert len(sr.any_hit_is_valid(case("deep_stack")[1], rows, any_hits, any_feat, reference("deep_stack")[2])) == 0


def test_casts_along_triangle_edges():
    """Paths exactly along an edge and turned off it by 1e-7 to 0.1, where an edge piece's A is zero or small and its t
    ill-conditioned: the kernel gives the brute force's bits there too (the CPU walk of tests/test_spherecast_abi.py likewise)."""
    raw = _scene(case("along_edges")[0])
    try:
        hits, _ = _assert_equals_brute_force(raw, "along_edges")
    finally:
        raw.close()
    assert np.count_nonzero(hits[:, 1] == 2) > 300


@pytest.mark.parametrize("name", ["far_1e3", "far_1e5"])
def test_far_from_origin_where_the_boxes_do_not_bound_the_contacts(name):
    """The scenes of the CPU slack test (tests/test_spherecast_abi.py): a kernel that pruned at its best t without the header's
    slacks would lose rows here."""
    raw = _scene(case(name)[0])
    try:
        hits, _ = _assert_equals_brute_force(raw, name)
    finally:
        raw.close()
    assert np.count_nonzero(hits[:, 1] == 1) > 500 and np.count_nonzero(hits[:, 1] == 0) > 300


# ---- 2. row counts ------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_a_wave_a_block_and_a_grid():
    text, _, base = case("row_counts")
    want_hits, want_feat, _ = reference("row_counts")
    assert set(want_hits[:257, 1].tolist()) == {0, 1, 2, 3}
    raw = _scene(text)
    try:
        for n in (1, 63, 64, 65, 255, 256, 257):
            hits, feat = _cast(raw, base[:n])
            assert np.array_equal(_hit_bits(hits), _hit_bits(want_hits[:n])) and np.array_equal(bits(feat), bits(want_feat[:n])), n
        # more rows than a grid's worth of lanes: every lane takes a second row
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = cus * 8 * 256 + 4096 + 37
        reps = -(-n // 4096)
        for any_hit in (False, True):
            hits, feat = _cast(raw, np.tile(base, (reps, 1))[:n], any_hit=any_hit)
            if any_hit:
                assert np.array_equal(hits[:, 1] != 0, np.tile(want_hits[:, 1] != 0, reps)[:n])
            else:
                assert np.array_equal(_hit_bits(hits), _hit_bits(np.tile(want_hits, (reps, 1))[:n]))
                assert np.array_equal(bits(feat), bits(np.tile(want_feat, (reps, 1))[:n]))
    finally:
        raw.close()


# ---- 3. chosen rows -------------------------------------------------------------------------------------------------------------------
def test_chosen_rows():
    text, arrays, rows = case("chosen")
    _, _, (ts, tt, tp) = reference("chosen")
    raw = _scene(text)
    try:
        hits, feat = _assert_equals_brute_force(raw, "chosen")
    finally:
        raw.close()
    at, i = {}, 0
    for name, group in chosen_groups():
        at[name] = list(range(i, i + len(group)))
        i += len(group)
    t, kind, pid = hits[:, 0].view(f32), hits[:, 1].tolist(), hits[:, 2].tolist()
    P, nn = feat[:, 0:3], feat[:, 4:7]
    rec = lambda j: (float(t[j]), kind[j], pid[j])
    v = lambda *x: np.array(x, f32)
    # a ball of radius 0.5 dropped onto the first triangle: the face exactly, the edges and the vertices to rounding
    j = at["face"][0]
    assert rec(j) == (2.5, 2, 0) and np.array_equal(P[j], v(0.5, 0.5, 0)) and np.array_equal(nn[j], v(0, 0, 1))
    for j, p, off2 in zip(at["edges"], [(1, 0, 0), (0, 1, 0), (1, 1, 0)], [0.0625, 0.0625, 0.125]):      # (off2: the squared offset from the edge)
        assert kind[j] == 2 and pid[j] == 0 and np.allclose(P[j], p, atol=1e-6) and abs(t[j] - (3 - np.sqrt(0.25 - off2))) < 1e-6
    for j, p in zip(at["vertices"], [(0, 0, 0), (2, 0, 0), (0, 2, 0)]):
        assert kind[j] == 2 and pid[j] == 0 and np.array_equal(P[j], v(*p)) and abs(t[j] - (3 - np.sqrt(0.125))) < 1e-6
    # the big sphere: from inside moving out, from outside moving in, a near-tangent pass that touches and one that does not
    a, b, c, d, e = at["big_sphere"]
    assert rec(a) == (3.5, 1, 2) and np.array_equal(nn[a], v(-1, 0, 0)) and np.array_equal(P[a], v(4, 20, 0))
    assert rec(b) == (4.0, 1, 2) and np.array_equal(nn[b], v(0, 1, 0)) and rec(c) == (5.5, 1, 2) and np.array_equal(nn[c], v(0, 1, 0))
    assert kind[d] == 1 and pid[d] == 2 and 9 < t[d] < 10 and kind[e] == 0
    # the plane from above and from below; parallel to it, moving away from it: misses
    a, b, c, d, e = at["plane"]
    assert rec(a) == (9.0, 3, 0) and np.array_equal(nn[a], v(0, 1, 0)) and rec(b) == (9.0, 3, 0) and np.array_equal(nn[b], v(0, -1, 0))
    assert [kind[c], kind[d], kind[e]] == [0, 0, 0]
    # overlap at the start: t = 0 with each kind
    assert [rec(j) for j in at["overlap"]] == [(0.0, 2, 0), (0.0, 1, 0), (0.0, 3, 0), (0.0, 1, 2), (0.0, 2, 0)]
    # ties: the lower id of the twins; the sphere before the triangle at the same t
    assert [rec(j) for j in at["twins"]] == [(3.5, 1, 0), (1.75, 1, 0)]
    for j, tie in zip(at["kind_tie"], (3.5, 4.0)):
        assert ts[j, 3] == tt[j, 1] == tie and rec(j) == (tie, 1, 3)
    # the six equal spheres: all touched at the start, the lowest id wins whatever the leaf order
    a, b, c, d = at["six"]
    assert np.all(ts[a, 4:10] == 0) and rec(a) == (0.0, 1, 4) and rec(b) == (0.5, 1, 5) and rec(c) == (0.5, 1, 8) and rec(d) == (1.0, 1, 4)
    # the triangle without area is met as the segment it is
    assert [rec(j) for j in at["no_area"]] == [(2.5, 2, 2), (-1.0, 0, 0), (-1.0, 0, 0), (1.5, 2, 2), (3.0, 2, 2)]
    # the small triangle with a zero record normal has no face piece: nothing far above it, the ball dropped onto it meets its edges
    small = arrays["triangles"][4]
    assert np.all(small["nor"] == 0) and np.linalg.norm(np.cross(small["p1"] - small["p0"], small["p2"] - small["p0"])) > 0
    a, b, c, d = at["small"]
    assert [kind[a], kind[b], kind[d]] == [0, 0, 0] and kind[c] == 2 and pid[c] == 4 and abs(t[c] - 2.9) < 1e-5 and np.allclose(nn[c], (0, 0, 1), atol=1e-2)
    # tmax at the contact, one step above it, one step below it
    assert [kind[j] for j in at["tmax"]] == [0, 2, 0] and t[at["tmax"][1]] == 2.5
    # r = 0 is a ray: no push-out direction
    a, b, c = at["ray"]
    assert rec(a) == (3.0, 2, 0) and rec(b) == (6.0, 1, 2) and kind[c] == 0 and np.all(nn[a] == 0) and np.all(nn[b] == 0)
    dead = at["dead"]
    assert len(dead) == 12 and [kind[j] for j in dead] == [0] * 12 and np.all(feat[dead] == 0) and np.all(t[dead] == -1)


# ---- 4. any contact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_planes"])
def test_any_hit_reports_an_admitted_candidate_exactly_where_there_is_one(name):
    text, arrays, rows = case(name)
    want_hits, _, cands = reference(name)
    raw = _scene(text)
    try:
        hits, feat = _cast(raw, rows, any_hit=True)
        only_hits, _ = _cast(raw, rows, want_features=False, any_hit=True)
    finally:
        raw.close()
    assert np.array_equal(hits[:, 1] != 0, want_hits[:, 1] != 0)
    bad = sr.any_hit_is_valid(arrays, rows, hits, feat, cands)
    assert len(bad) == 0, (len(bad), bad[:5], rows[bad[:5]], hits[bad[:5]])
    assert np.array_equal(only_hits, hits)
    print(f"{name}: {np.mean(np.any(hits != want_hits, axis=1)):.3f} of the rows report another contact than the first")


# ---- 5. after updates in place; another stream ------------------------------------------------------------------------------------------
def test_cast_follows_geometry_updated_in_place_and_runs_on_another_stream():
    moved, arrays, rows = case("update")
    text = moved.replace(UPDATE_MOVED[1], UPDATE_MOVED[0])
    assert moved != text
    raw = _scene(text)
    try:
        before, _ = _cast(raw, rows)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.cast_spheres(raw, torch.from_numpy(rows).to(DEV), torch.empty((len(rows), 6), dtype=torch.int32, device=DEV))
        assert e.value.status == 6 and b"mirt_cast_spheres" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        hits, feat = _assert_equals_brute_force(raw, "update")
        on_stream, feat_s = _cast(raw, rows, stream=torch.cuda.Stream())
    finally:
        raw.close()
    fresh = _scene(moved)
    try:
        fresh_hits, fresh_feat = _cast(fresh, rows)
    finally:
        fresh.close()
    assert np.array_equal(hits, fresh_hits) and np.array_equal(bits(feat), bits(fresh_feat)) and not np.array_equal(hits, before)
    assert np.array_equal(on_stream, hits) and np.array_equal(bits(feat_s), bits(feat))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n = 8
        Q = torch.zeros((4 * n, 8), dtype=torch.float32, device=DEV)
        Hh = torch.full((4 * n, 6), -7, dtype=torch.int32, device=DEV)
        F = torch.full((4 * n, 8), -7.0, dtype=torch.float32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.cast_spheres(raw, Q[:n], Hh[:n], F[:n])
        assert e.value.status == 6 and b"mirt_cast_spheres" in m.lib().mirt_last_error()
        # the state is checked before n: an unbuilt scene with n == 0 is MIRT_ERR_STATE as well
        assert spherecast.lib().mirt_cast_spheres(raw._h, None, 0, None, None, 0, None) == 6 and b"mirt_cast_spheres" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        L = spherecast.lib()
        pQ, pH, pF = Q.data_ptr(), Hh.data_ptr(), F.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(q=pQ, count=n, h=pH, f=pF, flags=0):
            return L.mirt_cast_spheres(raw._h, vp(q), count, vp(h), vp(f), flags, None)

        def refused(**kw):
            rc = call(**kw)
            return rc == 3 and b"mirt_cast_spheres" in m.lib().mirt_last_error()

        assert refused(count=-1)
        for flags in (2, 3, 0x80000000):
            assert refused(flags=flags)
        assert refused(q=0) and refused(h=0) and refused(q=0, h=0, f=0)
        assert refused(q=pQ + 4) and refused(q=pQ + 8) and refused(h=pH + 2) and refused(f=pF + 8) and refused(f=pF + 4)
        assert refused(h=pQ) and refused(h=pQ + 32 * n - 4) and refused(q=pH + 24 * n - 16, h=pH)       # hits over the casts
        assert refused(f=pQ) and refused(f=pQ + 32 * n - 16) and refused(q=pF + 32 * n - 16, f=pF)     # features over the casts
        assert refused(f=pH) and refused(f=pH + 16) and refused(h=pF + 32 * n - 8)                     # features over the hits
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(F == -7.0))      # nothing ran
        assert call(count=0) == 0 and call(q=0, count=0, h=0, f=0) == 0 and call(count=0, flags=1) == 0
        m.cast_spheres(raw, Q[:0], Hh[:0], F[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == -7)) and bool(torch.all(F == -7.0))
        # adjacent is not overlapping; the features are optional; d_hits needs 4-byte alignment only; the flag is known
        assert call(h=pQ + 32 * n) == 0 and call(f=pQ + 32 * n) == 0 and call(f=0) == 0 and call(h=pH + 4) == 0 and call(flags=1) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh[:n, 1] == 0)) and bool(torch.all(F[:n] == 0))      # rows of zeros have tmax = 0: misses
    finally:
        raw.close()


# ---- 7. into the surface-point queries -----------------------------------------------------------------------------------------------
def test_feature_rows_feed_hemisphere_visibility():
    text, arrays, rows = case("visibility")
    _, want_feat, _ = reference("visibility")
    n = len(rows)
    raw = _scene(text)
    try:
        d_rows = torch.from_numpy(rows).to(DEV)
        hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
        feat = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        m.cast_spheres(raw, d_rows, hits, feat)
        # the rows packed by hand: the restatement's points, the hit records' normals and kinds
        t, kind, _, nn = m.unpack_hits(hits)
        by_hand = m.pack_features(torch.from_numpy(want_feat[:, 0:3].copy()).to(DEV), nn, kind)
        dirs = m.cosine_directions(16, DEV)
        out = [torch.empty((n, 4), dtype=torch.float32, device=DEV) for _ in range(2)]
        mask = [torch.empty(n, dtype=torch.int64, device=DEV) for _ in range(2)]
        m.hemisphere_visibility(raw, feat, dirs, out[0], mask[0], radius=2.0)
        m.hemisphere_visibility(raw, by_hand, dirs, out[1], mask[1], radius=2.0)
        torch.cuda.synchronize()
    finally:
        raw.close()
    assert torch.equal(feat, by_hand) and torch.equal(mask[0], mask[1]) and np.array_equal(bits(out[0].cpu().numpy()), bits(out[1].cpu().numpy()))
    hit = kind.cpu().numpy() != 0
    assert 50 < hit.sum() < n and len(set(mask[0].cpu().numpy()[hit].tolist())) > 3 and bool(torch.all(out[0][torch.from_numpy(~hit).to(DEV)] == 0))

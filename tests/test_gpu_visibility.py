"""Hemisphere visibility at surface points on the GPU (include/mirt_visibility.h: mirt_hemisphere_visibility;
visibility.hemisphere_visibility / ambient_occlusion_frame).  Two yardsticks: the composition the call replaces -- the n x K rays
of the header made on the host by tests/visibility_ref.py, mirt_trace_rays' any-hit answers for them, and visibility_ref's sum --
compared on bit patterns; and f64_arbiter, a float64 brute force that shares no code with the walk, compared on the rows whose
decisions it calls clear.  Then the call itself under another row count, stack split, scene state or stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, visibility
import edge_scenes
import f64_arbiter as arb
import light_scenes
import pyscene
import visibility_ref as vr
from conftest import scene_path
from test_gpu_light import _rows_with_edges
from test_visibility_abi import ARBITER_CASES, arbiter_occlusion

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
W, H = light_scenes.W, light_scenes.H
INF = float("inf")


def bits(a):
    """The bit patterns, every NaN as one pattern: the header leaves a NaN's sign and payload open (the host's and the device's
    arithmetic hand on different ones), where it is NaN it does not."""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _scene(text, **options):
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _features(raw, w=W, h=H):
    _, _, feat = m.ambient_occlusion_frame(raw, w, h, 0, directions=1)
    torch.cuda.synchronize()
    return feat


def _table(k, seed=0):
    """cosine_directions(k) with weights and lengths of its own per row -- the call takes the table as given -- and, from five
    rows on, a row below the horizon and a row of zeros (a ray without a direction: a miss, hence visible)."""
    rng = np.random.default_rng(100 + k + seed)
    d = m.cosine_directions(k)
    d[:, 3] = rng.uniform(0.01, 1.0, k)
    d[:, 0:3] *= np.exp(rng.uniform(-1, 1, (k, 1))).astype(f32)
    if k >= 5:
        d[k - 2, 2] = -d[k - 2, 2]
        d[k - 1, 0:3] = 0
    return d


def _query(raw, rows, dirs, rot=None, radius=INF, want_mask=True, stream=None):
    """mirt_hemisphere_visibility on the rows (a device tensor): (out [n, 4], mask uint64 [n]); the row after the last keeps its
    sentinel."""
    n = rows.shape[0]
    out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device=DEV)
    mask = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV) if want_mask else None
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs, f32)).to(DEV)
    d_rot = torch.from_numpy(np.ascontiguousarray(rot, f32)).to(DEV) if rot is not None else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.hemisphere_visibility(raw, rows, d_dirs, out[:n], mask[:n] if want_mask else None, d_rot, radius, stream=stream)
    torch.cuda.synchronize()
    assert bool(torch.all(out[n] == -7.0)) and (mask is None or int(mask[n]) == -7)
    return out[:n].cpu().numpy(), (mask[:n].cpu().numpy().view(np.uint64) if want_mask else None)


def _composition(raw, F, dirs, rot, radius):
    """The same answer from the calls that were there before: the header's rays from the restatement, trace_rays(any_hit), and
    the restatement's sum.  (want out, want mask, occluded [n, K])."""
    n, k = len(F), len(dirs)
    rays = vr.hemisphere_rays(F, dirs, rot, radius)
    d_rays = torch.from_numpy(rays.reshape(-1, 8)).to(DEV)
    d_hits = torch.empty((n * k, 6), dtype=torch.int32, device=DEV)
    m.trace_rays(raw, d_rays, d_hits, any_hit=True)
    torch.cuda.synchronize()
    occluded = (d_hits.cpu().numpy().view(np.uint32)[:, 1] != 0).reshape(n, k)
    want, want_mask = vr.hemisphere_visibility(F, dirs, rot, radius, occluded)
    return want, want_mask, occluded


def _assert_equals_composition(raw, rows, dirs, rot, radius):
    F = rows.cpu().numpy()
    want, want_mask, occluded = _composition(raw, F, dirs, rot, radius)
    out, mask = _query(raw, rows, dirs, rot, radius)
    assert np.array_equal(mask, want_mask), int(np.count_nonzero(mask != want_mask))
    assert np.array_equal(bits(out), bits(want)), int(np.count_nonzero(np.any(bits(out) != bits(want), axis=1)))
    out_only, _ = _query(raw, rows, dirs, rot, radius, want_mask=False)
    assert np.array_equal(bits(out_only), bits(out))
    return F, out, mask, occluded


# ---- 1. mask and sum against the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 33, 64])
@pytest.mark.parametrize("geometry", ["mixed", "mixed_planes"])
def test_mask_and_sum_equal_the_composition(geometry, k):
    raw = _scene(light_scenes.scene(geometry, 3, "mixed"))
    try:
        feat = _features(raw)
        rows, nf, nodd = _rows_with_edges(feat, k)
        n = rows.shape[0]
        dirs = _table(k)
        some_occluded = some_free = False
        for radius in (0.75, INF):
            for rot in (None, m.rotations(n, k)):
                F, out, mask, occluded = _assert_equals_composition(raw, rows, dirs, rot, radius)
                hit = F[:, 3] != 0
                some_occluded |= bool(np.any(occluded[hit]))
                some_free |= bool(np.any(~occluded[hit]))
                assert np.all(out[~hit] == 0) and np.all(mask[~hit] == 0)
                assert k == 64 or np.all(mask >> np.uint64(k) == 0)
    finally:
        raw.close()
    assert some_occluded and some_free
    assert np.any(~hit[nf + nodd:]) and (geometry.endswith("_planes") or np.any(~hit[:nf])) and np.any(hit[:nf])
    odd = slice(nf, nf + nodd)
    assert np.all(mask[odd][:48] == np.uint64(2 ** k - 1)) and np.all(np.isnan(out[odd][:48, :3]))      # a NaN normal: no ray has a direction
    assert not np.any(np.isnan(out[odd][48:])) and not np.any(np.isnan(out[:nf])) and not np.any(np.isnan(out[:, 3]))
    if k >= 5:
        assert np.all(mask[hit] >> np.uint64(k - 1) == 1)      # the table's row of zeros is visible from everywhere


# ---- 2. against the float64 arbiter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,radius", ARBITER_CASES)
def test_mask_equals_the_float64_arbiter_on_clear_rows(k, radius):
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    raw = _scene(text)
    try:
        out, mask, feat = m.ambient_occlusion_frame(raw, W, H, 0, directions=k, radius=radius, rotate_seed=1, want_mask=True)
        torch.cuda.synchronize()
    finally:
        raw.close()
    F, mask = feat.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    n = len(F)
    hit = F[:, 3] != 0
    rays = vr.hemisphere_rays(F, m.cosine_directions(k), m.rotations(n, 1), radius)
    occluded = np.zeros((n, k), bool)
    margin = np.full(n, np.inf)
    occluded[hit], margin[hit] = arbiter_occlusion(pyscene.parse_lines(text.split("\n")), rays[hit], radius)
    want = ((hit[:, None] & ~occluded).astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    clear = hit & (margin > arb.CLEAR)
    print(f"K {k} radius {radius}: {hit.sum()} hit rows, {clear.sum()} clear, occluded ray share {occluded[hit].mean():.3f}, "
          f"rows differing on clear rows {int((mask != want)[clear].sum())}, on all rows {int((mask != want).sum())}")
    assert hit.sum() > 0.5 * n and clear.sum() >= 0.95 * hit.sum(), (int(hit.sum()), int(clear.sum()))
    assert np.array_equal(mask[clear], want[clear]), int((mask != want)[clear].sum())
    assert np.any(occluded[clear]) and np.any(~occluded[clear])


# ---- 3. row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 33])
def test_row_counts_around_a_wave(k):
    raw = _scene(light_scenes.scene("mixed", 3, "mixed"))
    try:
        rows = _features(raw)[W * 11 + 3:].contiguous()      # (a stretch with hits and misses)
        dirs, rot = _table(k), m.rotations(rows.shape[0], 4)
        full, full_mask = _query(raw, rows, dirs, rot, 2.0)
        assert np.any(full_mask[:63] != 0) and np.any(rows[:257, 3].cpu().numpy() == 0)
        assert len(set(full_mask[:257].tolist())) > 3
        for n in (1, 63, 64, 65, 257):
            out, mask = _query(raw, rows[:n], dirs, rot[:n], 2.0)
            assert np.array_equal(bits(out), bits(full[:n])) and np.array_equal(mask, full_mask[:n]), n
    finally:
        raw.close()


# ---- 4. the stack's spill path ------------------------------------------------------------------------------------------------------
def test_spill_path_gives_the_same_bits():
    raw = _scene(edge_scenes.deep_stack())
    try:
        feat = _features(raw, 64, 48)
        # probe points around the nest of spheres, facing its centre: their rays cross every box of the tree
        rng = np.random.default_rng(3)
        u = rng.normal(size=(500, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        P = (np.array([0, 0, -3]) + rng.uniform(1.0, 3.0, (500, 1)) * u).astype(f32)      # (from just off the largest sphere to far away)
        probes = m.pack_features(torch.from_numpy(P).to(DEV), torch.from_numpy((-u).astype(f32)).to(DEV))
        rows = torch.cat([feat, probes]).contiguous()
        dirs = m.cosine_directions(16)
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        out, mask = _query(raw, rows, dirs)
        full = np.uint64(2 ** 16 - 1)
        assert np.all(mask[-500:] != full) and np.all(mask[-500:] != 0) and len(set(mask.tolist())) > 3, sorted(set(mask.tolist()))[:20]
        for depth in (2, 0):
            raw.set_option("stack_lds_depth", depth)
            out_d, mask_d = _query(raw, rows, dirs)
            assert np.array_equal(bits(out_d), bits(out)) and np.array_equal(mask_d, mask), depth
    finally:
        raw.close()


# ---- 5. after updates in place ------------------------------------------------------------------------------------------------------
def test_query_follows_geometry_updated_in_place():
    raw = _scene(light_scenes.scene("spheres_planes", 3, "mixed"))
    try:
        rows = _features(raw)
        n = rows.shape[0]
        dirs, rot = m.cosine_directions(16), m.rotations(n, 2)
        _, mask0 = _query(raw, rows, dirs, rot, 1.5)
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.hemisphere_visibility(raw, rows, torch.from_numpy(dirs).to(DEV), torch.empty((n, 4), dtype=torch.float32, device=DEV))
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        _, _, mask1, _ = _assert_equals_composition(raw, rows, dirs, rot, 1.5)      # (the same points, the new geometry)
        assert not np.array_equal(mask1, mask0)
    finally:
        raw.close()


# ---- 6. beside a frame in flight ----------------------------------------------------------------------------------------------------
def test_query_on_another_stream_beside_a_render_in_flight():
    raw = m.initRawConfigFromStl(m.parseInput(scene_path("tenthousand")), 0)
    m.build_lbvh_karas(raw)
    try:
        w, h, spp = 320, 180, 16
        p = api.render_params(w, h, spp, counters=True)
        n = api.num_pixels(p)
        feat = _features(raw, w, h)
        dirs, rot = m.cosine_directions(16, DEV), m.rotations(n, 9, DEV)
        out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
        mask = torch.empty(n, dtype=torch.int64, device=DEV)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        keys = ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack", "rays_traversed", "overflow_events")

        def frame(render, queries):
            img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
            out.fill_(-7.0)
            mask.fill_(-7)
            torch.cuda.synchronize()
            if render:
                m.render(img, w, h, spp, raw, params=p, stream=s1)
            for _ in range(queries):
                m.hemisphere_visibility(raw, feat, dirs, out, mask, rot, 5.0, stream=s2)
            torch.cuda.synchronize()
            st = raw.stats() if render else {}
            return img.cpu().numpy(), out.cpu().numpy(), mask.cpu().numpy(), {k: st[k] for k in keys if render}

        img0, _, _, st0 = frame(True, 0)
        _, out1, mask1, _ = frame(False, 1)
        img2, out2, mask2, st2 = frame(True, 6)
        img3, _, _, st3 = frame(True, 0)
    finally:
        raw.close()
    assert np.array_equal(img0, img2) and np.array_equal(img0, img3)
    assert np.array_equal(bits(out1), bits(out2)) and np.array_equal(mask1, mask2) and len(set(mask1.tolist())) > 3
    assert st0 == st2 == st3 and st0["samples"] == n * spp


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n, k = 8, 16
        F = torch.zeros((2 * n, 8), dtype=torch.float32, device=DEV)
        D = torch.zeros((2 * k, 4), dtype=torch.float32, device=DEV)
        R = torch.zeros((4 * n, 2), dtype=torch.float32, device=DEV)      # (room for n float4 after its first n rows)
        out = torch.full((2 * n, 4), -7.0, dtype=torch.float32, device=DEV)
        mask = torch.full((2 * n,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.hemisphere_visibility(raw, F[:n], D[:k], out[:n], mask[:n], R[:n])
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        L = visibility.lib()
        pF, pD, pR, pO, pM = F.data_ptr(), D.data_ptr(), R.data_ptr(), out.data_ptr(), mask.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(f=pF, count=n, d=pD, nd=k, r=pR, radius=1.0, o=pO, km=pM, flags=0):
            return L.mirt_hemisphere_visibility(raw._h, vp(f), count, vp(d), nd, vp(r), radius, vp(o), vp(km), flags, None)

        assert call(count=-1) == 3
        for nd in (0, -1, 65, 1 << 20):
            assert call(nd=nd) == 3
        for radius in (0.0, -1.0, float("nan"), -INF):
            assert call(radius=radius) == 3
        for flags in (1, 2, 0x80000000):
            assert call(flags=flags) == 3
        assert call(f=0) == 3 and call(d=0) == 3 and call(o=0) == 3
        assert call(f=pF + 4) == 3 and call(d=pD + 8) == 3 and call(o=pO + 8) == 3 and call(r=pR + 4) == 3 and call(km=pM + 4) == 3
        assert call(o=pF) == 3 and call(o=pF + 32 * n - 16) == 3            # out inside the feature rows
        assert call(f=pF + 16, o=pF) == 3                                    # ... and the rows' first bytes inside out
        assert call(o=pD) == 3 and call(o=pD + 16 * k - 16) == 3            # out inside the table
        assert call(o=pR) == 3 and call(o=pR + 8 * n - 16, r=pR) == 3        # out inside the rotations
        assert call(km=pF + 32 * n - 8) == 3 and call(km=pD + 16 * k - 8) == 3 and call(km=pR + 8 * n - 8) == 3 and call(km=pO + 16 * n - 8) == 3
        assert b"mirt_hemisphere_visibility" in m.lib().mirt_last_error()
        torch.cuda.synchronize()
        assert bool(torch.all(out == -7.0)) and bool(torch.all(mask == -7))      # nothing ran
        assert call(count=0) == 0 and call(f=0, count=0, d=0, r=0, o=0, km=0) == 0
        m.hemisphere_visibility(raw, F[:0], D[:k], out[:0], mask[:0], R[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(out == -7.0)) and bool(torch.all(mask == -7))
        # adjacent is not overlapping; the mask and the rotations are optional; +inf is a radius
        assert call(o=pF + 32 * n, km=0) == 0 and call(o=pD + 16 * k, km=0) == 0 and call(o=pR + 8 * n, km=0) == 0
        assert call(km=pO + 16 * n) == 0 and call(km=0, r=0) == 0 and call(radius=INF) == 0 and call(nd=1) == 0
        assert call(nd=2 * k) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(out[:n] == 0)) and bool(torch.all(mask[:n] == 0))      # rows of zeros are misses
    finally:
        raw.close()


# ---- 8. the driver ------------------------------------------------------------------------------------------------------------------
def test_ambient_occlusion_frame_is_the_explicit_chain():
    text = light_scenes.scene("spheres_planes", 3, "mixed")
    raw = _scene(text)
    try:
        radius = 0.4
        out, mask, feat = m.ambient_occlusion_frame(raw, W, H, 0, directions=16, radius=radius, rotate_seed=7, want_mask=True)
        plain, no_mask, feat2 = m.ambient_occlusion_frame(raw, W, H, radius=radius)
        table = _table(5)
        own, _, _ = m.ambient_occlusion_frame(raw, W, H, directions=table, radius=radius)
        torch.cuda.synchronize()
        # the explicit chain
        n = W * H
        rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
        rows = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        m.camera_rays(raw, rays, W, H, 0)
        m.trace_rays(raw, rays, hits)
        m.hit_features(raw, rays, hits, rows)
        torch.cuda.synchronize()
        assert torch.equal(feat, rows) and torch.equal(feat2, rows) and no_mask is None
        dirs = m.cosine_directions(16)
        want, want_mask = _query(raw, rows, dirs, m.rotations(n, 7), radius)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(mask.cpu().numpy().view(np.uint64), want_mask)
        assert np.array_equal(bits(plain.cpu().numpy()), bits(_query(raw, rows, dirs, None, radius)[0]))
        assert np.array_equal(bits(own.cpu().numpy()), bits(_query(raw, rows, table, None, radius)[0]))
    finally:
        raw.close()
    F, a = rows.cpu().numpy(), want[:, 3]
    hit = F[:, 3] != 0
    assert hit.sum() > 0.9 * n and np.all(a[hit] >= 0) and np.all(a[hit] <= 1 + 1e-6) and np.any(a[hit] < 0.9) and np.all(a[~hit] == 0)
    # floor points out of the spheres' and the far wall's reach see the whole hemisphere: the butterfly sum of all 16 weights
    sc = pyscene.parse_lines(text.split("\n"))
    P = F[:, 0:3].astype(np.float64)
    reach = np.min([np.linalg.norm(P - np.asarray(s["c"], np.float64), axis=1) - float(s["r"]) for s in sc.spheres], axis=0)
    floor = hit & (np.abs(P[:, 1] + 1) < 1e-4) & (F[:, 5] > 0.99) & (reach > radius + 0.05) & (P[:, 2] > -9 + radius + 0.05)
    whole = vr.butterfly(dirs[None, :, 3:4])[0, 0]
    assert floor.sum() > 50 and whole == f32(1.0)
    assert np.all(a[floor] == whole) and np.all(want_mask[floor] == np.uint64(2 ** 16 - 1))

"""Indirect light at surface points on the GPU (include/mirt_indirect.h: mirt_indirect_light; indirect.indirect_light /
indirect_light_frame).  Three yardsticks: the composition the call replaces -- the n x K gather rays of the header made on the host
by tests/visibility_ref.py, mirt_trace_rays' closest hits for them, mirt_hit_features, mirt_direct_light with MIRT_LIGHT_RAW on the
n x K rows, the materials read back from the scene, and tests/indirect_ref.py's products and sum -- compared on bit patterns;
mirt_hemisphere_visibility, whose a channel and mask the header says this call repeats; and f64_arbiter, a float64 brute force that
shares no code with the walk, compared on the rows whose decisions it calls clear.  Then the call itself under another row count,
stack split, scene state or stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, indirect
import edge_scenes
import f64_arbiter as arb
import indirect_ref as ir
import light_scenes
import pyscene
import visibility_ref as vr
from conftest import scene_path
from test_gpu_light import _rows_with_edges
from test_gpu_visibility import _table, bits
from test_indirect_abi import ARBITER_CASES, arbiter_gather, arbiter_rows, material_scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
W, H = light_scenes.W, light_scenes.H
INF = float("inf")
SETS = {name: (n, kind) for name, n, kind in light_scenes.LIGHT_SETS}


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


def _query(raw, rows, dirs, rot=None, radius=INF, want_mask=True, stream=None):
    """mirt_indirect_light on the rows (a device tensor): (out [n, 4], mask uint64 [n]); the row after the last keeps its
    sentinel."""
    n = rows.shape[0]
    out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device=DEV)
    mask = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV) if want_mask else None
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs, f32)).to(DEV)
    d_rot = torch.from_numpy(np.ascontiguousarray(rot, f32)).to(DEV) if rot is not None else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.indirect_light(raw, rows, d_dirs, out[:n], mask[:n] if want_mask else None, d_rot, radius, stream=stream)
    torch.cuda.synchronize()
    assert bool(torch.all(out[n] == -7.0)) and (mask is None or int(mask[n]) == -7)
    return out[:n].cpu().numpy(), (mask[:n].cpu().numpy().view(np.uint64) if want_mask else None)


def _visibility(raw, rows, dirs, rot, radius):
    n = rows.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
    mask = torch.empty(n, dtype=torch.int64, device=DEV)
    d_rot = torch.from_numpy(np.ascontiguousarray(rot, f32)).to(DEV) if rot is not None else None
    m.hemisphere_visibility(raw, rows, torch.from_numpy(np.ascontiguousarray(dirs, f32)).to(DEV), out, mask, d_rot, radius)
    torch.cuda.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy().view(np.uint64)


def _materials(raw):
    """The scene's materials as it holds them now: float32 [*, 11] of the spheres, the triangles and the planes."""
    tables = []
    for count, get in ((raw.desc.num_spheres, m.get_sphere_materials), (raw.desc.num_triangles, m.get_triangle_materials)):
        t = torch.zeros((count, 11), dtype=torch.float32, device=DEV)
        if count:
            get(raw, t)
        torch.cuda.synchronize()
        tables.append(t.cpu().numpy())
    planes = raw.planes()
    tables.append(np.ascontiguousarray(planes["mat"]).view(f32).reshape(-1, 11) if len(planes) else np.zeros((0, 11), f32))
    return tables


def _composition(raw, F, dirs, rot, radius):
    """The same answer from the calls that were there before.  (want out, want mask, hit [n, K], D [n, K, 3])"""
    n, k = len(F), len(dirs)
    rays = vr.hemisphere_rays(F, dirs, rot, radius)
    d_rays = torch.from_numpy(rays.reshape(-1, 8)).to(DEV)
    d_hits = torch.empty((n * k, 6), dtype=torch.int32, device=DEV)
    d_rows = torch.empty((n * k, 8), dtype=torch.float32, device=DEV)
    d_light = torch.empty((n * k, 4), dtype=torch.float32, device=DEV)
    m.trace_rays(raw, d_rays, d_hits)
    m.hit_features(raw, d_rays, d_hits, d_rows)
    m.direct_light(raw, d_rows, d_light, raw_units=True)
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy().view(np.uint32)
    kind, ident = hits[:, 1], hits[:, 2]
    D = d_light.cpu().numpy()[:, 0:3].reshape(n, k, 3)
    weight = ir.rho(kind, ident, *_materials(raw)).reshape(n, k, 3)
    hit = (kind != 0).reshape(n, k)
    want, want_mask = ir.gather(F, dirs, hit, weight, D)
    return want, want_mask, hit, D, kind.reshape(n, k)


def _assert_equals_composition(raw, rows, dirs, rot, radius):
    F = rows.cpu().numpy()
    want, want_mask, hit, D, kind = _composition(raw, F, dirs, rot, radius)
    out, mask = _query(raw, rows, dirs, rot, radius)
    assert np.array_equal(mask, want_mask), int(np.count_nonzero(mask != want_mask))
    assert np.array_equal(bits(out), bits(want)), int(np.count_nonzero(np.any(bits(out) != bits(want), axis=1)))
    out_only, _ = _query(raw, rows, dirs, rot, radius, want_mask=False)
    assert np.array_equal(bits(out_only), bits(out))
    return F, out, mask, hit, D, kind


# ---- 1. all four channels and the mask against the composition ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 33, 64])
@pytest.mark.parametrize("lights", ["none", "sun", "bulb", "mixed3", "mixed31"])
@pytest.mark.parametrize("geometry", ["mixed", "mixed_planes"])
def test_all_channels_and_the_mask_equal_the_composition(geometry, lights, k):
    nl, kind_of_lights = SETS[lights]
    raw = _scene(material_scene(geometry, nl, kind_of_lights))
    try:
        feat = _features(raw)
        rows, nf, nodd = _rows_with_edges(feat, k)
        n = rows.shape[0]
        dirs = _table(k)
        some_hit = some_miss = some_light = False
        kinds = set()
        for radius in (0.75, INF):
            for rot in (None, m.rotations(n, k)):
                F, out, mask, hit, D, kind = _assert_equals_composition(raw, rows, dirs, rot, radius)
                row_hit = F[:, 3] != 0
                some_hit |= bool(np.any(hit[row_hit]))
                some_miss |= bool(np.any(~hit[row_hit]))
                some_light |= bool(np.any(out[:, 0:3] > 0))
                kinds |= set(kind[row_hit].reshape(-1).tolist())
                assert np.all(out[~row_hit] == 0) and np.all(mask[~row_hit] == 0)
                assert k == 64 or np.all(mask >> np.uint64(k) == 0)
                # the a channel and the complement of the mask are mirt_hemisphere_visibility's
                vis, vis_mask = _visibility(raw, rows, dirs, rot, radius)
                assert np.array_equal(bits(vis[:, 3]), bits(out[:, 3]))
                full = np.uint64(2 ** k - 1)
                assert np.array_equal(np.where(row_hit, ~mask & full, np.uint64(0)), vis_mask)
    finally:
        raw.close()
    assert some_hit and some_miss and some_light == (nl > 0)
    assert k < 5 or kinds >= ({0, 1, 2, 3} if geometry.endswith("_planes") else {0, 1, 2}), kinds
    odd = slice(nf, nf + nodd)
    assert np.all(mask[odd][:48] == 0) and not np.any(np.isnan(out[odd][:48]))      # a NaN normal: no ray has a direction, each adds (0, 0, 0, w)
    assert not np.any(np.isnan(out))
    if k >= 5:
        assert np.all(mask[row_hit] >> np.uint64(k - 1) == 0)      # the table's row of zeros hits nothing from anywhere


# ---- 2. against the float64 arbiter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry,k,radius", ARBITER_CASES)
def test_hit_mask_equals_the_float64_arbiter_on_clear_rows(geometry, k, radius):
    text = material_scene(geometry, 3, "mixed")
    raw = _scene(text)
    try:
        rows = torch.from_numpy(arbiter_rows(_features(raw).cpu().numpy())).to(DEV)
        n = rows.shape[0]
        dirs, rot = m.cosine_directions(k), m.rotations(n, 1)
        out, mask = _query(raw, rows, dirs, rot, radius)
    finally:
        raw.close()
    F = rows.cpu().numpy()
    rays = vr.hemisphere_rays(F, dirs, rot, radius)
    hit64, rgb64, margin = arbiter_gather(pyscene.parse_lines(text.split("\n")), rays, dirs, radius)
    want = (hit64.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    clear = margin > arb.CLEAR
    worst = float(np.abs(out[clear, 0:3].astype(np.float64) - rgb64[clear]).max())
    print(f"{geometry} K {k} radius {radius}: {n} rows, {clear.sum()} clear, hit ray share {hit64.mean():.3f}, "
          f"rows differing on clear rows {int((mask != want)[clear].sum())}, on all rows {int((mask != want).sum())}, worst |rgb - rgb64| {worst:.3g}")
    assert n >= 100 and clear.sum() >= 0.9 * n, (n, int(clear.sum()))
    assert np.array_equal(mask[clear], want[clear]), int((mask != want)[clear].sum())
    assert np.any(hit64[clear]) and np.any(~hit64[clear])


# ---- 3. row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 33])
def test_row_counts_around_a_wave(k):
    raw = _scene(material_scene("mixed_planes", 3, "mixed"))
    try:
        rows = _features(raw)[W * 11 + 3:].contiguous()
        dirs, rot = _table(k), m.rotations(rows.shape[0], 4)
        full, full_mask = _query(raw, rows, dirs, rot, 2.0)
        assert np.any(full_mask[:63] != 0) and len(set(full_mask[:129].tolist())) > 3 and np.any(full[:129, 0:3] > 0)
        for n in (1, 63, 64, 65, 127, 129):
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
        P = (np.array([0, 0, -3]) + rng.uniform(1.0, 3.0, (500, 1)) * u).astype(f32)
        probes = m.pack_features(torch.from_numpy(P).to(DEV), torch.from_numpy((-u).astype(f32)).to(DEV))
        rows = torch.cat([feat, probes]).contiguous()
        dirs = m.cosine_directions(16)
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        out, mask = _query(raw, rows, dirs)
        full = np.uint64(2 ** 16 - 1)
        assert np.all(mask[-500:] != full) and np.all(mask[-500:] != 0) and len(set(mask.tolist())) > 3, sorted(set(mask.tolist()))[:20]
        assert np.any(out[-500:, 0:3] > 0)      # (the sun reaches some of the hit points: the shadow walks ran too)
        for depth in (2, 0):
            raw.set_option("stack_lds_depth", depth)
            out_d, mask_d = _query(raw, rows, dirs)
            assert np.array_equal(bits(out_d), bits(out)) and np.array_equal(mask_d, mask), depth
    finally:
        raw.close()


# ---- 5. after updates in place ------------------------------------------------------------------------------------------------------
def test_query_follows_geometry_materials_and_lights_updated_in_place():
    text = material_scene("mixed_planes", 3, "mixed")
    raw = _scene(text)

    def fresh(new_text, rows, dirs, rot):
        other = _scene(new_text)
        try:
            return _query(other, rows, dirs, rot, 1.5)
        finally:
            other.close()

    try:
        rows = _features(raw)
        n = rows.shape[0]
        dirs, rot = m.cosine_directions(16), m.rotations(n, 2)
        out0, mask0 = _query(raw, rows, dirs, rot, 1.5)
        # geometry: not answered until the build, then the new geometry
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        with pytest.raises(m.MirtError) as e:
            m.indirect_light(raw, rows, torch.from_numpy(dirs).to(DEV), torch.empty((n, 4), dtype=torch.float32, device=DEV))
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        text1 = text.replace("sphere 0.9 -0.2 -2.6 0.6\n", "sphere 0.3 0.4 -2.4 0.7\n")
        assert text1 != text
        _, out1, mask1, _, _, _ = _assert_equals_composition(raw, rows, dirs, rot, 1.5)      # (the same points, the new geometry)
        want1, want_mask1 = fresh(text1, rows, dirs, rot)
        assert not np.array_equal(mask1, mask0) and np.array_equal(mask1, want_mask1) and np.array_equal(bits(out1), bits(want1))
        # materials: the new values with no build
        mats = _materials(raw)[0]
        mats[0, 0:3] = (0.125, 0.5, 0.25)
        m.update_sphere_materials(raw, torch.from_numpy(mats[0:1].copy()).to(DEV), first=0)
        text2 = text1.replace("color 0.8 0.3 0.2\n", "color 0.125 0.5 0.25\n")
        assert text2 != text1
        _, out2, mask2, _, _, _ = _assert_equals_composition(raw, rows, dirs, rot, 1.5)
        want2, want_mask2 = fresh(text2, rows, dirs, rot)
        assert np.array_equal(mask2, mask1) and not np.array_equal(bits(out2), bits(out1))
        assert np.array_equal(mask2, want_mask2) and np.array_equal(bits(out2), bits(want2))
        # lights: likewise
        suns, bulbs = raw.lights()
        suns["color"][0] = (0.25, 0.5, 0.75)
        raw.set_lights(suns, bulbs)
        first_colour = text2.index("color ")
        text3 = text2[:first_colour] + "color 0.25 0.5 0.75\n" + text2[text2.index("\n", first_colour) + 1:]
        _, out3, mask3, _, _, _ = _assert_equals_composition(raw, rows, dirs, rot, 1.5)
        want3, want_mask3 = fresh(text3, rows, dirs, rot)
        assert np.array_equal(mask3, mask1) and not np.array_equal(bits(out3), bits(out2))
        assert np.array_equal(mask3, want_mask3) and np.array_equal(bits(out3), bits(want3))
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
                m.indirect_light(raw, feat, dirs, out, mask, rot, 5.0, stream=s2)
            torch.cuda.synchronize()
            st = raw.stats() if render else {}
            return img.cpu().numpy(), out.cpu().numpy(), mask.cpu().numpy(), {k: st[k] for k in keys if render}

        img0, _, _, st0 = frame(True, 0)
        _, out1, mask1, _ = frame(False, 1)
        img2, out2, mask2, st2 = frame(True, 3)
        img3, _, _, st3 = frame(True, 0)
    finally:
        raw.close()
    assert np.array_equal(img0, img2) and np.array_equal(img0, img3)
    assert np.array_equal(bits(out1), bits(out2)) and np.array_equal(mask1, mask2) and len(set(mask1.tolist())) > 3
    assert st0 == st2 == st3 and st0["samples"] == n * spp


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(material_scene("mixed", 3, "mixed")), 0)
    try:
        n, k = 8, 16
        F = torch.zeros((2 * n, 8), dtype=torch.float32, device=DEV)
        D = torch.zeros((2 * k, 4), dtype=torch.float32, device=DEV)
        R = torch.zeros((4 * n, 2), dtype=torch.float32, device=DEV)      # (room for n float4 after its first n rows)
        out = torch.full((2 * n, 4), -7.0, dtype=torch.float32, device=DEV)
        mask = torch.full((2 * n,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.indirect_light(raw, F[:n], D[:k], out[:n], mask[:n], R[:n])
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        L = indirect.lib()
        pF, pD, pR, pO, pM = F.data_ptr(), D.data_ptr(), R.data_ptr(), out.data_ptr(), mask.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(f=pF, count=n, d=pD, nd=k, r=pR, radius=1.0, o=pO, km=pM, flags=0):
            return L.mirt_indirect_light(raw._h, vp(f), count, vp(d), nd, vp(r), radius, vp(o), vp(km), flags, None)

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
        assert b"mirt_indirect_light" in m.lib().mirt_last_error()
        torch.cuda.synchronize()
        assert bool(torch.all(out == -7.0)) and bool(torch.all(mask == -7))      # nothing ran
        assert call(count=0) == 0 and call(f=0, count=0, d=0, r=0, o=0, km=0) == 0
        m.indirect_light(raw, F[:0], D[:k], out[:0], mask[:0], R[:0])
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
def test_indirect_light_frame_is_the_explicit_chain():
    raw = _scene(material_scene("mixed_planes", 3, "mixed"))
    try:
        radius = 1.5
        out, mask, feat = m.indirect_light_frame(raw, W, H, 0, directions=16, radius=radius, rotate_seed=7, want_mask=True)
        plain, no_mask, feat2 = m.indirect_light_frame(raw, W, H, radius=radius)
        table = _table(5)
        own, _, _ = m.indirect_light_frame(raw, W, H, directions=table, radius=radius)
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
    hit = rows.cpu().numpy()[:, 3] != 0
    assert hit.sum() > 0.9 * n and np.all(want[hit, 0:3] >= 0) and np.any(want[hit, 0:3] > 0) and np.all(want[~hit] == 0)
    assert np.all(want[hit, 3] >= 0) and np.all(want[hit, 3] <= 1 + 1e-6) and len(set(want_mask.tolist())) > 3

"""Direct light at surface points on the GPU (include/mirt_light.h: mirt_direct_light; lighting.direct_light / direct_light_frame).
Three yardsticks, all compared on bit patterns: mirt_render's float image and the oracle's at spp 0 on matte-white scenes, where a
pixel is diffuseLight of its first hit and nothing else; the composition the call replaces -- the n x L shadow rays of the header
made on the host, mirt_trace_rays' any-hit answers for them, and tests/light_ref.py's sum; and the call itself under another row
count, stack split or stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, lighting
import edge_scenes
import light_ref
import light_scenes
import oracle_lib as ol
import pyscene
from conftest import scene_path

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
W, H = light_scenes.W, light_scenes.H
SETS = {name: (n, kind) for name, n, kind in light_scenes.LIGHT_SETS}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def gpu_expf(x):
    return api.probe_math(1, x)


def _scene(text, **options):
    raw = m.initRawConfigFromStl(m.parseText(text), 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _render_f32(raw, w, h):
    img = torch.empty(w * h * 4, dtype=torch.uint8, device=DEV)
    flt = torch.empty(w * h * 4, dtype=torch.float32, device=DEV)
    m.render(img, w, h, 0, raw, d_float=flt)
    torch.cuda.synchronize()
    return flt.cpu().numpy().reshape(-1, 4)


def _frame(raw, w=W, h=H, **kw):
    out, mask, feat = m.direct_light_frame(raw, w, h, 0, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (mask.cpu().numpy().view(np.uint64) if mask is not None else None), feat


def _query(raw, F, raw_units=False, want_mask=True, stream=None):
    """mirt_direct_light on the rows F (a device tensor): (out [n, 4], mask uint64 [n]); the row after the last keeps its sentinel."""
    n = F.shape[0]
    out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device=DEV)
    mask = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV) if want_mask else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.direct_light(raw, F, out[:n], mask[:n] if want_mask else None, raw_units=raw_units, stream=stream)
    torch.cuda.synchronize()
    assert bool(torch.all(out[n] == -7.0)) and (mask is None or int(mask[n]) == -7)
    return out[:n].cpu().numpy(), (mask[:n].cpu().numpy().view(np.uint64) if want_mask else None)


# ---- 1. the chain against the render and the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", list(SETS))
@pytest.mark.parametrize("geometry", light_scenes.GEOMETRIES)
def test_chain_equals_the_render_and_the_oracle(geometry, lights):
    nl, kind = SETS[lights]
    for expose in (None, 2.0):
        text = light_scenes.scene(geometry, nl, kind, expose)
        raw = _scene(text)
        try:
            assert raw.desc.num_suns + raw.desc.num_bulbs == nl
            out, mask, feat = _frame(raw)
            flt = _render_f32(raw, W, H)
        finally:
            raw.close()
        o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
        ref = o.render(W, H, 0, flags=ol.REFERENCE_WALK, nthreads=8)["f32"].reshape(-1, 4)
        o.close()
        hit = feat[:, 3].cpu().numpy() != 0
        assert np.array_equal(bits(out), bits(flt)), (expose, int(np.count_nonzero(np.any(bits(out) != bits(flt), axis=1))))
        assert np.array_equal(bits(out), bits(ref)), (expose, int(np.count_nonzero(np.any(bits(out) != bits(ref), axis=1))))
        assert np.all(out[hit, 3] == 1) and np.all(out[~hit] == 0) and np.all(mask[~hit] == 0)
        assert hit.any() and (geometry.endswith("_planes") or not hit.all())
        assert nl == 64 or np.all(mask >> np.uint64(nl) == 0)
        if nl:
            assert np.any(mask != 0) and np.any(out[hit, :3] > 0)
        else:
            assert np.all(out[hit, :3] == 0)


# ---- 2. mask and sum against the composition --------------------------------------------------------------------------------------
def _rows_with_edges(feat, seed):
    """The frame's rows (hits and misses), copies of hit rows with a NaN in the normal, a zero normal and other hit flags, and
    probe points off every surface with normals of any length (pack_features), a fifth of them marked as no hit."""
    rng = np.random.default_rng(seed)
    F = feat.cpu().numpy()
    hit_rows = F[F[:, 3] != 0]
    odd = hit_rows[rng.choice(len(hit_rows), 96, replace=False)].copy()
    odd[0:24, 4] = np.nan
    odd[24:48, 4:7] = np.nan
    odd[48:60, 4:7] = 0
    odd[60:72, 3] = 2.5
    odd[72:84, 3] = -1.0
    odd[84:96, 7] = 123.0      # the last word is not read
    k = 300
    P = rng.uniform([-3, -0.9, -7], [3, 3, -1], (k, 3)).astype(f32)
    N = (rng.normal(size=(k, 3)) * np.exp(rng.uniform(-2, 2, (k, 1)))).astype(f32)
    probes = m.pack_features(torch.from_numpy(P).to(DEV), torch.from_numpy(N).to(DEV), hit=torch.from_numpy(rng.random(k) > 0.2).to(DEV))
    rows = torch.cat([feat, torch.from_numpy(odd).to(DEV), probes]).contiguous()
    return rows, len(F), len(odd)


@pytest.mark.parametrize("lights", ["mixed3", "mixed33", "mixed64", "bulbs64"])
@pytest.mark.parametrize("geometry", ["mixed", "mixed_planes"])
def test_mask_and_sum_equal_the_composition(geometry, lights):
    nl, kind = SETS[lights]
    raw = _scene(light_scenes.scene(geometry, nl, kind, 2.0))
    try:
        _, _, feat = _frame(raw)
        rows, nf, nodd = _rows_with_edges(feat, nl)
        F = rows.cpu().numpy()
        n = len(F)
        suns, bulbs = raw.lights()
        # the header's MirtRay{o, tmax, d} of every (row, light), built by the restatement in numpy: each operation rounds once there,
        # which torch's own sqrt on the host does not
        rays, lam, tl = light_ref.shadow_rays(F, suns, bulbs)
        d_rays = torch.from_numpy(rays.reshape(-1, 8)).to(DEV)
        d_hits = torch.empty((n * nl, 6), dtype=torch.int32, device=DEV)
        m.trace_rays(raw, d_rays, d_hits, any_hit=True)
        torch.cuda.synchronize()
        occluded = (d_hits.cpu().numpy().view(np.uint32)[:, 1] != 0).reshape(n, nl)
        hit = F[:, 3] != 0
        lit = hit[:, None] & (lam > 0) & ~occluded
        want_mask = (lit.astype(np.uint64) << np.arange(nl, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        for raw_units in (False, True):
            out, mask = _query(raw, rows, raw_units=raw_units)
            want, ref_mask = light_ref.direct_light(F, suns, bulbs, raw.shading().expose, raw_units, occluded, gpu_expf)
            assert np.array_equal(ref_mask, want_mask)
            assert np.array_equal(mask, want_mask), int(np.count_nonzero(mask != want_mask))
            assert np.array_equal(bits(out), bits(want)), int(np.count_nonzero(np.any(bits(out) != bits(want), axis=1)))
            out_only, _ = _query(raw, rows, raw_units=raw_units, want_mask=False)
            assert np.array_equal(bits(out_only), bits(out))
    finally:
        raw.close()
    odd = slice(nf, nf + nodd)
    assert np.all(want_mask[odd][:60] == 0) and np.all(out[odd][:60] == np.array([0, 0, 0, 1], f32))      # NaN and zero normals: a hit that nothing lights
    assert np.any(want_mask[odd][60:] != 0) and np.all(out[odd][60:, 3] == 1)
    probes = slice(nf + nodd, n)
    assert np.any(~hit[probes]) and np.all(out[probes][~hit[probes]] == 0) and np.any(want_mask[probes] != 0)
    assert geometry.endswith("_planes") or np.any(~hit[:nf])
    assert 0 < np.count_nonzero(occluded & (lam > 0) & hit[:, None]) and np.any(lit)
    assert not np.any(np.isnan(out))


# ---- 3. row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", ["mixed3", "mixed33"])
def test_row_counts_around_a_wave(lights):
    nl, kind = SETS[lights]
    raw = _scene(light_scenes.scene("mixed", nl, kind, 2.0))
    try:
        _, _, feat = _frame(raw)
        rows = feat[W * 11 + 3:].contiguous()      # (a stretch with hits and misses)
        full, full_mask = _query(raw, rows)
        assert np.any(full_mask[:63] != 0) and np.any(rows[:257, 3].cpu().numpy() == 0)
        for n in (1, 63, 64, 65, 257):
            out, mask = _query(raw, rows[:n])
            assert np.array_equal(bits(out), bits(full[:n])) and np.array_equal(mask, full_mask[:n]), n
    finally:
        raw.close()


# ---- 4. the stack's spill path ------------------------------------------------------------------------------------------------------
def test_spill_path_gives_the_same_bits():
    text = edge_scenes.deep_stack().replace("sun 1 1 1\n", "sun 1 1 1\nbulb 0 0 -3\nbulb 0.2 0.1 -3.1\nbulb 3 3 0\n", 1)
    raw = _scene(text)
    try:
        _, _, feat = _frame(raw, 64, 48)
        # probe points around the nest of spheres, facing its centre: their shadow rays cross every box of the tree
        rng = np.random.default_rng(3)
        u = rng.normal(size=(500, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        P = (np.array([0, 0, -3]) + 2.0 * u).astype(f32)
        probes = m.pack_features(torch.from_numpy(P).to(DEV), torch.from_numpy((-u).astype(f32)).to(DEV))
        rows = torch.cat([feat, probes]).contiguous()
        assert raw.get_option("stack_lds_depth") not in (0, 2)
        out, mask = _query(raw, rows)
        assert np.any(mask != 0) and np.any(mask[-500:] & np.uint64(2) == 0)
        for depth in (2, 0):
            raw.set_option("stack_lds_depth", depth)
            out_d, mask_d = _query(raw, rows)
            assert np.array_equal(bits(out_d), bits(out)) and np.array_equal(mask_d, mask), depth
    finally:
        raw.close()


# ---- 5. after updates in place ------------------------------------------------------------------------------------------------------
def test_query_follows_lights_shading_and_geometry_updated_in_place():
    raw = _scene(light_scenes.scene("spheres_planes", 3, "mixed"))
    try:
        out0, mask0, _ = _frame(raw)
        assert np.array_equal(bits(out0), bits(_render_f32(raw, W, H)))
        suns, bulbs = raw.lights()
        bulbs["v"][0] = [1.5, 2.5, -1.0]
        bulbs["color"][0] = [0.2, 1.5, 0.7]
        suns["color"][0] = [0.9, 0.1, 0.4]
        raw.set_lights(suns, bulbs)
        out1, mask1, _ = _frame(raw)
        assert np.array_equal(bits(out1), bits(_render_f32(raw, W, H)))
        assert not np.array_equal(mask1, mask0) and not np.array_equal(out1, out0)
        raw.set_shading(expose=1.5)
        out2, mask2, _ = _frame(raw)
        assert np.array_equal(bits(out2), bits(_render_f32(raw, W, H)))
        assert np.array_equal(mask2, mask1) and not np.array_equal(out2, out1)
        rawu, _, _ = _frame(raw, raw_units=True)
        assert np.array_equal(bits(rawu), bits(out1))      # raw units: the terms before the exposure
        m.update_spheres(raw, torch.tensor([[0.3, 0.4, -2.4, 0.7]], dtype=torch.float32, device=DEV), first=1)
        L = lighting.lib()
        F, O = torch.zeros((4, 8), dtype=torch.float32, device=DEV), torch.zeros((4, 4), dtype=torch.float32, device=DEV)
        assert L.mirt_direct_light(raw._h, C.c_void_p(F.data_ptr()), 4, C.c_void_p(O.data_ptr()), None, 0, None) == 6      # updated, not yet built
        m.build_lbvh_karas(raw)
        out3, mask3, _ = _frame(raw)
        assert np.array_equal(bits(out3), bits(_render_f32(raw, W, H)))
        assert not np.array_equal(mask3, mask2)
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
        _, _, feat = _frame(raw, w, h)
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
                m.direct_light(raw, feat, out, mask, stream=s2)
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
    assert np.array_equal(bits(out1), bits(out2)) and np.array_equal(mask1, mask2) and np.any(mask1 != 0)
    assert st0 == st2 == st3 and st0["samples"] == n * spp


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(light_scenes.scene("mixed", 3, "mixed")), 0)
    try:
        n = 8
        F = torch.zeros((2 * n, 8), dtype=torch.float32, device=DEV)
        out = torch.full((2 * n, 4), -7.0, dtype=torch.float32, device=DEV)
        mask = torch.full((2 * n,), -7, dtype=torch.int64, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.direct_light(raw, F[:n], out[:n], mask[:n])
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        L = lighting.lib()
        pF, pO, pM = F.data_ptr(), out.data_ptr(), mask.data_ptr()

        def call(f=pF, count=n, o=pO, k=pM, flags=0):
            return L.mirt_direct_light(raw._h, C.c_void_p(f) if f else None, count, C.c_void_p(o) if o else None, C.c_void_p(k) if k else None, flags, None)

        assert call(count=-1) == 3
        assert call(f=0) == 3 and call(o=0) == 3
        assert call(f=pF + 4) == 3 and call(o=pO + 8) == 3 and call(k=pM + 4) == 3
        for flags in (2, 3, 0x80000000):
            assert call(flags=flags) == 3
        assert call(o=pF) == 3 and call(o=pF + 32 * n - 16) == 3            # out inside the feature rows
        assert call(f=pF + 16, o=pF) == 3                                    # ... and the rows' first bytes inside out
        assert call(k=pF + 32 * n - 8) == 3 and call(k=pO + 16 * n - 8) == 3      # the mask inside the rows, inside out
        assert b"mirt_direct_light" in m.lib().mirt_last_error()
        torch.cuda.synchronize()
        assert bool(torch.all(out == -7.0)) and bool(torch.all(mask == -7))      # nothing ran
        assert call(count=0) == 0 and call(f=0, count=0, o=0, k=0) == 0
        m.direct_light(raw, F[:0], out[:0], mask[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(out == -7.0)) and bool(torch.all(mask == -7))
        assert call(o=pF + 32 * n, k=0) == 0 and call(k=0) == 0 and call() == 0      # adjacent is not overlapping; the mask is optional
        torch.cuda.synchronize()
        assert bool(torch.all(out[:n] == 0)) and bool(torch.all(out[n:] == -7.0)) and bool(torch.all(mask[:n] == 0))      # rows of zeros are misses
    finally:
        raw.close()

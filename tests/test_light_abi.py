"""Direct light at surface points (include/mirt_light.h: mirt_direct_light): the wrappers' checks, the kernel's code generation,
and tests/light_ref.py -- the numpy restatement of the header's text -- against the oracle's renders of matte-white scenes.  The
header against lighting.py's signature table and the built library is a row of tests/test_extension_abi.py.  No GPU needed."""
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import denoise_ref as dr
import f64_arbiter as arb
import light_ref
import light_scenes
import oracle_lib as ol
import pyscene
from test_denoise_abi import _pinhole_rays
from codegen_lib import _resource_usage

f32 = np.float32


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------
def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    F, out, mask = torch.zeros((4, 8)), torch.zeros((4, 4)), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="dtype"):
        m.direct_light(raw, F.double(), out)
    with pytest.raises(ValueError, match="shape"):
        m.direct_light(raw, torch.zeros((4, 7)), out)
    with pytest.raises(ValueError, match="shape"):
        m.direct_light(raw, F, torch.zeros((5, 4)))
    with pytest.raises(ValueError, match="dtype"):
        m.direct_light(raw, F, out, mask.int())
    with pytest.raises(ValueError, match="shape"):
        m.direct_light(raw, F, out, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        m.direct_light(raw, F, torch.zeros((4, 8))[:, ::2])
    with pytest.raises(ValueError, match="cuda"):
        m.direct_light(raw, F, out, mask)
    P = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    rows = m.pack_features(P, -P, hit=[1, 0, 2, 1])
    assert rows.shape == (4, 8) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows[:, 0:3], P) and torch.equal(rows[:, 4:7], -P) and rows[:, 3].tolist() == [1, 0, 1, 1] and torch.all(rows[:, 7] == 0)
    assert torch.all(m.pack_features(P, P)[:, 3] == 1)
    with pytest.raises(ValueError, match="shape"):
        m.pack_features(P, P[:3])


# ---- code generation ----------------------------------------------------------------------------------------------------------------
def test_light_kernel_codegen_runs_8_waves_per_simd_with_scratch_only_for_the_stack():
    """light.hip compiled for gfx950: the kernel within the 64 VGPRs of 8 waves per SIMD, a 20-entry LDS stack per lane of a
    256-thread block, no register spills, and the private segment of the query kernels: the 64-entry spill array of the stack
    (256 B) and the 16 B the compiler adds to it there too -- nothing else lives in scratch."""
    res, _ = _resource_usage("light.hip")
    kernels = [k for k in res if "direct_light_kernel" in k]
    assert len(kernels) == 1, list(res)
    r = res[kernels[0]]
    assert r["Occupancy [waves/SIMD]"] == 8, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
    assert r["ScratchSize [bytes/lane]"] == 64 * 4 + 16, r
    query, _ = _resource_usage("query.hip")
    assert {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k} == {r["ScratchSize [bytes/lane]"]}


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------
def _brute_force_occlusion(sc, rays, lam, tl):
    """Every shadow ray [n, L] against every primitive and plane of the scene in float64 (f64_arbiter's intersections, which
    record the relative margin of each of their decisions): occluded [n, L] and the smallest margin of a row's decisions -- the
    facing tests, every hit or miss, and a hit's distance against the light's."""
    a = arb.Arbiter(sc)
    n, L, _ = rays.shape
    occluded = np.zeros((n, L), bool)
    margin = np.full(n, np.inf)
    for i in range(n):
        for li in range(L):
            a.margin, a.what = arb.INF, None
            a._decide(abs(float(lam[i, li])), "facing")      # a cosine of unit vectors against 0
            if lam[i, li] > 0:
                o = tuple(float(x) for x in rays[i, li, 0:3])
                d = arb._normalize(tuple(float(x) for x in rays[i, li, 4:7]))
                h = a.hit_nearest(o, d, 1)
                if h.is_hit and li >= len(sc.suns):
                    a._decide(arb._rel(h.t, float(tl[i, li])), "shadow hit before the light")
                occluded[i, li] = h.is_hit and h.t < float(tl[i, li])
            margin[i] = min(margin[i], a.margin)
    return occluded, margin


@pytest.mark.parametrize("geometry", ["spheres_planes", "mixed_planes"])
@pytest.mark.parametrize("expose", [None, 2.0])
def test_restatement_equals_the_oracle_on_matte_white_scenes(geometry, expose):
    """The chain of include/mirt_light.h on the CPU: the oracle's spp-0 render of a matte-white scene (the reference's walk), its
    primary-hit records turned into feature rows, the shadow rays decided by brute force in float64, and light_ref's sum.  On
    every row whose decisions are clear of f64_arbiter.CLEAR the rgb equals the oracle's bit for bit and alpha is 1; at most a
    tenth of the hit rows may be left out."""
    w, h = light_scenes.W, light_scenes.H
    sc = pyscene.parse_lines(light_scenes.scene(geometry, 3, "mixed", expose).split("\n"))
    assert (len(sc.suns), len(sc.bulbs)) == (2, 1) and sc.gi == 0 and sc.bounces >= 1
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        ref = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)
    finally:
        o.close()
    F = dr.features(_pinhole_rays(sc, w, h), np.ascontiguousarray(ref["aov"]).reshape(-1).view(np.uint32).reshape(-1, 6))
    A = sc.arrays()
    rays, lam, tl = light_ref.shadow_rays(F, A["suns"], A["bulbs"])
    hit = F[:, 3] != 0
    occluded = np.zeros(lam.shape, bool)
    margin = np.full(len(F), np.inf)
    occluded[hit], margin[hit] = _brute_force_occlusion(sc, rays[hit], lam[hit], tl[hit])
    out, mask = light_ref.direct_light(F, A["suns"], A["bulbs"], sc.expose, False, occluded, dr.expf)
    want = ref["f32"].reshape(-1, 4)
    clear = hit & (margin > arb.CLEAR)
    print(f"{geometry} expose {expose}: {hit.sum()} hit rows, {clear.sum()} clear, lit bits {[int(((mask >> np.uint64(k)) & np.uint64(1)).sum()) for k in range(3)]}")
    assert hit.sum() > 0.5 * len(F) and clear.sum() >= 0.9 * hit.sum(), (int(hit.sum()), int(clear.sum()))
    assert np.array_equal(out[clear, :3].view(np.uint32), want[clear, :3].view(np.uint32))
    assert np.all(out[clear, 3] == 1) and np.all(want[clear, 3] == 1)
    assert np.all(out[~hit] == 0) and np.all(want[~hit] == 0) and np.all(mask[~hit] == 0)
    # some rows are reached by several lights, some by one, some by none (the sun from below reaches nothing over a floor); raw units
    # differ exactly where exposure acts
    assert len(set(mask[hit].tolist())) >= 3 and np.any(mask[hit] == 0) and np.all(mask < 8)
    raw_out, raw_mask = light_ref.direct_light(F, A["suns"], A["bulbs"], sc.expose, True, occluded, dr.expf)
    assert np.array_equal(raw_mask, mask)
    assert np.array_equal(raw_out, out) == (expose is None)

"""Hemisphere visibility at surface points (include/mirt_visibility.h: mirt_hemisphere_visibility): the wrappers' checks, the
kernel's code generation, the properties of tests/visibility_ref.py -- the numpy restatement of the header's text -- and the
restatement's rays decided twice on the CPU: by f64_arbiter in float64 and by the float32 brute force of
tests/test_gpu_queries.py.  The header against visibility.py's signature table and the built library:
tests/test_extension_abi.py.  No GPU needed."""
import functools
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
import denoise_ref as dr
import f64_arbiter as arb
import light_scenes
import oracle_lib as ol
import pyscene
import visibility_ref as vr
from test_denoise_abi import _pinhole_rays
from codegen_lib import _resource_usage

f32 = np.float32
# (K, radius) of the arbiter comparisons, here and on the GPU
ARBITER_CASES = [(16, 1.5), (33, 3.0), (64, float("inf"))]


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------
def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    F, D, out = torch.zeros((4, 8)), torch.zeros((16, 4)), torch.zeros((4, 4))
    mask, rot = torch.zeros(4, dtype=torch.int64), torch.zeros((4, 2))
    with pytest.raises(ValueError, match="dtype"):
        m.hemisphere_visibility(raw, F.double(), D, out)
    with pytest.raises(ValueError, match="dtype"):
        m.hemisphere_visibility(raw, F, D.double(), out)
    with pytest.raises(ValueError, match="shape"):
        m.hemisphere_visibility(raw, torch.zeros((4, 7)), D, out)
    with pytest.raises(ValueError, match="shape"):
        m.hemisphere_visibility(raw, F, torch.zeros((16, 3)), out)
    with pytest.raises(ValueError, match="1 to 64 rows"):
        m.hemisphere_visibility(raw, F, torch.zeros((65, 4)), out)
    with pytest.raises(ValueError, match="1 to 64 rows"):
        m.hemisphere_visibility(raw, F, torch.zeros((0, 4)), out)
    with pytest.raises(ValueError, match="shape"):
        m.hemisphere_visibility(raw, F, D, torch.zeros((5, 4)))
    with pytest.raises(ValueError, match="dtype"):
        m.hemisphere_visibility(raw, F, D, out, mask.int())
    with pytest.raises(ValueError, match="shape"):
        m.hemisphere_visibility(raw, F, D, out, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        m.hemisphere_visibility(raw, F, D, out, mask, torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="dtype"):
        m.hemisphere_visibility(raw, F, D, out, mask, rot.double())
    with pytest.raises(ValueError, match="contiguous"):
        m.hemisphere_visibility(raw, F, D, torch.zeros((4, 8))[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.hemisphere_visibility(raw, F, torch.zeros((16, 8))[:, ::2], out)
    with pytest.raises(ValueError, match="cuda"):
        m.hemisphere_visibility(raw, F, D, out, mask, rot)
    with pytest.raises(ValueError, match="1 to 64"):
        m.cosine_directions(65)
    assert isinstance(m.cosine_directions(5), np.ndarray) and isinstance(m.rotations(3, 0), np.ndarray)
    t = m.cosine_directions(5, "cpu")
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), m.cosine_directions(5))
    assert np.array_equal(m.rotations(7, 2, "cpu").numpy(), m.rotations(7, 2))


# ---- code generation ----------------------------------------------------------------------------------------------------------------
def test_visibility_kernel_codegen_runs_8_waves_per_simd_with_scratch_only_for_the_stack():
    """visibility.hip compiled for gfx950: one kernel, within the 64 VGPRs of 8 waves per SIMD, a 20-entry LDS stack per lane of
    a 256-thread block, no register spills, and the private segment of the query kernels."""
    res, _ = _resource_usage("visibility.hip")
    assert len(res) == 1 and "hemisphere_visibility_kernel" in list(res)[0], list(res)
    r = list(res.values())[0]
    assert r["Occupancy [waves/SIMD]"] == 8, r
    assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
    query, _ = _resource_usage("query.hip")
    assert {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k} == {r["ScratchSize [bytes/lane]"]}


# ---- properties of the restatement --------------------------------------------------------------------------------------------------
def test_the_basis_is_orthonormal():
    """T, B, N of the header for 10^4 random unit normals and the edge cases: every pairwise dot within 4e-7 of 0, every squared
    length within 4e-7 of 1.  The bound: N has unit length to 2^-23 (three roundings of normalize); each entry of T and B is made
    by at most 4 rounded operations on quantities of magnitude <= 1 (a = -1 / (s + N.z) has |a| <= 1, because |s + N.z| >= 1), so
    carries an error of at most 4 x 2^-24 = 2.4e-7 in an entry of magnitude <= 1; measured 3.1e-7 on these normals."""
    rng = np.random.default_rng(11)
    u = rng.normal(size=(10000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    edge = np.array([[0, 0, 1], [0, 0, -1], [0.6, 0.8, 0.0], [0.6, -0.8, -0.0], [0, 1, 0.0], [1, 0, -0.0]], np.float64)
    z = -1.0 + 2.0 ** -24
    edge = np.concatenate([edge, [[np.sqrt(1 - z * z), 0, z], [0, -np.sqrt(1 - z * z), z]]])
    with np.errstate(all="ignore"):
        N = np.concatenate([vr._normalize(u.astype(f32)), edge.astype(f32)])      # (the edge cases as written: their z is the point)
        T, Bv = vr.basis(N)
    assert np.signbit(N[10003, 2]) and not np.signbit(N[10002, 2]) and N[10006, 2] == f32(z) and N[10006, 2] > -1
    assert T.dtype == f32 and Bv.dtype == f32 and np.all(np.isfinite(T)) and np.all(np.isfinite(Bv))
    T, Bv, N = (a.astype(np.float64) for a in (T, Bv, N))
    dots = [np.abs((a * b).sum(axis=1) - want) for a, b, want in ((T, T, 1), (Bv, Bv, 1), (N, N, 1), (T, Bv, 0), (T, N, 0), (Bv, N, 0))]
    worst = max(float(d.max()) for d in dots)
    print(f"worst deviation from orthonormal: {worst:.3g}")
    assert worst <= 4e-7
    # right-handed: T x B = N
    assert np.abs(np.cross(T, Bv) - N).max() <= 1e-6


@pytest.mark.parametrize("k", [1, 2, 5, 16, 33, 64])
def test_cosine_directions(k):
    d = m.cosine_directions(k)
    assert d.shape == (k, 4) and d.dtype == f32 and d.flags["C_CONTIGUOUS"]
    d64 = d.astype(np.float64)
    assert np.abs(np.sqrt((d64[:, :3] ** 2).sum(axis=1)) - 1).max() <= 1e-6
    assert np.all(d[:, 2] > 0) and abs(d64[:, 3].sum() - 1) <= 1e-6 and np.all(d[:, 3] == f32(1.0 / k))
    assert np.array_equal(d, m.cosine_directions(k))
    i = k - 1
    u = (i + 0.5) / k
    phi = 0.3 + i * 2.399963229728653
    assert np.array_equal(d[i], np.array([np.sqrt(u) * np.cos(phi), np.sqrt(u) * np.sin(phi), np.sqrt(1 - u), 1 / k]).astype(f32))


def test_rotations_are_cosine_and_sine_of_seeded_angles():
    r = m.rotations(1000, 5)
    assert r.shape == (1000, 2) and r.dtype == f32 and np.array_equal(r, m.rotations(1000, 5)) and not np.array_equal(r, m.rotations(1000, 6))
    assert np.abs((r.astype(np.float64) ** 2).sum(axis=1) - 1).max() <= 2e-7
    angle = np.random.default_rng(5).random(1000) * 2 * np.pi
    assert np.array_equal(r, np.stack([np.cos(angle), np.sin(angle)], axis=1).astype(f32))
    assert len({(a > 0, b > 0) for a, b in r.tolist()}) == 4


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    F = np.zeros((n, 8), f32)
    F[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    F[:, 3] = 1
    F[:, 4:7] = rng.normal(size=(n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1)))
    return F


@pytest.mark.parametrize("k", [1, 5, 16, 33, 64])
def test_nothing_occluded_gives_the_butterfly_sum_of_the_weights_and_the_full_mask(k):
    F = _rows(50, k)
    F[7, 3] = 0
    F[8, 3] = -2.5
    dirs = m.cosine_directions(k)
    dirs[:, 3] = np.random.default_rng(k).uniform(0.01, 1.0, k).astype(f32)      # (weights whose sum depends on the order)
    out, mask = vr.hemisphere_visibility(F, dirs, None, np.inf, np.zeros((50, k), bool))
    G = 1 << (k - 1).bit_length()
    w = np.zeros(G, f32)
    w[:k] = dirs[:, 3]
    off = G // 2
    while off:
        w = w + w[np.arange(G) ^ off]
        off //= 2
    assert w.dtype == f32 and np.all(w == w[0])
    hit = np.arange(50) != 7
    assert np.all(out[hit, 3].view(np.uint32) == w[0].view(np.uint32))
    assert np.all(mask[hit] == np.uint64(2 ** k - 1))
    assert np.all(out[7] == 0) and not np.any(np.signbit(out[7])) and mask[7] == 0      # hit == 0: zeros
    # everything occluded: +0 everywhere; one direction visible: that direction's term, unsummed
    out0, mask0 = vr.hemisphere_visibility(F, dirs, None, np.inf, np.ones((50, k), bool))
    assert np.all(out0.view(np.uint32) == 0) and np.all(mask0 == 0)
    occ = np.ones((50, k), bool)
    occ[:, k - 1] = False
    out1, mask1 = vr.hemisphere_visibility(F, dirs, None, np.inf, occ)
    rays = vr.hemisphere_rays(F, dirs, None, np.inf)
    u = vr._normalize(rays[:, k - 1, 4:7].copy())
    assert np.array_equal(out1[hit, :3], (u * dirs[k - 1, 3])[hit]) and np.all(out1[hit, 3] == dirs[k - 1, 3])
    assert np.all(mask1[hit] == np.uint64(1 << (k - 1)))
    # the rays: the origin of the header, tmax = radius, a direction of unit length that the rotation turns about the normal
    rot = m.rotations(50, 3)
    turned = vr.hemisphere_rays(F, dirs, rot, 0.75)
    N = vr._normalize(F[:, 4:7].copy())
    assert np.all(turned[:, :, 3] == f32(0.75)) and np.array_equal(turned[:, :, 0:3], rays[:, :, 0:3]) and np.all(turned[:, :, 7] == 0)
    assert np.array_equal(rays[:, 0, 0:3], F[:, 0:3] + F[:, 4:7] * f32(0.001))
    for r in (rays, turned):
        d = r[:, :, 4:7].astype(np.float64)
        assert np.abs(np.sqrt((d ** 2).sum(axis=2)) - 1).max() <= 2e-6
        assert np.abs((d * N[:, None, :]).sum(axis=2) - dirs[None, :, 2]).max() <= 2e-6      # lz is the cosine to the normal
    assert not np.array_equal(turned[:, :, 4:7], rays[:, :, 4:7])


# ---- the restatement's rays decided twice ---------------------------------------------------------------------------------------------
def arbiter_occlusion(sc, rays, radius):
    """Every ray [n, K, 8] of the restatement against every primitive and plane of the scene in float64 (f64_arbiter's
    intersections, which record the relative margin of each of their decisions): occluded [n, K] and the smallest margin of a
    row's decisions -- every hit or miss, and a hit's distance against the radius."""
    a = arb.Arbiter(sc)
    n, K, _ = rays.shape
    occluded = np.zeros((n, K), bool)
    margin = np.full(n, np.inf)
    R = rays.astype(np.float64)
    for i in range(n):
        a.margin, a.what = arb.INF, None
        o = tuple(R[i, 0, 0:3].tolist())
        for k in range(K):
            h = a.hit_nearest(o, arb._normalize(tuple(R[i, k, 4:7].tolist())), 1)
            if h.is_hit:
                a._decide(arb._rel(h.t, radius), "hit within the radius")
                occluded[i, k] = h.t < radius
        margin[i] = a.margin
    return occluded, margin


@functools.lru_cache(maxsize=None)
def _oracle_rows():
    """The first hits of the pinhole rays of mixed_planes at 40 x 30, as test_light_abi makes them."""
    w, h = light_scenes.W, light_scenes.H
    text = light_scenes.scene("mixed_planes", 3, "mixed")
    sc = pyscene.parse_lines(text.split("\n"))
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        ref = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)
    finally:
        o.close()
    F = dr.features(_pinhole_rays(sc, w, h), np.ascontiguousarray(ref["aov"]).reshape(-1).view(np.uint32).reshape(-1, 6))
    return text, sc, F


@pytest.mark.parametrize("k,radius", ARBITER_CASES)
def test_restatement_decided_in_float64_and_in_float32_gives_the_same_result(k, radius):
    """The rays of visibility_ref.hemisphere_rays for the first-hit rows of mixed_planes, cosine_directions(k) and
    rotations(n, 1), decided by f64_arbiter (float64, brute force, margins recorded) and by test_gpu_queries.brute_force (float32,
    the reference's intersections restated in numpy).  On every row whose decisions are clear of f64_arbiter.CLEAR the two masks
    and the two sums are the same; at most 5 % of the hit rows may be left out."""
    from test_gpu_queries import brute_force
    text, sc, F = _oracle_rows()
    n = len(F)
    hit = F[:, 3] != 0
    dirs, rot = m.cosine_directions(k), m.rotations(n, 1)
    rays = vr.hemisphere_rays(F, dirs, rot, radius)
    occ64 = np.zeros((n, k), bool)
    margin = np.full(n, np.inf)
    occ64[hit], margin[hit] = arbiter_occlusion(sc, rays[hit], radius)
    flat = rays.reshape(-1, 8)
    with np.errstate(all="ignore"):
        t32, _, _, _ = brute_force(m.parseText(text), np.ascontiguousarray(flat[:, 0:3]), np.ascontiguousarray(flat[:, 4:7]))
    occ32 = (t32 < f32(radius)).reshape(n, k)
    out64, mask64 = vr.hemisphere_visibility(F, dirs, rot, radius, occ64)
    out32, mask32 = vr.hemisphere_visibility(F, dirs, rot, radius, occ32)
    clear = hit & (margin > arb.CLEAR)
    share = occ64[hit].mean()
    print(f"K {k} radius {radius}: {hit.sum()} hit rows, {clear.sum()} clear, occluded ray share {share:.3f}, "
          f"rows differing {int((mask64 != mask32)[hit].sum())}")
    assert hit.sum() > 0.5 * n and clear.sum() >= 0.95 * hit.sum(), (int(hit.sum()), int(clear.sum()))
    assert np.array_equal(mask64[clear], mask32[clear])
    assert np.array_equal(out64[clear].view(np.uint32), out32[clear].view(np.uint32))
    assert 0.05 < share < 0.7 and len(set(mask64[clear].tolist())) > 3
    assert np.isinf(radius) or np.any(mask64[clear] == np.uint64(2 ** k - 1))      # (without a radius the far wall ends some ray of every row)
    assert np.all(out64[~hit] == 0) and np.all(mask64[~hit] == 0)
    a = out64[clear, 3]
    assert np.all(a >= 0) and np.all(a <= 1 + 1e-6)

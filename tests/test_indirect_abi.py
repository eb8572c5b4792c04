"""Indirect light at surface points (include/mirt_indirect.h: mirt_indirect_light): the wrappers' checks, the kernel's code
generation, the properties of tests/indirect_ref.py -- the numpy restatement of the header's text -- and the restatement decided
twice on the CPU: by f64_arbiter in float64 and by the float32 brute force of tests/test_gpu_queries.py.  The header against
indirect.py's signature table and the built library: tests/test_extension_abi.py.  No GPU needed."""
import functools
import os
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import binding, indirect, visibility
import denoise_ref as dr
import f64_arbiter as arb
import indirect_ref as ir
import light_ref
import light_scenes
import oracle_lib as ol
import pyscene
import visibility_ref as vr
from test_denoise_abi import _pinhole_rays
from codegen_lib import _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAME = "mirt_indirect_light"
# (geometry, K, radius) of the arbiter comparisons, here and on the GPU: 16 gather rays and up to 16 x 3 shadow rays per row
ARBITER_CASES = [("mixed", 16, 1.5), ("mixed", 16, float("inf")), ("mixed_planes", 16, 1.5), ("mixed_planes", 16, float("inf"))]
# The kernel's registers under its launch bound, as -Rpass-analysis=kernel-resource-usage reports them
KERNEL_VGPRS, KERNEL_WAVES_PER_SIMD = 72, 7
# |rgb of the float32 restatement - the float64 value| on the clear rows of ARBITER_CASES: the largest seen on the CPU, and the
# bound asserted, 8 x that
RGB_WORST_SEEN = 6.21e-8      # (mixed_planes, K 16, radius inf; rgb up to 0.66)
RGB_TOLERANCE = 8 * RGB_WORST_SEEN

# ---- scenes -------------------------------------------------------------------------------------------------------------------------
# light_scenes' geometries with materials of their own: a coloured sphere, a glass sphere, a half-shiny sphere, a matte cream back
# triangle and a mirror triangle; the floor and the far wall coloured, the wall a little shiny
_SPHERE_MATS = ["color 0.8 0.3 0.2\n", "color 1 1 1\ntransparency 0.9\nior 1.5\n", "color 0.5 0.9 0.6\ntransparency 0\nshininess 0.3 0.1 0\n"]
_TRIANGLE_MATS = ["color 0.9 0.9 0.7\nshininess 0\n", "color 1 1 1\nshininess 1\n"]
_PLANES = "color 0.4 0.6 0.9\nplane 0 1 0 1\ncolor 0.7 0.7 0.3\nshininess 0.2\nplane 0 0 1 9\nshininess 0\n"


def material_scene(geometry, nlights, kind, w=light_scenes.W, h=light_scenes.H):
    """light_scenes.scene(geometry, nlights, kind) -- "mixed" or "mixed_planes" -- with the materials above."""
    assert geometry.split("_")[0] == "mixed"
    lines = light_scenes.GEOMETRY["mixed"].splitlines(keepends=True)
    body = []
    for i in range(3):
        body += [_SPHERE_MATS[i], lines[i]]
    for j in range(2):
        body += [_TRIANGLE_MATS[j]] + lines[3 + 4 * j:7 + 4 * j]
    return "".join([f"png {w} {h} indirect.png\n", light_scenes.lights(nlights, kind), _PLANES if geometry.endswith("_planes") else ""] + body)


# ---- header, library, wrappers -------------------------------------------------------------------------------------------------------
def test_the_header_takes_over_the_parameters_of_the_hemisphere_visibility():
    assert indirect.INDIRECT_SIGNATURES[NAME] == visibility.VISIBILITY_SIGNATURES["mirt_hemisphere_visibility"]


def test_a_library_without_the_symbol_is_an_error(monkeypatch):
    monkeypatch.setattr(binding, "lib", lambda: types.SimpleNamespace())
    with pytest.raises(binding.MirtError, match="does not export mirt_indirect_light"):
        indirect.lib()


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = types.SimpleNamespace(device=0, _h=None)
    F, D, out = torch.zeros((4, 8)), torch.zeros((16, 4)), torch.zeros((4, 4))
    mask, rot = torch.zeros(4, dtype=torch.int64), torch.zeros((4, 2))
    with pytest.raises(ValueError, match="dtype"):
        m.indirect_light(raw, F.double(), D, out)
    with pytest.raises(ValueError, match="dtype"):
        m.indirect_light(raw, F, D.double(), out)
    with pytest.raises(ValueError, match="shape"):
        m.indirect_light(raw, torch.zeros((4, 7)), D, out)
    with pytest.raises(ValueError, match="shape"):
        m.indirect_light(raw, F, torch.zeros((16, 3)), out)
    with pytest.raises(ValueError, match="1 to 64 rows"):
        m.indirect_light(raw, F, torch.zeros((65, 4)), out)
    with pytest.raises(ValueError, match="1 to 64 rows"):
        m.indirect_light(raw, F, torch.zeros((0, 4)), out)
    with pytest.raises(ValueError, match="shape"):
        m.indirect_light(raw, F, D, torch.zeros((5, 4)))
    with pytest.raises(ValueError, match="dtype"):
        m.indirect_light(raw, F, D, out, mask.int())
    with pytest.raises(ValueError, match="shape"):
        m.indirect_light(raw, F, D, out, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        m.indirect_light(raw, F, D, out, mask, torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="dtype"):
        m.indirect_light(raw, F, D, out, mask, rot.double())
    with pytest.raises(ValueError, match="contiguous"):
        m.indirect_light(raw, F, D, torch.zeros((4, 8))[:, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        m.indirect_light(raw, F, torch.zeros((16, 8))[:, ::2], out)
    with pytest.raises(ValueError, match="cuda"):
        m.indirect_light(raw, F, D, out, mask, rot)


# ---- code generation ----------------------------------------------------------------------------------------------------------------
def test_indirect_kernel_codegen_spills_nothing_and_keeps_scratch_for_the_stack_only():
    """indirect.hip compiled for gfx950: one kernel, no VGPR or SGPR spill, a 20-entry LDS stack per lane of a 256-thread block,
    the private segment of the query kernels (the stack's spill array and nothing else), and the register count and occupancy
    that DESIGN.md section 6m states."""
    res, _ = _resource_usage("indirect.hip")
    assert len(res) == 1 and "indirect_light_kernel" in list(res)[0], list(res)
    r = list(res.values())[0]
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 272, r
    assert r["LDS Size [bytes/block]"] == 20 * 256 * 4, r
    assert r["VGPRs"] == KERNEL_VGPRS and r["AGPRs"] == 0 and r["Occupancy [waves/SIMD]"] == KERNEL_WAVES_PER_SIMD, r
    query, _ = _resource_usage("query.hip")
    assert {query[k]["ScratchSize [bytes/lane]"] for k in query if "trace_rays_kernel" in k} == {r["ScratchSize [bytes/lane]"]}
    assert {query[k]["LDS Size [bytes/block]"] for k in query if "trace_rays_kernel" in k} == {r["LDS Size [bytes/block]"]}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("## 6m."):]
    assert f"{KERNEL_VGPRS} VGPRs" in section and f"{KERNEL_WAVES_PER_SIMD} waves per SIMD" in section


# ---- properties of the restatement --------------------------------------------------------------------------------------------------
def _rows(n, seed):
    rng = np.random.default_rng(seed)
    F = np.zeros((n, 8), f32)
    F[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    F[:, 3] = 1
    F[:, 4:7] = rng.normal(size=(n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1)))
    return F


def _never(rays):
    m_ = len(rays)
    return np.full(m_, -1, f32), np.zeros(m_, np.uint32), np.zeros(m_, np.uint32), np.zeros((m_, 3), f32)


def _lights(nsuns, nbulbs):
    suns, bulbs = np.zeros(nsuns, pyscene.LIGHT), np.zeros(nbulbs, pyscene.LIGHT)
    return suns, bulbs


@pytest.mark.parametrize("k", [1, 5, 16, 33, 64])
def test_nothing_in_reach_gives_the_butterfly_sum_of_the_weights_and_an_empty_mask(k):
    F = _rows(50, k)
    F[7, 3] = 0
    F[8, 3] = -2.5
    dirs = m.cosine_directions(k)
    dirs[:, 3] = np.random.default_rng(k).uniform(0.01, 1.0, k).astype(f32)      # (weights whose sum depends on the order)
    suns, bulbs = _lights(1, 1)
    suns["v"], suns["color"], bulbs["v"], bulbs["color"] = (0, 1, 0), (1, 1, 1), (0, 3, 0), (2, 2, 2)
    called = []
    out, mask = ir.indirect_light(F, dirs, m.rotations(50, 2), 0.75, suns, bulbs, np.ones((1, 11), f32), np.zeros((0, 11), f32), np.zeros((0, 11), f32),
                                  _never, lambda rays: called.append(len(rays)) or np.zeros(len(rays), bool))
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
    assert np.all(out[:, 0:3].view(np.uint32) == 0) and np.all(mask == 0)
    assert np.all(out[7].view(np.uint32) == 0)      # hit == 0: zeros
    # ... which is mirt_hemisphere_visibility's a channel when nothing is occluded
    vis, vis_mask = vr.hemisphere_visibility(F, dirs, m.rotations(50, 2), 0.75, np.zeros((50, k), bool))
    assert np.array_equal(vis[:, 3].view(np.uint32), out[:, 3].view(np.uint32))
    assert np.all((vis_mask ^ mask)[hit] == np.uint64(2 ** k - 1))


def test_one_sun_over_one_matte_white_plane_gives_the_butterfly_sum_of_w_lam_colour():
    """Every direction ends on the plane y = -1 (normal +y) under the sun (1, 2, 0.5) of colour (0.9, 0.5, 0.25), nothing in the
    sun's way: a term is w * (1 * (colour * lam)), lam = dot((0, 1, 0), normalize(sun))."""
    k = 33
    F = _rows(40, 3)
    dirs = m.cosine_directions(k)
    dirs[:, 3] = np.random.default_rng(1).uniform(0.01, 1.0, k).astype(f32)
    suns, bulbs = _lights(1, 0)
    suns["v"], suns["color"] = (1, 2, 0.5), (0.9, 0.5, 0.25)
    plane_mats = np.array([[1, 1, 1, 0, 0, 0, 0, 0, 0, 1.458, 0]], f32)

    def closest(rays):
        n_ = len(rays)
        return np.full(n_, 2.0, f32), np.full(n_, 3, np.uint32), np.zeros(n_, np.uint32), np.tile(np.array([0, 1, 0], f32), (n_, 1))

    seen = []

    def occluded(rays):
        seen.append(rays.copy())
        return np.zeros(len(rays), bool)

    out, mask = ir.indirect_light(F, dirs, None, np.inf, suns, bulbs, np.zeros((0, 11), f32), np.zeros((0, 11), f32), plane_mats, closest, occluded)
    lam = light_ref._dot(np.array([[0, 1, 0]], f32), light_ref._normalize(np.array([[1, 2, 0.5]], f32)))[0]
    colour = np.array([0.9, 0.5, 0.25], f32) * lam
    G = 64
    e = np.zeros((1, G, 3), f32)
    e[0, :k] = dirs[:, 3:4] * colour[None, :]
    want = vr.butterfly(e)[0]
    assert want.dtype == f32 and np.all(want > 0)
    assert np.all(out[:, 0:3].view(np.uint32) == want.view(np.uint32)[None, :]) and np.all(out[:, 3].view(np.uint32) == 0)
    assert np.all(mask == np.uint64(2 ** k - 1))
    # the shadow rays start a little above the hit point, which lies 2 along the gather ray
    gather_rays = vr.hemisphere_rays(F, dirs, None, np.inf).reshape(-1, 8)
    P2 = ir.hit_points(gather_rays, np.full(len(gather_rays), 2.0, f32))
    assert len(seen) == 1 and np.array_equal(seen[0][:, 0:3], P2 + np.array([0, 1, 0], f32) * f32(0.001)) and np.all(np.isinf(seen[0][:, 3]))
    # a mirror or a glass plane bounces nothing, a coloured one its colour
    for mat, factor in (([1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0], (0, 0, 0)), ([1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0], (0, 0, 0)),
                        ([0.5, 0.25, 1, 0, 0.5, 0, 0, 0, 0.5, 1, 0.3], (0.5, 0.125, 0.5))):
        got, _ = ir.indirect_light(F[:1], dirs[:1], None, np.inf, suns, bulbs, np.zeros((0, 11), f32), np.zeros((0, 11), f32), np.array([mat], f32), closest,
                                   occluded)
        assert np.array_equal(got[0, 0:3], dirs[0, 3] * (np.array(factor, f32) * colour))


# ---- the restatement decided twice ----------------------------------------------------------------------------------------------------
def _brute_force(sph, tri, pl, o, dirs):
    """test_gpu_queries.brute_force -- hitNearest (draw.cu:292-318) by testing every primitive with that file's restated
    intersections -- for a scene that may have no plane: (t, kind, id) per ray."""
    import test_gpu_queries as q
    d = q._normalize(dirs)
    n = len(o)
    prim = np.concatenate([q._sphere_t(o, d, sph["c"], sph["r"])[0], q._triangle_t(o, d, tri)[0]], axis=1)
    pj = np.argmin(prim, axis=1)
    tb = prim[np.arange(n), pj]
    if len(pl):
        tp = q._plane_t(o, d, pl)
        pk = np.argmin(tp, axis=1)
        tpl = tp[np.arange(n), pk]
    else:
        pk, tpl = np.zeros(n, np.int64), np.full(n, np.inf, f32)
    # the BVH's nearest, then the plane rule: the BVH hit wins only when strictly nearer
    use_b = np.isfinite(tb) & ~(np.isfinite(tpl) & ~(tb < tpl))
    hit = np.isfinite(tb) | np.isfinite(tpl)
    t = np.where(use_b, tb, np.where(hit, tpl, np.inf)).astype(f32)
    kind = np.where(use_b, np.where(pj < len(sph), 1, 2), np.where(hit, 3, 0)).astype(np.uint32)
    ident = np.where(use_b, np.where(pj < len(sph), pj, pj - len(sph)), np.where(hit, pk, 0)).astype(np.uint32)
    return t, kind, ident


def brute_force_callbacks(text):
    """(closest, occluded) for indirect_ref from the float32 brute force of test_gpu_queries: the reference's intersections
    restated in numpy over every primitive and plane, and the normals mirt_trace_rays reports for them."""
    stl = m.parseText(text)
    sph, tri, pl = stl.array("spheres"), stl.array("triangles"), stl.array("planes")

    def brute_force(o, dirs, chunk=8192):
        parts = [_brute_force(sph, tri, pl, o[a:a + chunk], dirs[a:a + chunk]) for a in range(0, len(o), chunk)]
        return [np.concatenate([p[i] for p in parts]) for i in range(3)] if parts else [np.zeros(0, f32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)]

    def closest(rays):
        rays = np.asarray(rays, f32)
        o, tmax = np.ascontiguousarray(rays[:, 0:3]), rays[:, 3]
        with np.errstate(all="ignore"):
            t, kind, ident = brute_force(o, np.ascontiguousarray(rays[:, 4:7]))
            d = light_ref._normalize(rays[:, 4:7].copy())
            kind = np.where(t < tmax, kind, 0).astype(np.uint32)
            n = np.zeros((len(rays), 3), f32)
            s = kind == 1
            if np.any(s):
                c, r = sph["c"][ident[s]], sph["r"][ident[s]]
                p = d[s] * t[s, None] + o[s]
                cr0 = c - o[s]
                inside = light_ref._dot(cr0, cr0) < r * r
                n[s] = light_ref._normalize(np.where(inside[:, None], c - p, p - c))
            for code, nor in ((2, tri["nor"]), (3, pl["nor"])):
                s = kind == code
                if np.any(s):
                    v = nor[ident[s]]
                    n[s] = np.where((light_ref._dot(d[s], v) < 0)[:, None], v, -v)
        return np.where(kind != 0, t, f32(-1)), kind, ident, n

    def occluded(rays):
        rays = np.asarray(rays, f32)
        with np.errstate(all="ignore"):
            t, _, _ = brute_force(np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 4:7]))
        return t < rays[:, 3]

    return closest, occluded


def arbiter_gather(sc, rays, dirs, radius):
    """Every gather ray [n, K, 8] of the restatement, and every shadow ray from what it hits, against every primitive and plane of
    the scene in float64 (f64_arbiter's intersections, which record the relative margin of each of their decisions):
    hit [n, K], the header's sum in float64 rgb [n, 3], and the smallest margin of a row's decisions -- every hit or miss, a
    hit's distance against the radius, a shadow hit's against the distance of the bulb."""
    a = arb.Arbiter(sc)
    n, K, _ = rays.shape
    hit = np.zeros((n, K), bool)
    rgb = np.zeros((n, 3))
    margin = np.full(n, np.inf)
    R = rays.astype(np.float64)
    W = np.asarray(dirs, np.float64)[:, 3]
    for i in range(n):
        a.margin, a.what = arb.INF, None
        o = tuple(R[i, 0, 0:3].tolist())
        for k in range(K):
            h = a.hit_nearest(o, arb._normalize(tuple(R[i, k, 4:7].tolist())), 1)
            if not h.is_hit:
                continue
            a._decide(arb._rel(h.t, radius), "hit within the radius")
            if not h.t < radius:
                continue
            hit[i, k] = True
            N = arb._normalize(h.n)
            so = arb._add(h.p, arb._mul(h.n, arb.EPSILON))
            D = [0.0, 0.0, 0.0]
            for ldir, lc in a.suns:
                ld = arb._normalize(ldir)
                lam = arb._dot(N, ld)
                if not lam > 0.0:
                    continue
                if a.hit_nearest(so, ld, 1).is_hit:
                    continue
                D = [D[c] + lc[c] * lam for c in range(3)]
            for lp, lc in a.bulbs:
                bd = arb._sub(lp, h.p)
                dist = arb._length(bd)
                L = arb._normalize(bd)
                lam = arb._dot(N, L)
                if not lam > 0.0:
                    continue
                sh = a.hit_nearest(so, L, 1)
                if sh.is_hit:
                    a._decide(arb._rel(sh.t, dist), "shadow hit before the light")
                    if sh.t < dist:
                        continue
                D = [D[c] + lc[c] * lam / (dist * dist) for c in range(3)]
            mat = h.mat
            for c in range(3):
                rgb[i, c] += W[k] * ((1.0 - mat["shine"][c]) * (1.0 - mat["trans"][c]) * mat["color"][c] * D[c])
        margin[i] = a.margin
    return hit, rgb, margin


@functools.lru_cache(maxsize=None)
def _oracle_rows(geometry):
    """The first hits of the pinhole rays of the geometry at 40 x 30, as test_light_abi makes them, and probe points for the
    geometry without planes, whose frame is mostly sky."""
    w, h = light_scenes.W, light_scenes.H
    text = material_scene(geometry, 3, "mixed")
    sc = pyscene.parse_lines(text.split("\n"))
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        ref = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)
    finally:
        o.close()
    F = dr.features(_pinhole_rays(sc, w, h), np.ascontiguousarray(ref["aov"]).reshape(-1).view(np.uint32).reshape(-1, 6))
    return text, sc, np.ascontiguousarray(F, f32)


def arbiter_rows(F):
    """The hit rows of a frame's features, at most 400 of them, evenly spread."""
    F = F[F[:, 3] != 0]
    step = max(1, len(F) // 400)
    return np.ascontiguousarray(F[::step][:400])


@pytest.mark.parametrize("geometry,k,radius", ARBITER_CASES)
def test_restatement_decided_in_float64_and_in_float32_gives_the_same_result(geometry, k, radius):
    """The restatement for first-hit rows of the scene with three mixed lights, cosine_directions(k) and rotations(n, 1), decided
    by the float32 brute force of test_gpu_queries, against the same sum made in float64 by f64_arbiter.  On every row whose
    decisions -- every gather ray's and every shadow ray's -- are clear of f64_arbiter.CLEAR the hit masks are the same and rgb
    agrees within RGB_TOLERANCE; at most 10 % of the rows may be left out.  Measured here: 252, 252, 395 and 393 of 254, 254, 400
    and 400 rows clear, no mask differing, |rgb32 - rgb64| at most 3.21e-8, 3.21e-8, 5.65e-8 and 6.2e-8 (rgb up to 0.66); the
    bound asserted is 8 x the largest, 4.97e-7."""
    text, sc, frame = _oracle_rows(geometry)
    F = arbiter_rows(frame)
    n = len(F)
    dirs, rot = m.cosine_directions(k), m.rotations(n, 1)
    rays = vr.hemisphere_rays(F, dirs, rot, radius)
    hit64, rgb64, margin = arbiter_gather(sc, rays, dirs, radius)
    mask64 = (hit64.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    closest, occluded = brute_force_callbacks(text)
    stl = m.parseText(text)
    mats = [np.ascontiguousarray(stl.array(name)["mat"]).view(f32).reshape(-1, 11) for name in ("spheres", "triangles", "planes")]
    suns, bulbs = stl.array("suns"), stl.array("bulbs")
    out32, mask32 = ir.indirect_light(F, dirs, rot, radius, suns, bulbs, mats[0], mats[1], mats[2], closest, occluded)
    clear = margin > arb.CLEAR
    worst = float(np.abs(out32[clear, 0:3].astype(np.float64) - rgb64[clear]).max())
    print(f"{geometry} K {k} radius {radius}: {n} rows, {clear.sum()} clear, hit ray share {hit64.mean():.3f}, "
          f"rows with another mask {int((mask64 != mask32).sum())}, largest rgb {rgb64[clear].max():.4f}, worst |rgb32 - rgb64| {worst:.3g}")
    assert n >= 100 and clear.sum() >= 0.9 * n, (n, int(clear.sum()))
    assert np.array_equal(mask64[clear], mask32[clear])
    assert worst <= RGB_TOLERANCE, worst
    assert 0.05 < hit64.mean() and len(set(mask64[clear].tolist())) > 3 and rgb64[clear].max() > 0.01
    assert np.all(out32[:, 0:3] >= 0) and np.all(out32[:, 3] >= 0) and np.all(out32[:, 3] <= 1 + 1e-6)

"""Unit tests of the oracle's parts (no GPU): RNG, deterministic math, LBVH validity, invariances."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol


# ---------------------------------------------------------------- XORWOW ----
def _step(v):
    t = (v[0] ^ (v[0] >> 2)) & 0xFFFFFFFF
    v = [v[1], v[2], v[3], v[4], ((v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))) & 0xFFFFFFFF]
    return v


def test_xorwow_seeding_and_stepping_follow_the_published_algorithm():
    seed = 1234
    s0 = (seed & 0xFFFFFFFF) ^ 0xaad26b49
    s1 = (seed >> 32) ^ 0xf7dcefdd
    t0 = (1099087573 * s0) & 0xFFFFFFFF
    t1 = (2591861531 * s1) & 0xFFFFFFFF
    d = (6615241 + t1 + t0) & 0xFFFFFFFF
    v = [(123456789 + t0) & 0xFFFFFFFF, 362436069 ^ t0, (521288629 + t1) & 0xFFFFFFFF, 88675123 ^ t1, (5783321 + t0) & 0xFFFFFFFF]
    want = []
    for _ in range(8):
        v = _step(v)
        d = (d + 362437) & 0xFFFFFFFF
        want.append((v[4] + d) & 0xFFFFFFFF)
    got = np.zeros(8, np.uint32)
    ol.lib().orc_xorwow_seq(seed, 0, 0, 8, got.ctypes.data)
    assert got.tolist() == want


def test_sequence_jump_matrix_equals_rocrands_precomputed_table():
    """The recurrence and the 2^67 jump are the same in rocRAND (only seeding/uniform mapping differ), so its
    precomputed matrix cross-checks the oracle's own 67 squarings.  The first matrix of rocRAND's
    h_xorwow_sequence_jump_matrices is stored in tests/golden/xorwow_jump_matrix0.npy; where the rocRAND header is
    installed, the stored copy is checked against it as well."""
    vals = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xorwow_jump_matrix0.npy"))
    assert vals.dtype == np.uint32 and vals.shape == (800,)
    hdr = "/opt/rocm/include/rocrand/rocrand_xorwow_precomputed.h"
    if os.path.exists(hdr):
        txt = open(hdr).read()
        m = re.search(r"h_xorwow_sequence_jump_matrices\s*\[[^\]]*\]\s*\[[^\]]*\]\s*=\s*\{\s*\{(.*?)\}", txt, re.S)
        assert m, "table not found"
        hv = np.array([int(x, 0) for x in re.findall(r"0x[0-9a-fA-F]+|\d+", m.group(1))][:800], dtype=np.uint32)
        assert np.array_equal(hv, vals)
    mine = np.zeros(800, np.uint32)
    ol.lib().orc_jump_matrix(0, mine.ctypes.data)       # column-major: col[word i*32 + bit j][k]
    assert np.array_equal(mine, vals)


def test_subsequence_jumps_compose():
    st = lambda sub: (lambda a: (ol.lib().orc_xorwow_state(99, sub, a.ctypes.data), a)[1])(np.zeros(6, np.uint32))
    a, b = st(5), st(12)
    assert not np.array_equal(a, b)
    # jump(5) then jump(7) == jump(12): apply matrix pow2 decomposition manually through the API
    cols = np.zeros((160, 5), np.uint32)

    def apply(k, v):
        ol.lib().orc_jump_matrix(k, cols.ctypes.data)
        out = np.zeros(5, np.uint32)
        for w in range(5):
            for bit in range(32):
                if (int(v[w]) >> bit) & 1:
                    out ^= cols[w * 32 + bit]
        return out
    v = a[:5].copy()
    for k in (0, 1, 2):          # 7 = 1 + 2 + 4
        v = apply(k, v)
    assert np.array_equal(v, b[:5]) and a[5] == b[5]


def test_uniform_and_normal_ranges():
    out = np.zeros(20000 + 20000, np.float32)
    ol.lib().orc_xorwow_floats(1234, 3, 20000, 20000, out.ctypes.data)
    u, n = out[:20000], out[20000:]
    assert u.min() > 0.0 and u.max() <= 1.0 and abs(u.mean() - 0.5) < 0.01
    assert abs(n.mean()) < 0.03 and abs(n.std() - 1.0) < 0.03


# ------------------------------------------------------- deterministic math ----
@pytest.mark.parametrize("which,fn,lo,hi,ulps,abs_tol", [
    (0, np.log, 1e-10, 10.0, 2.0, None), (1, np.exp, -40.0, 10.0, 1.5, None),            # single-precision forms: CUDA libm's accuracy class
    (2, np.sin, -7.0, 7.0, None, 1.2e-7), (3, np.cos, -7.0, 7.0, None, 1.2e-7),          # (absolute: the relative error is unbounded at the zeros)
    (4, lambda x: np.power(x, float(np.float32(1) / np.float32(2.4))), 0.0, 4.0, 0.51, None),   # double-based, rounded once (the sRGB curve)
    (6, np.sqrt, 0.0, 1e6, 0.51, None)])
def test_math_accuracy_against_a_float64_reference(which, fn, lo, hi, ulps, abs_tol):
    x = np.random.default_rng(which).uniform(lo, hi, 200000).astype(np.float32)
    got = np.zeros_like(x)
    ol.lib().orc_math_probe(which, x.size, x.ctypes.data, got.ctypes.data)
    want = fn(x.astype(np.float64))
    if abs_tol is not None:
        assert np.abs(got.astype(np.float64) - want).max() <= abs_tol
        return
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / np.maximum(ulp, 1e-300)
    assert err.max() <= ulps, err.max()


def test_math_edge_values():
    x = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, -1.0], np.float32)
    out = np.zeros_like(x)
    ol.lib().orc_math_probe(0, x.size, x.ctypes.data, out.ctypes.data)      # logf
    assert out[0] == -np.inf and out[1] == -np.inf and out[2] == 0.0 and out[3] == np.inf and np.isnan(out[4]) and np.isnan(out[5]) and np.isnan(out[8])
    assert abs(out[6] - np.log(1.401298464e-45)) < 1e-4 and abs(out[7] - np.log(3.4e38)) < 1e-4
    y = np.array([0.0, -0.0, 88.8, -104.0, -87.5, 88.0, np.nan, np.inf, -np.inf], np.float32)
    ol.lib().orc_math_probe(1, y.size, y.ctypes.data, out.ctypes.data)      # expf
    assert out[0] == 1.0 and out[1] == 1.0 and out[2] == np.inf and out[3] == 0.0 and np.isnan(out[6]) and out[7] == np.inf and out[8] == 0.0
    assert abs(out[4] / np.exp(-87.5) - 1) < 1e-5 and abs(out[5] / np.exp(88.0) - 1) < 1e-6
    z = np.array([0.0, np.pi / 2, np.pi, -np.pi / 2, 2 * np.pi, np.inf, np.nan], np.float32)
    ol.lib().orc_math_probe(2, z.size, z.ctypes.data, out.ctypes.data)      # sinf
    assert out[0] == 0.0 and abs(out[1] - 1) < 1e-7 and abs(out[2]) < 2e-7 and abs(out[3] + 1) < 1e-7 and abs(out[4]) < 4e-7 and np.isnan(out[5]) and np.isnan(out[6])


def test_srgb_curve_endpoints():
    x = np.array([-1.0, 0.0, 0.0031307, 0.0031308, 0.5, 1.0, 2.0, np.nan, np.inf], np.float32)
    y = np.zeros_like(x)
    ol.lib().orc_math_probe(5, x.size, x.ctypes.data, y.ctypes.data)
    assert y[0] == 0 and y[1] == 0 and abs(y[5] - 1.0) < 1e-6 and y[6] == 1.0 and y[7] == 0.0 and y[8] == 1.0
    assert abs(y[4] - 0.7353569) < 1e-6


# ----------------------------------------------------------------- LBVH ----
@pytest.mark.parametrize("name", ["tri", "redchair", "spiral", "tenthousand"])
def test_tree_is_a_valid_bvh(name, oracle_scenes):
    o = oracle_scenes(name)
    nd, codes, n = o.nodes(), o.codes(), o.n
    assert len(nd) == 2 * n - 1
    assert np.all(np.diff(codes.astype(np.int64)) >= 0)
    seen = np.zeros(2 * n - 1, np.int32)
    stack = [0]
    depth = {0: 0}
    while stack:
        i = stack.pop()
        seen[i] += 1
        if nd[i]["count"] == 0:
            for c in (int(nd[i]["left"]), int(nd[i]["right"])):
                assert nd[c]["xmin"] >= nd[i]["xmin"] and nd[c]["xmax"] <= nd[i]["xmax"]
                assert nd[c]["ymin"] >= nd[i]["ymin"] and nd[c]["ymax"] <= nd[i]["ymax"]
                assert nd[c]["zmin"] >= nd[i]["zmin"] and nd[c]["zmax"] <= nd[i]["zmax"]
                depth[c] = depth[i] + 1
                stack.append(c)
    assert np.all(seen == 1)                       # every node reached exactly once
    assert sorted(int(x) for x in nd[n - 1:]["prim_offset"]) == list(range(n))
    assert max(depth.values()) < 64


def test_duplicate_morton_codes_keep_file_order(oracle_scenes):
    """thrust::sort_by_key is stable (lbvh_utils.cu:110); spiral.txt has duplicate codes."""
    o = oracle_scenes("spiral")
    codes, refs = o.codes(), o.refs()
    dup = np.flatnonzero(codes[1:] == codes[:-1])
    assert len(dup) > 0
    assert np.all(refs["id"][dup + 1] > refs["id"][dup])


def test_morton_code_corners():
    mn, mx = np.zeros(3, np.float32), np.ones(3, np.float32)
    f = lambda x, y, z: ol.lib().orc_morton(x, y, z, mn.ctypes.data, mx.ctypes.data)
    assert f(0, 0, 0) == 0 and f(1, 1, 1) == 0x3FFFFFFF
    assert f(1, 0, 0) == 0x09249249 and f(0, 1, 0) == 0x12492492 and f(0, 0, 1) == 0x24924924
    assert f(-5, 9, 0.5) == (0x12492492 | (0x24924924 & ol.lib().orc_morton(0, 0, 0.5, mn.ctypes.data, mx.ctypes.data)))


# ----------------------------------------------------------- invariances ----
@pytest.mark.parametrize("name,spp", [("tenthousand", 16), ("redchair", 32), ("spiral", 1)])
def test_any_hit_shadow_rays_give_the_same_image(name, spp, oracle_scenes):
    o = oracle_scenes(name)
    a = o.render(64, 36, spp, nthreads=8)
    b = o.render(64, 36, spp, flags=ol.FLAG_ANYHIT_SHADOW, nthreads=8)
    assert np.array_equal(a["f32"].view(np.uint32), b["f32"].view(np.uint32))
    assert a["stats"]["rays"] == b["stats"]["rays"]
    assert b["stats"]["internal_visits"] < a["stats"]["internal_visits"]


@pytest.mark.parametrize("name,w,h,spp", [("tenthousand", 64, 36, 16), ("spiral", 64, 36, 4), ("redchair", 48, 27, 32), ("tri", 128, 128, 0)])
def test_the_mirror_of_the_products_default_mode_gives_the_image_of_the_reference_walk(name, w, h, spp, oracle_scenes):
    """The link between the two halves of the parity chain.  GPU tests compare libmirt with the oracle run under the flags that
    mirror the product's default mode (any-hit shadow rays, unlit shadow rays skipped, near child first where it cannot change
    the hit, quantised boxes on sphere-only scenes).  Here that mirror is compared with the oracle's plain restatement of the
    reference (flags = 0: left-first walk, every shadow ray traced to its nearest hit): same float image bit for bit, same
    rays, fewer node visits."""
    o = oracle_scenes(name)
    plain = o.render(w, h, spp, flags=0, nthreads=8)
    mirror = o.render(w, h, spp, flags=ol.product_flags(name in ("redchair", "tri")), nthreads=8)
    assert np.array_equal(plain["f32"].view(np.uint32), mirror["f32"].view(np.uint32))
    assert np.array_equal(plain["u8"], mirror["u8"])
    assert plain["stats"]["rays"] == mirror["stats"]["rays"]
    assert mirror["stats"]["internal_visits"] <= plain["stats"]["internal_visits"]


@pytest.mark.parametrize("scene", ["bulbs_and_planes", "fisheye", "panorama", "glass_gi_dof", "glass_spheres_bulb", "axis_parallel_rays", "far_camera"])
@pytest.mark.parametrize("spp", [0, 4])
def test_the_mirror_equals_the_reference_walk_on_the_edge_scenes(scene, spp):
    """The same on the synthetic edge cases: point lights, glass + gi, rays with zero direction components inside the scene's
    bounds, a camera 30 000 scene sizes away."""
    import edge_scenes
    import pyscene
    text = edge_scenes.far_camera() if scene == "far_camera" else edge_scenes.ALL[scene]()
    sc = pyscene.parse_lines(text.split("\n"))
    o = ol.OracleScene(sc, bounds_mode=0)
    w, h = 64, 48
    plain = o.render(w, h, spp, flags=0, nthreads=8)
    mirror = o.render(w, h, spp, flags=ol.product_flags(any(l.startswith("tri ") for l in text.split("\n"))), nthreads=8)
    o.close()
    both_nan = np.isnan(plain["f32"]) & np.isnan(mirror["f32"])
    assert np.array_equal(np.where(both_nan, 0, plain["f32"].view(np.uint32)), np.where(both_nan, 0, mirror["f32"].view(np.uint32)))
    assert np.array_equal(plain["u8"], mirror["u8"])
    assert plain["stats"]["rays"] == mirror["stats"]["rays"]


@pytest.mark.parametrize("name,w,h,spp", [("redchair", 96, 54, 8), ("tri", 128, 128, 0), ("tenthousand", 48, 27, 4)])
def test_quantised_and_wide_walks_give_the_image_of_the_reference_walk(name, w, h, spp, oracle_scenes):
    """qnodes = 2 on the GPU side: the oracle's mirrors of the quantised walk on a scene with triangles (ORC_FLAG_QNODES: a
    triangle hit the reference's walk may not reach re-walks the exact boxes) and of the wide walk (ORC_FLAG_WIDE: the boxes of a
    node's four grandchildren per step, the reference's order) against the plain restatement: same float image bit for bit, same
    rays; the wide walk takes about half the steps; the re-walk rule fires on redchair.txt's silhouettes and nowhere on a
    sphere-only scene."""
    o = oracle_scenes(name)
    plain = o.render(w, h, spp, flags=0, nthreads=8)
    q = o.render(w, h, spp, flags=ol.PRODUCT_FLAGS, nthreads=8)
    wide = o.render(w, h, spp, flags=ol.PRODUCT_FLAGS_TRI, nthreads=8)
    for m in (q, wide):
        assert np.array_equal(plain["f32"].view(np.uint32), m["f32"].view(np.uint32))
        assert plain["stats"]["rays"] == m["stats"]["rays"]
    assert wide["stats"]["internal_visits"] < 0.75 * q["stats"]["internal_visits"]
    assert wide["stats"]["qn_retraces"] == q["stats"]["qn_retraces"]
    if name == "redchair":
        assert q["stats"]["qn_retraces"] > 0
    if name == "tenthousand":
        assert q["stats"]["qn_retraces"] == 0


def test_a_hit_below_the_entry_distance_of_its_own_box_is_vetted():
    """tests/golden/far_camera_tie.txt, pixel (50, 97) of a 192x108 frame: two overlapping spheres 4 256 units from the camera
    are hit within one ulp of t (4256.1167 and 4256.11719).  The reference's walk meets the farther one first and then culls
    the leaf box of the nearer one (its entry distance rounds above the best distance), so it shades the farther sphere; a walk
    over the quantised boxes reaches the nearer one, shades it, and traces one ray more (found by tools/fuzz_modes.py: seed 47,
    scene 795; the pixel is black either way).  With ORC_FLAG_REACH (the product's hit_needs_literal_walk) the hit is recognised
    as one the reference may not reach and the ray is walked again literally: counters and image of the plain restatement."""
    import os
    import pyscene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "far_camera_tie.txt")
    o = ol.OracleScene(pyscene.parse_lines(open(path).read().split("\n")), bounds_mode=0)
    tile = (50, 97, 1, 1)
    plain = o.render(192, 108, 0, tile=tile, flags=0)
    unvetted = o.render(192, 108, 0, tile=tile, flags=ol.PRODUCT_FLAGS & ~ol.FLAG_REACH)
    vetted = o.render(192, 108, 0, tile=tile, flags=ol.PRODUCT_FLAGS)
    assert unvetted["stats"]["rays"] == plain["stats"]["rays"] + 1 and unvetted["stats"]["qn_retraces"] == 0
    assert vetted["stats"]["rays"] == plain["stats"]["rays"] and vetted["stats"]["qn_retraces"] == 1
    whole = [o.render(192, 108, 0, flags=f, nthreads=8) for f in (0, ol.PRODUCT_FLAGS, ol.PRODUCT_FLAGS_TRI, ol.PRODUCT_FLAGS_SMALL_TRI)]
    for m in whole[1:]:
        assert np.array_equal(whole[0]["f32"].view(np.uint32), m["f32"].view(np.uint32))
        for k in ("rays", "shadow_rays", "mat_fetches"):
            assert whole[0]["stats"][k] == m["stats"][k], k


def test_a_shadow_ray_to_a_point_light_from_very_far_away_is_vetted():
    """tests/golden/far_plane_point_light.txt (three spheres of tools/fuzz_modes.py --offset --far, seed 72, scene 2868), pixel
    (144, 65) of a 192x108 frame at 2 spp: a panorama ray hits the infinite plane 1.2e8 units away; from there the point light
    and the two large spheres around it are all 121 323 3xx units away, ulp(t) = 8.  "Occluded" means nearer than the light: the
    reference's walk ends with one sphere at t = ...344 (not nearer), the walk over the quantised boxes with the other at
    t = ...328 (nearer) -- a hit the reference never tests -- and the pixel turns black.  With ORC_FLAG_REACH such shadow
    queries are traced to their nearest hit and vetted like every shaded hit: image and ray count of the plain restatement."""
    import os
    import pyscene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "far_plane_point_light.txt")
    o = ol.OracleScene(pyscene.parse_lines(open(path).read().split("\n")), bounds_mode=0)
    assert o.grid_ok()
    tile = (144, 65, 1, 1)
    plain = o.render(192, 108, 2, tile=tile, flags=0)
    unvetted = o.render(192, 108, 2, tile=tile, flags=ol.PRODUCT_FLAGS & ~ol.FLAG_REACH)
    vetted = o.render(192, 108, 2, tile=tile, flags=ol.PRODUCT_FLAGS)
    assert not np.array_equal(plain["f32"], unvetted["f32"]) and np.array_equal(plain["f32"].view(np.uint32), vetted["f32"].view(np.uint32))
    assert vetted["stats"]["qn_retraces"] >= 1 and vetted["stats"]["rays"] == plain["stats"]["rays"]
    whole_plain, whole = o.render(192, 108, 2, flags=0, nthreads=8), o.render(192, 108, 2, flags=ol.PRODUCT_FLAGS, nthreads=8)
    assert np.array_equal(whole_plain["f32"].view(np.uint32), whole["f32"].view(np.uint32)) and whole_plain["stats"]["rays"] == whole["stats"]["rays"]


def test_far_camera_scenes_vetted_walk_equals_the_plain_restatement():
    """The regime of the finding above, at random (tools/fuzz_scenes.py, far = True: cameras 10^3 .. 10^5 scene sizes away, many
    large overlapping spheres): the mirror of the product's default mode, vetting included, gives the float image and the ray
    count of the plain restatement on every scene, and the vetting is at work (rays are walked again).  On 300 such scenes at
    192x108 the oracle counts 1 679 re-walks in 6.1e7 rays and one scene whose unvetted ray count differs; on the GPU,
    7 000 of them against the reference-walk mode: no differing byte or ray count (tools/r03_fuzz3.sh)."""
    import os
    import sys
    import pyscene
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    from fuzz_scenes import scene_text
    rng = np.random.default_rng(61)
    rewalks = 0
    for _ in range(40):
        text = scene_text(rng, 0.0, True)
        spp = int(rng.choice([0, 1, 2, 4]))
        o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
        plain = o.render(96, 54, spp, flags=0, nthreads=8)
        mirror = o.render(96, 54, spp, flags=ol.PRODUCT_FLAGS, nthreads=8)
        o.close()
        both_nan = np.isnan(plain["f32"]) & np.isnan(mirror["f32"])
        assert np.array_equal(np.where(both_nan, 0, plain["f32"].view(np.uint32)), np.where(both_nan, 0, mirror["f32"].view(np.uint32)))
        assert plain["stats"]["rays"] == mirror["stats"]["rays"]
        rewalks += mirror["stats"]["qn_retraces"]
    assert rewalks > 0


def test_a_zero_direction_component_does_not_switch_an_axis_off_in_the_quantised_walk(oracle_scenes):
    """redchair.txt's `sun 0 1 2` has a zero x component.  Rounds 1-2 ignored such an axis in the quantised box test (a superset,
    so still exact) and every shadow ray of that sun then tested two axes only; the reciprocal is clamped instead.  The quantised
    walk must stay within a few per cent of the exact boxes' node visits."""
    o = oracle_scenes("redchair")
    exact = o.render(96, 54, 4, flags=ol.PRODUCT_ALWAYS | ol.FLAG_ORDERED, nthreads=8)["stats"]
    quant = o.render(96, 54, 4, flags=ol.PRODUCT_FLAGS, nthreads=8)["stats"]
    assert exact["internal_visits"] <= quant["internal_visits"] < 1.08 * exact["internal_visits"]


def test_tiles_and_threads_do_not_change_pixels(oracle_scenes):
    o = oracle_scenes("tenthousand")
    whole = o.render(50, 30, 16, nthreads=1)["f32"]
    parts = np.zeros_like(whole)
    for (x0, y0, tw, th) in [(0, 0, 20, 30), (20, 0, 30, 11), (20, 11, 30, 19)]:
        parts[y0:y0 + th, x0:x0 + tw] = o.render(50, 30, 16, tile=(x0, y0, tw, th), nthreads=8)["f32"]
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))


def test_struct_sizes_match_the_reference():
    want = {0: 44, 1: 60, 2: 116, 3: 84, 4: 24, 5: 8}
    for k, v in want.items():
        assert ol.lib().orc_sizeof(k) == v


def test_accumulate_in_one_pass_equals_render(oracle_scenes):
    """orc_render_accumulate + orc_finalize (render_kernel_atomic_aa + finalize_kernel, draw.cu:13-92) over all samples at once
    is the same sum tree as the warp kernel (draw.cu:135-213): identical 8-bit image; two passes agree within rounding."""
    o = oracle_scenes("tenthousand")
    w, h, spp = 40, 24, 16
    r = o.render(w, h, spp, nthreads=8)
    acc = np.zeros((h, w, 4), np.float32)
    o.render_accumulate(acc, w, h, 0, spp, nthreads=8)
    assert np.array_equal(ol.OracleScene.finalize(acc, spp), r["u8"])
    acc2 = np.zeros((h, w, 4), np.float32)
    o.render_accumulate(acc2, w, h, 0, 8, nthreads=8)
    o.render_accumulate(acc2, w, h, 8, 8, nthreads=8)
    assert np.max(np.abs(acc2 - acc)) <= 1e-4 * spp

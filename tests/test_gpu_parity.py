"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same inputs."""
import os
import sys

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import oracle_lib as ol

pytestmark = pytest.mark.gpu


class options:
    """Temporarily set scene options on a (session-cached) device scene."""

    def __init__(self, raw, rebuild=False, **kv):
        self.raw, self.kv, self.rebuild = raw, kv, rebuild

    def __enter__(self):
        self.old = {k: self.raw.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            self.raw.set_option(k, v)
        if self.rebuild:
            m.build_lbvh_karas(self.raw)
        return self.raw

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.raw.set_option(k, v)
        if self.rebuild:
            m.build_lbvh_karas(self.raw)

TOL = 1e-4   # north_star: output pixels within 1e-4 per channel (linear float RGBA before quantisation)
COUNTER_KEYS = ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack")


def gpu_render(raw, w, h, spp, stripe_rows=None, num_parts=1, part=0, counters=False):
    p = api.render_params(w, h, spp, stripe_rows, num_parts, part, counters)
    n = api.num_pixels(p)
    img = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
    flt = torch.empty(n * 4, dtype=torch.float32, device="cuda")
    m.render(img, w, h, spp, raw, d_float=flt, params=p)
    torch.cuda.synchronize()
    return img.cpu().numpy().reshape(-1, 4), flt.cpu().numpy().reshape(-1, 4)


@pytest.mark.parametrize("which,lo,hi", [(0, 1e-10, 1.0), (1, -30.0, 5.0), (2, -7.0, 7.0), (3, -7.0, 7.0), (4, 0.0, 4.0), (5, -0.5, 2.0), (6, 0.0, 100.0), (7, -10.0, 10.0)])
def test_device_math_is_bit_identical_to_oracle(which, lo, hi):
    rng = np.random.default_rng(which)
    x = rng.uniform(lo, hi, 1 << 18).astype(np.float32)
    x[:8] = [0.0, 1.0, 0.5, 0.0031308, 1e-30, 3.0, np.float32(lo), np.float32(hi)]
    want = np.zeros_like(x)
    ol.lib().orc_math_probe(which, x.size, x.ctypes.data, want.ctypes.data)
    got = api.probe_math(which, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("spp,streams", [(16, 16 * 300), (32, 32 * 64), (128, 128 * 8), (1, 70000), (0, 1000)])
def test_xorwow_streams_match_oracle(spp, streams):
    got = api.probe_xorwow(spp, streams, 6)
    want = np.zeros(6, np.uint32)
    idx = np.unique(np.concatenate([np.arange(0, min(streams, 40)), np.random.default_rng(1).integers(0, streams, 200)]))
    for i in idx:
        if spp > 1:
            ol.lib().orc_xorwow_seq(1234 + int(i) // spp, int(i) % spp, 0, 6, want.ctypes.data)
        else:
            ol.lib().orc_xorwow_seq(1234, int(i), 0, 6, want.ctypes.data)
        assert np.array_equal(got[i], want), (spp, i)


@pytest.mark.parametrize("name", ["tri", "redchair", "spiral", "tenthousand"])
def test_lbvh_is_identical_to_oracle(name, gpu_scenes, oracle_scenes):
    stl, raw = gpu_scenes(name)
    o = oracle_scenes(name)
    nodes, codes, refs, bounds = raw.tree()
    mn, mx = o.bounds()
    assert np.array_equal(bounds[:3], mn) and np.array_equal(bounds[3:], mx)
    assert np.array_equal(codes, o.codes())
    orefs = o.refs()
    assert np.array_equal(refs["type"], orefs["type"]) and np.array_equal(refs["id"], orefs["id"])
    on = o.nodes()
    for f in ("left", "right", "prim_offset", "count"):
        assert np.array_equal(nodes[f], on[f]), f
    for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"):
        assert np.array_equal(nodes[f].view(np.uint32), on[f].view(np.uint32)), f


def check_image(gu8, gf, ref, tol=TOL):
    of, ou8 = ref["f32"].reshape(-1, 4), ref["u8"].reshape(-1, 4)
    d = np.abs(gf.astype(np.float64) - of.astype(np.float64))
    d = np.where(np.isnan(gf) & np.isnan(of), 0.0, d)
    assert np.nanmax(d) <= tol, f"max float diff {np.nanmax(d)} at pixel {np.unravel_index(np.nanargmax(d), d.shape)}"
    assert np.array_equal(np.isnan(gf), np.isnan(of))
    du = np.abs(gu8.astype(np.int32) - ou8.astype(np.int32))
    assert du.max() <= 1, f"u8 diff {du.max()}"
    return float(np.nanmax(d)), int(du.max())


def test_tri_256_aa0_matches_oracle_and_golden_pixels(gpu_scenes, oracle_scenes):
    stl, raw = gpu_scenes("tri")
    gu8, gf = gpu_render(raw, 256, 256, 0)
    ref = oracle_scenes("tri").render(256, 256, 0)
    check_image(gu8, gf, ref)
    img = gu8.reshape(256, 256, 4)
    # SURVEY.md 8c pixel values (x, y)
    assert img[128, 64].tolist() == [188, 138, 0, 255]
    assert img[128, 128].tolist() == [238, 238, 238, 255]
    assert img[192, 64].tolist() == [188, 138, 0, 255]
    assert img[192, 128].tolist() == [0, 0, 0, 255]
    assert img[64, 64].tolist() == [0, 0, 0, 0]
    assert int((img[..., 3] > 0).sum()) == 20555


@pytest.mark.parametrize("name,w,h,spp", [
    ("tri", 100, 100, 1), ("tri", 64, 64, 4),
    ("redchair", 96, 54, 0), ("redchair", 96, 54, 1), ("redchair", 64, 36, 32), ("redchair", 48, 27, 20),
    ("spiral", 160, 90, 1), ("spiral", 96, 54, 16),
    ("tenthousand", 160, 90, 1), ("tenthousand", 96, 54, 16), ("tenthousand", 40, 30, 40),
    ("spiral", 24, 16, 100),      # next power of two > 64: the per-pixel fallback of the sample resolve
])
def test_small_frames_match_oracle(name, w, h, spp, gpu_scenes, oracle_scenes):
    stl, raw = gpu_scenes(name)
    gu8, gf = gpu_render(raw, w, h, spp, counters=True)
    st = raw.stats()
    ref = oracle_scenes(name).render(w, h, spp, flags=ol.product_flags(stl.num_triangles > 0), nthreads=8)
    check_image(gu8, gf, ref)
    os_ = ref["stats"]
    for k in ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack"):
        assert st[k] == os_[k], (k, st[k], os_[k])


@pytest.mark.parametrize("name,spp", [("tenthousand", 16), ("spiral", 16)])
def test_full_size_stripes_match_oracle(name, spp, gpu_scenes, oracle_scenes):
    """1920x1080 at the bench's spp: the GPU renders 3 four-row stripes of the full frame; the oracle the same rows."""
    stl, raw = gpu_scenes(name)
    w, h, rows = 1920, 1080, 2
    parts = h // rows // 3          # 180 parts -> part k owns stripes k, k+180, k+360
    part = 97
    gu8, gf = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part)
    o = oracle_scenes(name)
    refs = [o.render(w, h, spp, tile=(0, (part + j * parts) * rows, w, rows), flags=ol.PRODUCT_FLAGS, nthreads=8) for j in range(3)]
    ref = dict(f32=np.concatenate([r["f32"].reshape(-1, 4) for r in refs]), u8=np.concatenate([r["u8"].reshape(-1, 4) for r in refs]))
    check_image(gu8, gf, ref)


def test_config4_redchair_4k_64spp_stripes_match_oracle(gpu_scenes, oracle_scenes):
    """BASELINE config 4 (redchair.txt 3840x2160 at 64 spp): two 2-row stripes of the full-size frame against the oracle."""
    stl, raw = gpu_scenes("redchair")
    w, h, spp, rows = 3840, 2160, 64, 2
    parts = h // rows // 2          # 540 parts -> part k owns stripes k and k+540
    part = 333
    gu8, gf = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part)
    o = oracle_scenes("redchair")
    refs = [o.render(w, h, spp, tile=(0, (part + j * parts) * rows, w, rows), flags=ol.PRODUCT_FLAGS_SMALL_TRI, nthreads=8) for j in range(2)]
    ref = dict(f32=np.concatenate([r["f32"].reshape(-1, 4) for r in refs]), u8=np.concatenate([r["u8"].reshape(-1, 4) for r in refs]))
    check_image(gu8, gf, ref)


def test_config5_two_million_primitives_4k_256spp_stripe_matches_oracle():
    """BASELINE config 5 (1 M spheres + 1 M triangles, 3840x2160 at 256 spp): one row of the full-size frame -- pixels, and
    the ray / node / primitive counters with `==`."""
    stl = m.syntheticScene(1_000_000, 1_000_000, seed=1234)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    w, h, spp, rows = 3840, 2160, 256, 1
    parts, part = h, 1201
    gu8, gf = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part, counters=True)
    st = raw.stats()
    o = ol.OracleScene(ol.ArrayScene(stl), bounds_mode=0)
    ref = o.render(w, h, spp, tile=(0, part, w, rows), flags=ol.PRODUCT_FLAGS_TRI, nthreads=8)
    check_image(gu8, gf, ref)
    for k in ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack"):
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    # the same row walked over the exact records (qnodes = 0): identical bytes, its own counters
    for opts, flags in ((dict(qnodes=0), ol.product_flags(True, qnodes=0)),):
        with options(raw, **opts):
            b8, bf = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part, counters=True)
            sb = raw.stats()
        assert np.array_equal(gu8, b8) and np.array_equal(gf.view(np.uint32), bf.view(np.uint32))
        refb = o.render(w, h, spp, tile=(0, part, w, rows), flags=flags, nthreads=8)
        for k in COUNTER_KEYS:
            assert sb[k] == refb["stats"][k], (opts, k, sb[k], refb["stats"][k])
    raw.close()
    o.close()


def test_config5_ordered_everywhere_gives_the_same_bytes_on_this_scene():
    """Option traversal = 2 (near child first at every node, not only between sphere-only subtrees) is NOT exact in general:
    where a triangle is hit in the reference's 0.001 slack outside its box the reference's own result depends on its visiting
    order (redchair.txt: 0.1 % of the pixels change).  On BASELINE config 5's scene (random, unconnected triangles) it is:
    three rows of the 3840x2160 x 256 spp frame give identical bytes, float image included, with 57 % fewer node visits --
    and its counters equal the oracle's mirror (ORC_FLAG_ORDERED_ALL)."""
    stl = m.syntheticScene(1_000_000, 1_000_000, seed=1234)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    w, h, spp, rows = 3840, 2160, 256, 1
    parts, part = h // 3, 401                      # part k owns rows k, k + 720, k + 1440
    raw.set_option("traversal", 0)
    a8, af = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part, counters=True)
    sa = raw.stats()
    raw.set_option("traversal", 2)
    b8, bf = gpu_render(raw, w, h, spp, stripe_rows=rows, num_parts=parts, part=part, counters=True)
    sb = raw.stats()
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    assert sa["rays"] == sb["rays"] and sb["internal_visits"] < 0.5 * sa["internal_visits"]
    o = ol.OracleScene(ol.ArrayScene(stl), bounds_mode=0)
    ref = o.render(w, h, spp, tile=(0, part, w, rows), flags=ol.product_flags(True, traversal=2), nthreads=8)
    n = w * rows
    check_image(b8[:n], bf[:n], ref)
    rawc = m.initRawConfigFromStl(stl, 0)          # counters of the first row alone, against the oracle
    m.build_lbvh_karas(rawc)
    rawc.set_option("traversal", 2)
    c8, cf = gpu_render(rawc, w, h, spp, stripe_rows=rows, num_parts=h, part=part, counters=True)
    sc = rawc.stats()
    for k in COUNTER_KEYS:
        assert sc[k] == ref["stats"][k], (k, sc[k], ref["stats"][k])
    raw.close(); rawc.close(); o.close()


def test_stripe_partition_is_bit_identical_to_whole_frame(gpu_scenes):
    """Tile-split invariance: any partition gives the same bytes."""
    stl, raw = gpu_scenes("tenthousand")
    w, h, spp = 200, 121, 16
    whole_u8, whole_f = gpu_render(raw, w, h, spp)
    for parts, rows in ((2, 8), (3, 5), (8, 4)):
        frame = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        for part in range(parts):
            p = api.render_params(w, h, spp, rows, parts, part)
            n = api.num_pixels(p)
            buf = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
            m.render(buf, w, h, spp, raw, params=p)
            m.scatter_part(p, buf, frame)
        torch.cuda.synchronize()
        assert np.array_equal(frame.cpu().numpy().reshape(-1, 4), whole_u8), (parts, rows)


@pytest.mark.parametrize("ns,nt", [(30000, 30000), (300000, 200000)])
def test_synthetic_scene_build_and_render_match_oracle(ns, nt):
    """BASELINE config 5's generator at reduced size: multi-block radix sort, duplicate Morton codes, mixed primitives."""
    stl = m.syntheticScene(ns, nt, seed=1234)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    o = ol.OracleScene(ol.ArrayScene(stl), bounds_mode=0)
    nodes, codes, refs, bounds = raw.tree()
    assert np.array_equal(codes, o.codes())
    orefs = o.refs()
    assert np.array_equal(refs["type"], orefs["type"]) and np.array_equal(refs["id"], orefs["id"])
    on = o.nodes()
    for f in ("left", "right"):
        assert np.array_equal(nodes[f], on[f]), f
    for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"):
        assert np.array_equal(nodes[f].view(np.uint32), on[f].view(np.uint32)), f
    w, h, spp = 96, 54, 4
    gu8, gf = gpu_render(raw, w, h, spp, counters=True)
    st = raw.stats()
    ref = o.render(w, h, spp, flags=ol.product_flags(True, nprims=ns + nt), nthreads=8)
    check_image(gu8, gf, ref)
    for k in ("rays", "internal_visits", "sphere_tests", "tri_tests", "max_stack"):
        assert st[k] == ref["stats"][k], k
    raw.close()
    o.close()


@pytest.mark.parametrize("ns,nt", [(1024, 1025)])
def test_synthetic_scene_tree_matches_oracle_at_the_tile_edge(ns, nt):
    """The tree alone, no render: 2049 primitives are one full sort / scan tile (2048 items) and a second workgroup with one item."""
    stl = m.syntheticScene(ns, nt, seed=1234)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    o = ol.OracleScene(ol.ArrayScene(stl), bounds_mode=0)
    nodes, codes, refs, bounds = raw.tree()
    assert len(codes) == ns + nt and np.array_equal(codes, o.codes())
    orefs = o.refs()
    assert np.array_equal(refs["type"], orefs["type"]) and np.array_equal(refs["id"], orefs["id"])
    on = o.nodes()
    for f in ("left", "right"):
        assert np.array_equal(nodes[f], on[f]), f
    for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"):
        assert np.array_equal(nodes[f].view(np.uint32), on[f].view(np.uint32)), f
    raw.close()
    o.close()


@pytest.mark.parametrize("name,w,h,spp", [("tenthousand", 96, 54, 16), ("redchair", 64, 36, 32), ("spiral", 96, 54, 1), ("tri", 256, 256, 0)])
def test_wavefront_path_matches_oracle(name, w, h, spp, gpu_scenes, oracle_scenes):
    """The trace/shade kernel pair (option "wavefront") must give the same pixels and the same counters."""
    stl, raw = gpu_scenes(name)
    with options(raw, wavefront=1, wf_pool=4096):      # small pool: many rounds, slots refilled many times
        gu8, gf = gpu_render(raw, w, h, spp, counters=True)
        st = raw.stats()
    ref = oracle_scenes(name).render(w, h, spp, flags=ol.product_flags(stl.num_triangles > 0, wavefront=True), nthreads=8)
    check_image(gu8, gf, ref)
    for k in ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack"):
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])


def test_both_paths_give_identical_bytes(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    a8, af = gpu_render(raw, 200, 120, 16)
    with options(raw, wavefront=1):
        b8, bf = gpu_render(raw, 200, 120, 16)
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))


@pytest.mark.parametrize("name,w,h,spp", [("tenthousand", 96, 54, 16), ("spiral", 96, 54, 4), ("redchair", 64, 36, 32), ("tri", 128, 128, 0)])
@pytest.mark.parametrize("traversal,qnodes", [(0, 1), (1, 1), (2, 1), (1, 2), (1, 0)])
def test_every_traversal_mode_matches_its_oracle_mirror(name, w, h, spp, traversal, qnodes, gpu_scenes, oracle_scenes):
    """traversal 0 = node for node the reference's left-first walk, 1 = near child first where both subtrees hold spheres
    only (default), 2 = near child first everywhere; qnodes 2 = quantised records on every scene (the wide walk on redchair.txt and
    tri.txt, which run on the exact records by default), 0 = never.  The oracle mirrors each: pixels within tolerance, visit
    counters equal."""
    stl, raw = gpu_scenes(name)
    with options(raw, traversal=traversal, qnodes=qnodes):
        gu8, gf = gpu_render(raw, w, h, spp, counters=True)
        st = raw.stats()
    flags = ol.product_flags(stl.num_triangles > 0, traversal=traversal, qnodes=qnodes)
    ref = oracle_scenes(name).render(w, h, spp, flags=flags, nthreads=8)
    check_image(gu8, gf, ref)
    for k in COUNTER_KEYS:
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    assert st["rays_traversed"] == ref["stats"]["traversals"] <= st["rays"]


REFERENCE_WALK = dict(traversal=0, shadow_anyhit=0, skip_unlit=0, qnodes=0)


@pytest.mark.parametrize("name,w,h,spp,rays_per_sample,iters,leaf", [
    ("tenthousand", 240, 135, 1, 5.49, 27.5, 1.86), ("spiral", 240, 135, 1, 9.43, 57.6, 14.36), ("redchair", 240, 135, 1, 6.18, 18.0, 2.55),
    ("tri", 256, 256, 0, 1.31, 4.0, 1.03)])
def test_reference_walk_mode_is_the_plain_restatement_counter_for_counter(name, w, h, spp, rays_per_sample, iters, leaf, gpu_scenes, oracle_scenes):
    """One direct link from the HIP path to the reference's walk: with {traversal: 0, shadow_anyhit: 0, skip_unlit: 0,
    qnodes: 0} the kernel is draw.cu:292-377 + bvh_traversal.cu:92-183 as written -- left child first, every shadow ray traced
    to its nearest hit, every light's shadow ray traced, 64-byte exact boxes -- and is compared with the oracle's plain
    restatement (flags = 0): pixels within 1e-4, every ray / node / primitive counter with ==.  The same counters reproduce the
    statistics SURVEY.md Appendix G measured on the reference's own code (stub RNG there: 2 %; a node-loop iteration of
    bvh_traversal.cu:107 is an internal visit or a leaf test)."""
    stl, raw = gpu_scenes(name)
    with options(raw, **REFERENCE_WALK):
        gu8, gf = gpu_render(raw, w, h, spp, counters=True)
        st = raw.stats()
    ref = oracle_scenes(name).render(w, h, spp, flags=ol.REFERENCE_WALK, nthreads=8)
    check_image(gu8, gf, ref)
    for k in COUNTER_KEYS:
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    assert st["rays_traversed"] == ref["stats"]["traversals"] == st["rays"]      # this mode walks the BVH for every ray
    assert abs(st["rays"] / st["samples"] / rays_per_sample - 1) < 0.02
    assert abs((st["internal_visits"] + st["sphere_tests"] + st["tri_tests"]) / st["rays"] / iters - 1) < 0.02
    assert abs((st["sphere_tests"] + st["tri_tests"]) / st["rays"] / leaf - 1) < 0.02


@pytest.mark.parametrize("name", ["tenthousand", "redchair"])
def test_default_mode_gives_the_bytes_of_the_reference_walk_mode(name, gpu_scenes):
    """... and the default options (near child first, any-hit shadow rays, unlit lights skipped, quantised records) give the bytes
    of that mode, float image included, with a fraction of the node visits: 1920x1080 x 16 spp."""
    stl, raw = gpu_scenes(name)
    w, h, spp = 1920, 1080, 16
    a8, af = gpu_render(raw, w, h, spp, counters=True)
    sa = raw.stats()
    with options(raw, **REFERENCE_WALK):
        b8, bf = gpu_render(raw, w, h, spp, counters=True)
        sb = raw.stats()
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    assert sa["rays"] == sb["rays"] and sa["internal_visits"] < 0.9 * sb["internal_visits"]


@pytest.mark.parametrize("qnodes", [1, 0])
def test_a_hit_the_reference_never_tests_sends_the_ray_over_its_literal_walk(qnodes):
    """tests/golden/far_camera_tie.txt (three spheres of a fuzz scene, tools/fuzz_modes.py seed 47 scene 795; the camera 4 000
    units away): the primary ray of pixel (50, 97) touches two spheres within one ulp of t, and the nearer hit rounds to just
    below the entry distance of its own leaf box -- the reference, having met the other sphere first, never tests it; a walk
    over the larger quantised boxes does.  The shade phase vets the hit (hit_needs_literal_walk) and walks the ray again literally:
    every counter equals the oracle's mirror (one re-walk), and the frame -- bytes, float image, ray count -- is the
    reference-walk mode's.  Without the vetting the frame traces one ray more (the oracle restates that too)."""
    import cuda_ray_tracer_amd as m
    import pyscene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "far_camera_tie.txt")
    stl = m.parseInput(path)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    osc = ol.OracleScene(pyscene.parse_lines(open(path).read().split("\n")), bounds_mode=0)
    w, h, spp = 192, 108, 0
    try:
        with options(raw, qnodes=qnodes):
            a8, af = gpu_render(raw, w, h, spp, counters=True)
            sa = raw.stats()
        with options(raw, **REFERENCE_WALK):
            b8, bf = gpu_render(raw, w, h, spp, counters=True)
            sb = raw.stats()
        flags = ol.product_flags(False, qnodes=qnodes)
        ref = osc.render(w, h, spp, flags=flags, nthreads=8)
        plain = osc.render(w, h, spp, flags=0, nthreads=8)
        unvetted = osc.render(w, h, spp, flags=flags & ~ol.FLAG_REACH, nthreads=8)
    finally:
        raw.close()
    for k in COUNTER_KEYS:
        assert sa[k] == ref["stats"][k], (k, sa[k], ref["stats"][k])
        assert sb[k] == plain["stats"][k], (k, sb[k], plain["stats"][k])
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    assert sa["rays"] == sb["rays"] == plain["stats"]["rays"]
    if qnodes:
        assert ref["stats"]["qn_retraces"] == 1 and unvetted["stats"]["rays"] == plain["stats"]["rays"] + 1


def test_a_shadow_ray_to_a_point_light_whose_occluder_the_reference_never_tests():
    """tests/golden/far_plane_point_light.txt (tests/test_oracle_units.py has the story): shadow rays towards a point light are
    traced to their nearest hit and vetted when the walk is over the quantised records -- every counter equals the oracle's
    mirror (re-walks included), and the frame is the reference-walk mode's: bytes, float image, ray count."""
    import pyscene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "far_plane_point_light.txt")
    stl = m.parseInput(path)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    osc = ol.OracleScene(pyscene.parse_lines(open(path).read().split("\n")), bounds_mode=0)
    w, h, spp = 192, 108, 2
    try:
        a8, af = gpu_render(raw, w, h, spp, counters=True)
        sa = raw.stats()
        with options(raw, **REFERENCE_WALK):
            b8, bf = gpu_render(raw, w, h, spp, counters=True)
            sb = raw.stats()
        ref = osc.render(w, h, spp, flags=ol.product_flags(False, grid_ok=osc.grid_ok()), nthreads=8)
        plain = osc.render(w, h, spp, flags=0, nthreads=8)
    finally:
        raw.close()
    assert ref["stats"]["qn_retraces"] > 0
    for k in COUNTER_KEYS:
        assert sa[k] == ref["stats"][k], (k, sa[k], ref["stats"][k])
        assert sb[k] == plain["stats"][k], (k, sb[k], plain["stats"][k])
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32)) and sa["rays"] == sb["rays"]


@pytest.mark.parametrize("name", ["tenthousand", "spiral", "redchair", "tri"])
def test_default_traversal_gives_the_bytes_of_the_reference_order(name, gpu_scenes):
    """The ordered traversal changes which nodes are visited, never the closest hit: the whole 1920x1080 x 16 spp frame
    (BASELINE configs 2 and 3) is byte-identical, float image included, to the frame rendered in the reference's left-first
    order -- and it takes fewer node visits."""
    stl, raw = gpu_scenes(name)
    w, h, spp = 1920, 1080, 16
    a8, af = gpu_render(raw, w, h, spp, counters=True)
    sa = raw.stats()
    with options(raw, traversal=0):
        b8, bf = gpu_render(raw, w, h, spp, counters=True)
        sb = raw.stats()
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    # (a handful of rays per frame are walked twice: hit_needs_literal_walk)
    assert sa["rays"] == sb["rays"] and sa["internal_visits"] <= sb["internal_visits"] * 1.00001
    if name in ("tenthousand", "spiral"):
        assert sa["internal_visits"] < 0.85 * sb["internal_visits"]


@pytest.mark.parametrize("name", ["tenthousand", "spiral", "redchair"])
def test_specialised_kernels_give_the_bytes_and_counters_of_the_general_ones(name, gpu_scenes):
    """render.hip compiles the trace kernel without what a scene does not have (triangles, point lights, the pending list of
    refraction / gi; option `specialise`).  Whole 1920x1080 x 16 spp frames: the general kernel (specialise = 0) gives the same
    bytes, float image included, and the same value of every counter."""
    stl, raw = gpu_scenes(name)
    w, h, spp = 1920, 1080, 16
    a8, af = gpu_render(raw, w, h, spp, counters=True)
    sa = raw.stats()
    with options(raw, specialise=0):
        b8, bf = gpu_render(raw, w, h, spp, counters=True)
        sb = raw.stats()
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    for k in COUNTER_KEYS:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def test_random_sphere_scenes_default_mode_equals_reference_order(tmp_path):
    """tools/fuzz_modes.py, 60 scenes of a fixed seed: random sphere clouds at scales 1e-3 .. 1e6, cameras inside / outside / far
    away, pinhole / fisheye / panorama, some with point lights, glass and gi.  The default mode (near child first, quantised
    records with the permute box test, specialised kernels) must give the frame of traversal = 0 (left-first walk over the float
    records) byte for byte, float image included.  (2300 scenes of five other seeds were run once by hand: no mismatch.)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_modes
    assert fuzz_modes.main(["--scenes", "60", "--seed", "11", "--out", str(tmp_path)]) == 0


@pytest.mark.parametrize("extra", [["--far"], ["--far", "--triangles", "1.0", "--qnodes", "2"], ["--offset"], ["--offset", "--far", "--triangles", "0.3", "--qnodes", "2"]],
                         ids=["far-spheres", "far-mixed-wide", "offset-spheres", "offset-far-mixed-wide"])
def test_far_camera_scenes_default_mode_equals_the_reference_walk_mode(extra, tmp_path):
    """The regimes of tests/golden/far_camera_tie.txt and far_plane_point_light.txt at random (fuzz_modes.py --far: cameras
    10^3 .. 10^5 scene sizes away, many large overlapping spheres -- the oracle counts five literal re-walks per scene there on
    average; --offset: the whole scene 3 .. 3000 of its sizes away from the world origin): 100 scenes per kind, the
    default mode -- rendered twice, the second time in the measured hand-out order -- against the reference-walk mode
    (traversal 0, shadow_anyhit 0, skip_unlit 0, qnodes 0): bytes, float image and ray count."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_modes
    assert fuzz_modes.main(["--scenes", "100", "--seed", "71", "--reference-walk", "--out", str(tmp_path)] + extra) == 0


def test_shipped_tree_mode_reproduces_the_survey_golden_image(gpu_scenes, oracle_scenes):
    """Build option bounds_as_shipped: the reference as shipped never stores its scene bounds (parse.cpp:28), so every
    Morton code is 0.  With it, and the reference's traversal order, the HIP path itself reproduces the RNG-free known
    answer SURVEY.md 8c recorded from the reference's own code: tri.txt 256x256 aa 0, SHA-256 of the RGBA bytes."""
    import hashlib
    stl, raw = gpu_scenes("tri")
    with options(raw, rebuild=True, bounds_as_shipped=1, traversal=0):
        nodes, codes, refs, bounds = raw.tree()
        gu8, gf = gpu_render(raw, 256, 256, 0)
    o = oracle_scenes("tri", 1)
    assert np.all(codes == 0) and np.array_equal(nodes["left"], o.nodes()["left"]) and np.array_equal(nodes["right"], o.nodes()["right"])
    assert np.isposinf(bounds[:3]).all() and np.isneginf(bounds[3:]).all()
    assert hashlib.sha256(gu8.tobytes()).hexdigest() == "ddfa3b865899303f54ad788218e8908fe5553b9ed4b085f9401dcabd19db64c9"
    assert gu8.reshape(256, 256, 4)[164, 100].tolist() == [238, 238, 238, 255]      # the order-dependent pixel, as shipped


def test_two_million_primitive_build_matches_oracle():
    """BASELINE config 5's scene at full size (1 M spheres + 1 M triangles): the whole tree, bit for bit.  Also the
    regression test of the refit's fence-free hand-off (write-through stores + drained counter add)."""
    stl = m.syntheticScene(1_000_000, 1_000_000, seed=1234)
    raw = m.initRawConfigFromStl(stl, 0)
    for _ in range(3):                       # rebuild a few times: the hand-off must hold under different timings
        m.build_lbvh_karas(raw)
    o = ol.OracleScene(ol.ArrayScene(stl), bounds_mode=0)
    nodes, codes, refs, bounds = raw.tree()
    assert np.array_equal(codes, o.codes())
    on = o.nodes()
    for f in ("left", "right"):
        assert np.array_equal(nodes[f], on[f]), f
    for f in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax"):
        assert np.array_equal(nodes[f].view(np.uint32), on[f].view(np.uint32)), f
    gu8, gf = gpu_render(raw, 64, 36, 1, counters=True)
    ref = o.render(64, 36, 1, flags=ol.PRODUCT_FLAGS, nthreads=8)
    check_image(gu8, gf, ref)
    raw.close()
    o.close()


def test_full_size_frame_equals_its_eight_stripe_sets(gpu_scenes):
    """BASELINE config 3 at full size, through a size-independent property: the whole 1920x1080 frame at 16 spp (256-sample
    chunks, longest-first order from the first render applied in the second) against the same frame rendered as the
    eight interleaved stripe sets an 8-GPU job uses (64-sample chunks) and re-interleaved -- byte for byte."""
    stl, raw = gpu_scenes("tenthousand")
    w, h, spp = 1920, 1080, 16
    whole = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    for _ in range(2):                      # second pass: the chunk order measured by the first is in use
        m.render(whole, w, h, spp, raw)
    frame = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    for part in range(8):
        p = api.render_params(w, h, spp, 4, 8, part)
        buf = torch.zeros(api.num_pixels(p) * 4, dtype=torch.uint8, device="cuda")
        m.render(buf, w, h, spp, raw, params=p)
        api.scatter_part(p, buf, frame)
    torch.cuda.synchronize()
    assert torch.equal(whole, frame)
    img = whole.cpu().numpy().reshape(h, w, 4)
    assert img[..., 3].max() == 255 and 0 < int((img[..., 3] == 0).sum()) < w * h      # sky and geometry both present


def test_frames_in_flight_and_chunk_order_do_not_change_pixels(gpu_scenes):
    """Four frames overlapped on four streams (each uses its own workspace set), rendered repeatedly so that later frames
    run with a longest-first chunk order measured on earlier ones: every frame must be byte-identical."""
    stl, raw = gpu_scenes("tenthousand")
    w, h, spp = 320, 180, 16
    ref8, reff = gpu_render(raw, w, h, spp)
    streams = [torch.cuda.Stream() for _ in range(4)]
    p = api.render_params(w, h, spp)
    bufs = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(12)]
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        with torch.cuda.stream(streams[i % 4]):
            m.render(b, w, h, spp, raw, params=p)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy().reshape(-1, 4), ref8), i
    st = raw.stats()
    assert st["frames_timed"] >= 1 and st["trace_kernel_ms_mean"] > 0


def test_slabs_do_not_change_pixels_or_counters(gpu_scenes):
    """A call is rendered in slabs of at most 2^slab_log2 samples (bounded per-sample workspace: BASELINE config 5 would
    otherwise need 34 GB).  Forced here on a small frame (2^10 samples per slab -> 169 slabs, ragged last one)."""
    stl, raw = gpu_scenes("redchair")
    w, h, spp = 120, 90, 16
    a8, af = gpu_render(raw, w, h, spp, counters=True)
    sa = raw.stats()
    with options(raw, slab_log2=10):
        b8, bf = gpu_render(raw, w, h, spp, counters=True)
        sb = raw.stats()
        c8, cf = gpu_render(raw, w, h, spp, stripe_rows=4, num_parts=3, part=1)
    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32))
    for k in COUNTER_KEYS:
        assert sa[k] == sb[k], k
    d8, df = gpu_render(raw, w, h, spp, stripe_rows=4, num_parts=3, part=1)
    assert np.array_equal(c8, d8) and np.array_equal(cf.view(np.uint32), df.view(np.uint32))


@pytest.mark.parametrize("name,w,h,spp", [("tenthousand", 200, 120, 16), ("redchair", 160, 90, 32)])
def test_the_hand_out_order_never_changes_a_byte(name, w, h, spp, gpu_scenes):
    """sched = 2 (default): the first frame of a shape measures every sample's cost class (counting kernels + a stable one-byte
    radix sort per launch) and later frames hand the samples out most expensive class first; sched = 1 does the same by chunk,
    0 takes them in frame order.  Scheduling only: every frame of every mode -- the measuring one, the ordered ones, one-slab
    and multi-slab calls, a stripe part, counters on or off -- gives the same bytes and the same counters."""
    stl, raw = gpu_scenes(name)
    with options(raw, sched=0):
        a8, af = gpu_render(raw, w, h, spp, counters=True)
        sa = raw.stats()
    for sched in (2, 1):
        for slab_log2 in (28, 12):
            with options(raw, sched=sched, slab_log2=slab_log2):
                for frame in range(3):                  # measure, (maybe unordered while the sort lands), ordered
                    b8, bf = gpu_render(raw, w, h, spp, counters=(frame == 2))
                    assert np.array_equal(a8, b8) and np.array_equal(af.view(np.uint32), bf.view(np.uint32)), (sched, slab_log2, frame)
                sb = raw.stats()
                for k in COUNTER_KEYS:
                    assert sa[k] == sb[k], (sched, slab_log2, k)
                p8, pf = gpu_render(raw, w, h, spp, stripe_rows=4, num_parts=3, part=1)      # another shape: measured afresh
                q8, qf = gpu_render(raw, w, h, spp, stripe_rows=4, num_parts=3, part=1)
                assert np.array_equal(p8, q8) and np.array_equal(pf.view(np.uint32), qf.view(np.uint32))


def gpu_accumulate(raw, w, h, passes, total):
    acc = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    for first, count in passes:
        m.render_accumulate(acc, w, h, first, count, raw)
    img = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
    m.finalize(img, acc, w, h, total)
    torch.cuda.synchronize()
    return img.cpu().numpy().reshape(h, w, 4), acc.cpu().numpy().reshape(h, w, 4)


@pytest.mark.parametrize("name,w,h,spp", [("tenthousand", 96, 54, 16), ("redchair", 64, 36, 32), ("spiral", 48, 27, 20),
                                              ("spiral", 48, 27, 100)])
def test_accumulate_then_finalize_gives_the_bytes_of_render(name, w, h, spp, gpu_scenes):
    """render_kernel_atomic_aa + finalize_kernel (draw.cu:13-92) as mirt_render_accumulate + mirt_finalize: all samples in one
    call is the same sum tree as mirt_render -> identical bytes.  (100 samples: P = 128, the one-thread-per-pixel sum in both.)"""
    stl, raw = gpu_scenes(name)
    r8, rf = gpu_render(raw, w, h, spp)
    a8, acc = gpu_accumulate(raw, w, h, [(0, spp)], spp)
    assert np.array_equal(a8.reshape(-1, 4), r8)


@pytest.mark.parametrize("name,w,h,passes", [("tenthousand", 64, 36, [(0, 8), (8, 8), (16, 5)]), ("redchair", 48, 27, [(0, 1), (1, 1), (2, 30)]),
                                             ("tri", 40, 40, [(0, 100), (100, 100)])])
def test_progressive_accumulation_matches_the_oracle(name, w, h, passes, gpu_scenes, oracle_scenes):
    """Several calls (progressive rendering; more than 64 samples per pixel): every call adds its own butterfly-ordered sum.
    The oracle does the same arithmetic: accumulation buffer within the float tolerance, 8-bit image within 1 LSB."""
    stl, raw = gpu_scenes(name)
    total = sum(c for _, c in passes)
    g8, gacc = gpu_accumulate(raw, w, h, passes, total)
    o = oracle_scenes(name)
    oacc = np.zeros((h, w, 4), np.float32)
    for first, count in passes:
        o.render_accumulate(oacc, w, h, first, count, flags=ol.PRODUCT_FLAGS, nthreads=8)
    assert np.nanmax(np.abs(gacc.astype(np.float64) - oacc.astype(np.float64))) <= TOL * total
    assert np.abs(g8.astype(np.int32) - ol.OracleScene.finalize(oacc, total).astype(np.int32)).max() <= 1

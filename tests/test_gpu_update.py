"""GPU: updates of a built scene in place (mirt_scene_set_camera, mirt_scene_update_spheres / update_triangles, mirt_multi_set_camera).
The yardstick throughout is a FRESH scene: a new RawConfig made from a descriptor that holds the new values, then built -- tree,
frame bytes, float frame, counters and primary-hit records must be equal (==).  Where stated the CPU oracle is a second
yardstick, with the tolerance and the counter equality of gpu_case.check_against_oracle.  Every call is made once."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import edge_scenes
import gpu_case
import oracle_lib as ol
import pyscene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
f32 = np.float32
KEYS = gpu_case.COUNTER_KEYS + ("rays_traversed", "overflow_events")
MODES = {"reference_walk": gpu_case.REFERENCE_WALK, "default": {}}


def _file(name):
    return open(os.path.join(ROOT, "scenes", name + ".txt")).read()


class _Held:
    """What RawConfig takes: a descriptor, and whatever owns the memory its pointers name."""

    def __init__(self, desc, *keep):
        self.desc, self.keep = desc, keep


def _built(source, **options):
    raw = m.RawConfig(source, 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return raw


def _camera_of(desc):
    c = api.Camera()
    c.eye, c.forward, c.right, c.up = desc.eye, desc.forward, desc.right, desc.up
    c.dof_focus, c.dof_lens, c.fisheye, c.panorama = desc.dof_focus, desc.dof_lens, desc.fisheye, desc.panorama
    return c


def _camera_words(c):
    return np.frombuffer(bytes(c), np.uint32)


def _fresh_source(stl, spheres=None, triangles=None, cam=None):
    """A descriptor like stl's with the sphere / triangle arrays (numpy, layouts.SPHERE / TRIANGLE) and the camera replaced."""
    d = api.SceneDesc.from_buffer_copy(bytes(stl.desc))
    if spheres is not None:
        assert len(spheres) == d.num_spheres
        d.spheres = spheres.ctypes.data if len(spheres) else None
    if triangles is not None:
        assert len(triangles) == d.num_triangles
        d.triangles = triangles.ctypes.data if len(triangles) else None
    if cam is not None:
        d.eye, d.forward, d.right, d.up = cam.eye, cam.forward, cam.right, cam.up
        d.dof_focus, d.dof_lens, d.fisheye, d.panorama = cam.dof_focus, cam.dof_lens, cam.fisheye, cam.panorama
    return _Held(d, stl, spheres, triangles)


def _oracle_of(stl, spheres=None, triangles=None):
    """The oracle over the same arrays (built)."""
    a = ol.ArrayScene(stl)
    if spheres is not None:
        a._arrays["spheres"] = spheres
    if triangles is not None:
        a._arrays["triangles"] = triangles
    return ol.OracleScene(a, bounds_mode=0)


def _primary_hits(raw, w, h, spp):
    n = api.num_pixels(api.render_params(w, h, spp))
    rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.full((n, 6), -7, dtype=torch.int32, device=DEV)
    m.camera_rays(raw, rays, w, h, spp)
    m.trace_rays(raw, rays, hits)
    torch.cuda.synchronize()
    return rays.cpu().numpy().view(np.uint32), hits.cpu().numpy().view(np.uint32)


def _words_equal(a, b):
    """Equal bits, except that a NaN may stand against a NaN of another payload (the positions of the NaNs must agree)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    na = np.isnan(a.view(f32)) if a.dtype != np.uint8 else np.zeros(a.shape, bool)
    nb = np.isnan(b.view(f32)) if b.dtype != np.uint8 else np.zeros(b.shape, bool)
    wa = a if a.dtype == np.uint8 else a.view(np.uint32)
    wb = b if b.dtype == np.uint8 else b.view(np.uint32)
    return bool(np.array_equal(na, nb) and np.array_equal(wa[~na], wb[~nb]))


def _observe(raw, w, h, spp):
    gu, gf, st = gpu_case.gpu_render(raw, w, h, spp)
    rays, hits = _primary_hits(raw, w, h, spp)
    return dict(u8=gu, f32=gf, stats={k: st[k] for k in KEYS}, st=st, rays=rays, hits=hits)


def _assert_same(got, want, what=""):
    assert np.array_equal(got["u8"], want["u8"]), what + ": 8-bit frame"
    assert _words_equal(got["f32"], want["f32"]), what + ": float frame"
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["stats"]["overflow_events"] == 0
    assert _words_equal(got["rays"], want["rays"]), what + ": camera rays"
    assert _words_equal(got["hits"], want["hits"]), what + ": closest-hit records"


def _assert_same_tree(raw, other):
    a, b = raw.tree(), other.tree()
    for x, y, name in zip(a, b, ("nodes", "codes", "refs", "bounds")):
        assert x.tobytes() == y.tobytes(), name


def _assert_oracle_tree(raw, o):
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


def _xyzr(sph):
    return np.ascontiguousarray(np.concatenate([sph["c"], sph["r"][:, None]], axis=1), dtype=f32)


def _with_xyzr(sph, xyzr, first=0):
    out = sph.copy()
    out["c"][first:first + len(xyzr)] = xyzr[:, :3]
    out["r"][first:first + len(xyzr)] = xyzr[:, 3]
    return out


def _moved(sph, seed, scale=0.05):
    """Every sphere displaced (and resized a little) by a seeded offset."""
    rng = np.random.default_rng(seed)
    x = _xyzr(sph)
    x[:, :3] += rng.uniform(-scale, scale, (len(x), 3)).astype(f32)
    x[:, 3] *= rng.uniform(0.9, 1.1, len(x)).astype(f32)
    return x


def _sphere_cluster(n=300, seed=21):
    rng = np.random.default_rng(seed)
    out = ["png 64 48 cluster.png\n", "bounces 3\n", "eye 0 0.3 4\n", "color 1 1 1\n", "sun 1 1 1\n", "sun -1 2 0.5\n", "shininess 0.4\n"]
    for _ in range(n):
        c = rng.uniform(-1, 1, 3)
        out.append("color %.3f %.3f %.3f\n" % tuple(rng.uniform(0.2, 1, 3)))
        out.append("sphere %.4f %.4f %.4f %.4f\n" % (c[0], c[1], c[2], rng.uniform(0.03, 0.12)))
    return "".join(out)


def _mixed_scene(seed=9, ns=150, nt=150):
    """Spheres and triangles over a plane, file order interleaved (the _random_scene_text style of test_gpu_queries.py)."""
    rng = np.random.default_rng(seed)
    out = ["png 8 8 q.png\n", "eye 0 0 6\n", "bounces 3\n", "color 1 1 1\n", "sun 1 1 1\n", "color 0.8 0.7 0.6\n", "shininess 0.3\n", "plane 0 1 0 3.5\n"]
    nv = 0
    for k in range(max(ns, nt)):
        if k < ns:
            c = rng.uniform(-3, 3, 3)
            out.append("sphere %.5f %.5f %.5f %.5f\n" % (c[0], c[1], c[2], rng.uniform(0.1, 0.5)))
        if k < nt:
            c = rng.uniform(-3, 3, 3)
            for _ in range(3):
                out.append("xyz %.5f %.5f %.5f\n" % tuple(c + rng.uniform(-0.7, 0.7, 3)))
            out.append("tri %d %d %d\n" % (nv + 1, nv + 2, nv + 3))
            nv += 3
    return "".join(out)


def _tri_verts(tri):
    return np.ascontiguousarray(np.concatenate([tri["p0"], tri["p1"], tri["p2"]], axis=1), dtype=f32)


def _with_verts(tri, verts, first=0):
    """The triangle records the parser would make of these vertices: pyscene's float32 restatement of object.cuh:177-191."""
    out = tri.copy()
    with np.errstate(all="ignore"):
        for i, v in enumerate(verts):
            p0, p1, p2 = v[0:3].astype(f32), v[3:6].astype(f32), v[6:9].astype(f32)
            nor = pyscene._normalize(pyscene._cross(p1 - p0, p2 - p0))
            a1 = pyscene._cross(p2 - p0, nor)
            a2 = pyscene._cross(p1 - p0, nor)
            k1 = f32(f32(1) / pyscene._dot(a1, p1 - p0))
            k2 = f32(f32(1) / pyscene._dot(a2, p2 - p0))
            t = out[first + i]
            t["p0"], t["p1"], t["p2"], t["nor"] = p0, p1, p2, nor
            t["e1"] = pyscene._v(a1[0] * k1, a1[1] * k1, a1[2] * k1)
            t["e2"] = pyscene._v(a2[0] * k2, a2[1] * k2, a2[2] * k2)
    return out


# ---- 1. camera ---------------------------------------------------------------------------------------------------------------
CAMERA_B = "eye 0.3 0.2 0.5\nforward -0.1 -0.05 -1\nup 0.1 1 0\n"
CAMERA_VARIANTS = {"plain": "dof 0 0\n", "dof": "dof 3 0.05\n", "fisheye": "dof 0 0\nfisheye\n", "panorama": "panorama\n"}


@pytest.fixture(scope="module")
def scene_a():
    stl = m.parseText(_file("tenthousand"))
    raw = _built(stl)
    yield stl, raw
    raw.close()


@pytest.mark.parametrize("variant", sorted(CAMERA_VARIANTS))
@pytest.mark.parametrize("spp", [0, 1, 16])
def test_set_camera_gives_the_fresh_scene_of_the_new_camera(variant, spp, scene_a):
    stl_a, raw = scene_a
    w, h = 96, 54
    cam_a = _camera_of(stl_a.desc)
    assert np.array_equal(_camera_words(raw.camera()), _camera_words(cam_a))
    first_a = _observe(raw, w, h, spp)

    text_b = _file("tenthousand") + "\n" + CAMERA_B + CAMERA_VARIANTS[variant]
    stl_b = m.parseText(text_b)
    cam_b = _camera_of(stl_b.desc)
    assert not np.array_equal(_camera_words(cam_a), _camera_words(cam_b))
    raw.set_camera(cam_b)
    assert np.array_equal(_camera_words(raw.camera()), _camera_words(cam_b))       # get_camera returns what was set
    got = _observe(raw, w, h, spp)

    fresh = _built(stl_b)
    want = _observe(fresh, w, h, spp)
    fresh.close()
    _assert_same(got, want, "camera B in place vs fresh")
    assert not np.array_equal(got["u8"], first_a["u8"])

    o = ol.OracleScene(pyscene.parse_lines(text_b.split("\n")), bounds_mode=0)
    ref = o.render(w, h, spp, flags=gpu_case.mirror_flags(stl_b, o), nthreads=8)
    o.close()
    gpu_case.check_against_oracle(got["f32"], got["u8"], got["st"], ref)

    raw.set_camera(cam_a)                                                           # setting A back gives A's first frame again
    _assert_same(_observe(raw, w, h, spp), first_a, "camera A again")


def test_set_camera_keyword_fields(scene_a):
    stl_a, raw = scene_a
    cam_a = raw.camera()
    new = raw.set_camera(eye=(0.5, 0.25, 1.0), fisheye=1)
    got = raw.camera()
    assert np.array_equal(_camera_words(got), _camera_words(new))
    assert got.eye.tolist() == [0.5, 0.25, 1.0] and got.fisheye == 1 and got.forward.tolist() == cam_a.forward.tolist()
    raw.set_camera(cam_a)
    assert np.array_equal(_camera_words(raw.camera()), _camera_words(cam_a))
    L = m.lib()
    assert L.mirt_scene_set_camera(raw._h, None) == 3 and L.mirt_scene_get_camera(raw._h, None) == 3


# ---- 2. spheres --------------------------------------------------------------------------------------------------------------
SPHERE_SCENES = {"tenthousand": lambda: _file("tenthousand"), "glass_spheres_bulb": edge_scenes.glass_spheres_bulb,
                 "single_sphere": edge_scenes.single_sphere}


@pytest.mark.parametrize("name", sorted(SPHERE_SCENES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_update_spheres_and_rebuild_give_the_fresh_scene(name, mode):
    w, h, spp = 96, 54, 4
    opts = MODES[mode]
    stl = m.parseText(SPHERE_SCENES[name]())
    sph0 = stl.array("spheres")
    raw = _built(stl, **opts)
    before = _observe(raw, w, h, spp)

    # every sphere, through a device tensor
    x1 = _moved(sph0, seed=101)
    m.update_spheres(raw, torch.from_numpy(x1).to(DEV))
    m.build_lbvh_karas(raw)
    sph1 = _with_xyzr(sph0, x1)
    fresh = _built(_fresh_source(stl, spheres=sph1), **opts)
    _assert_same_tree(raw, fresh)
    o = _oracle_of(stl, spheres=sph1)
    _assert_oracle_tree(raw, o)
    o.close()
    got = _observe(raw, w, h, spp)
    _assert_same(got, _observe(fresh, w, h, spp), "all spheres moved")
    fresh.close()
    assert not np.array_equal(got["u8"], before["u8"])

    # a sub-range: first > 0 and a count that is not a multiple of 64 (the one-sphere scene: its only sphere, again)
    n = len(sph0)
    first, count = (37, min(n - 37, 1000 + 27)) if n > 64 else (n - 1, 1)
    x2 = _moved(sph1[first:first + count], seed=202, scale=0.1)
    m.update_spheres(raw, torch.from_numpy(x2).to(DEV), first=first)
    m.build_lbvh_karas(raw)
    sph2 = _with_xyzr(sph1, x2, first)
    outside = np.ones(n, bool)
    outside[first:first + count] = False
    assert sph2[outside].tobytes() == sph1[outside].tobytes()
    fresh = _built(_fresh_source(stl, spheres=sph2), **opts)
    _assert_same_tree(raw, fresh)                      # (the spheres outside the range are untouched: the fresh scene holds sph1's)
    o = _oracle_of(stl, spheres=sph2)
    _assert_oracle_tree(raw, o)
    o.close()
    _assert_same(_observe(raw, w, h, spp), _observe(fresh, w, h, spp), "sub-range moved")
    fresh.close()
    raw.close()


# ---- 3. triangles ------------------------------------------------------------------------------------------------------------
TRIANGLE_SCENES = {"redchair": lambda: _file("redchair"), "mixed": _mixed_scene}


@pytest.mark.parametrize("name", sorted(TRIANGLE_SCENES))
@pytest.mark.parametrize("qnodes", [0, 2])
def test_update_triangles_and_rebuild_give_the_fresh_scene(name, qnodes):
    w, h, spp = 96, 54, 4
    stl = m.parseText(TRIANGLE_SCENES[name]())
    tri0 = stl.array("triangles")
    n = len(tri0)
    raw = _built(stl, qnodes=qnodes)
    before = _observe(raw, w, h, spp)
    assert before["st"]["node_record_bytes"] == 64

    rng = np.random.default_rng(303)
    v1 = _tri_verts(tri0)
    v1 += np.tile(rng.uniform(-0.2, 0.2, (n, 3)), (1, 3)).astype(f32)           # each triangle translated ...
    v1 += rng.uniform(-0.02, 0.02, (n, 9)).astype(f32)                           # ... and bent a little
    zero_area = n // 3
    v1[zero_area, 6:9] = v1[zero_area, 3:6]                                       # p2 = p1: cross = 0, nor = 0, e1 = e2 = NaN
    m.update_triangles(raw, torch.from_numpy(v1).to(DEV))
    m.build_lbvh_karas(raw)
    tri1 = _with_verts(tri0, v1)
    assert np.all(np.isnan(tri1["e1"][zero_area])) and np.all(tri1["nor"][zero_area] == 0)
    assert np.count_nonzero(np.isnan(tri1["e1"]).any(axis=1)) == 1
    fresh = _built(_fresh_source(stl, triangles=tri1), qnodes=qnodes)
    _assert_same_tree(raw, fresh)
    o = _oracle_of(stl, triangles=tri1)
    _assert_oracle_tree(raw, o)
    o.close()
    got = _observe(raw, w, h, spp)
    want = _observe(fresh, w, h, spp)
    _assert_same(got, want, "all triangles moved")
    fresh.close()
    assert not np.array_equal(got["u8"], before["u8"])
    assert np.any(got["hits"][:, 1] == api.MIRT_HIT_TRIANGLE)

    # a sub-range with first > 0 and a count that is not a multiple of 64
    first, count = 29, min(n - 29, 64 + 37)
    v2 = v1[first:first + count] + rng.uniform(-0.05, 0.05, (count, 9)).astype(f32)
    m.update_triangles(raw, torch.from_numpy(np.ascontiguousarray(v2)).to(DEV), first=first)
    m.build_lbvh_karas(raw)
    tri2 = _with_verts(tri1, v2, first)
    fresh = _built(_fresh_source(stl, triangles=tri2), qnodes=qnodes)
    _assert_same_tree(raw, fresh)
    _assert_same(_observe(raw, w, h, spp), _observe(fresh, w, h, spp), "sub-range of triangles moved")
    fresh.close()
    raw.close()


# ---- 4. grid flip ------------------------------------------------------------------------------------------------------------
def test_a_translation_far_from_the_origin_flips_the_quantised_grid_and_back():
    w, h, spp = 96, 54, 4
    stl = m.parseText(_sphere_cluster())
    sph0 = stl.array("spheres")
    raw = _built(stl)
    cam0 = raw.camera()
    near = _observe(raw, w, h, spp)
    assert near["st"]["node_record_bytes"] == 32                                 # the quantised records are walked

    far_x = _xyzr(sph0)
    far_x[:, 0] += f32(1e4)
    m.update_spheres(raw, torch.from_numpy(far_x).to(DEV))
    m.build_lbvh_karas(raw)
    cam_far = raw.set_camera(eye=(cam0.eye.x + 1e4, cam0.eye.y, cam0.eye.z))
    fresh = _built(_fresh_source(stl, spheres=_with_xyzr(sph0, far_x), cam=cam_far))
    got = _observe(raw, w, h, spp)
    assert got["st"]["node_record_bytes"] == 64                                  # grid_ok turned false: the exact records
    _assert_same_tree(raw, fresh)
    _assert_same(got, _observe(fresh, w, h, spp), "far scene")
    fresh.close()

    m.update_spheres(raw, torch.from_numpy(_xyzr(sph0)).to(DEV))
    m.build_lbvh_karas(raw)
    raw.set_camera(cam0)
    back = _observe(raw, w, h, spp)
    assert back["st"]["node_record_bytes"] == 32
    _assert_same(back, near, "back at the origin")
    raw.close()


# ---- 5. state and errors -----------------------------------------------------------------------------------------------------
def test_state_and_errors():
    stl = m.parseText(_mixed_scene(ns=40, nt=40))
    raw = _built(stl)
    L = m.lib()
    w, h, spp = 32, 24, 2
    n = w * h
    img = torch.empty(n * 4, dtype=torch.uint8, device=DEV)
    acc = torch.zeros(n * 4, dtype=torch.float32, device=DEV)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.zeros((n, 6), dtype=torch.int32, device=DEV)
    xyzr = torch.from_numpy(_xyzr(stl.array("spheres"))).to(DEV)
    verts = torch.from_numpy(_tri_verts(stl.array("triangles"))).to(DEV)
    sp, vp = C.c_void_p(xyzr.data_ptr()), C.c_void_p(verts.data_ptr())

    # argument errors leave the scene built
    assert L.mirt_scene_update_spheres(raw._h, sp, 1, 40, None) == 3            # a range past the end
    assert L.mirt_scene_update_spheres(raw._h, sp, -1, 4, None) == 3            # a negative first
    assert L.mirt_scene_update_spheres(raw._h, sp, 0, -1, None) == 3
    assert L.mirt_scene_update_spheres(raw._h, None, 0, 4, None) == 3           # a null pointer with count > 0
    assert L.mirt_scene_update_spheres(raw._h, C.c_void_p(xyzr.data_ptr() + 4), 0, 4, None) == 3      # 16-byte alignment
    assert L.mirt_scene_update_triangles(raw._h, vp, 1, 40, None) == 3
    assert L.mirt_scene_update_triangles(raw._h, vp, -1, 4, None) == 3
    assert L.mirt_scene_update_triangles(raw._h, vp, 0, -1, None) == 3
    assert L.mirt_scene_update_triangles(raw._h, None, 0, 4, None) == 3
    assert L.mirt_scene_update_triangles(raw._h, C.c_void_p(verts.data_ptr() + 2), 0, 4, None) == 3   # 4-byte alignment
    # count = 0 leaves the scene built (null pointer allowed)
    assert L.mirt_scene_update_spheres(raw._h, None, 0, 0, None) == 0
    assert L.mirt_scene_update_triangles(raw._h, None, 40, 0, None) == 0
    m.update_spheres(raw, xyzr[:0])
    m.update_triangles(raw, verts[:0], first=7)
    m.render(img, w, h, spp, raw)
    torch.cuda.synchronize()
    want = img.cpu().numpy().copy()

    for update in (lambda: m.update_spheres(raw, xyzr[3:8], first=3), lambda: m.update_triangles(raw, verts[5:6], first=5)):
        update()
        for call in (lambda: m.render(img, w, h, spp, raw), lambda: m.render_accumulate(acc, w, h, 0, 2, raw),
                     lambda: m.trace_rays(raw, rays, hits), lambda: m.camera_rays(raw, rays, w, h, spp), lambda: raw.tree()):
            with pytest.raises(m.MirtError) as e:
                call()
            assert e.value.status == 6
        update()                                                                 # several updates may precede one build
        m.build_lbvh_karas(raw)
        m.render(img, w, h, spp, raw)                                            # (the same values: the same frame)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy(), want)
    raw.stats()
    raw.close()


# ---- 6. frames in flight -----------------------------------------------------------------------------------------------------
def test_a_frame_in_flight_keeps_its_camera_and_its_geometry():
    w, h, spp = 1920, 1080, 16                        # large enough to still be running when the next call is made
    stl = m.parseText(_file("tenthousand"))
    text_b = _file("tenthousand") + "\n" + CAMERA_B
    stl_b = m.parseText(text_b)
    cam_a, cam_b = _camera_of(stl.desc), _camera_of(stl_b.desc)
    sph0 = stl.array("spheres")
    x1 = _moved(sph0, seed=404)
    sph1 = _with_xyzr(sph0, x1)
    n = w * h

    def alone(source):
        raw = _built(source)
        img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
        m.render(img, w, h, spp, raw)
        torch.cuda.synchronize()
        raw.stats()
        raw.close()
        return img.cpu().numpy()

    want_a, want_b = alone(stl), alone(stl_b)
    want_b_moved = alone(_fresh_source(stl, spheres=sph1, cam=cam_b))
    assert not np.array_equal(want_a, want_b) and not np.array_equal(want_b, want_b_moved)

    raw = _built(stl)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_x1 = torch.from_numpy(x1).to(DEV)
    img1 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    img2 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    img3 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    img4 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    # camera: A on s1, then -- without synchronising -- B on s2
    m.render(img1, w, h, spp, raw, stream=s1)
    raw.set_camera(cam_b)
    m.render(img2, w, h, spp, raw, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(img1.cpu().numpy(), want_a)
    assert np.array_equal(img2.cpu().numpy(), want_b)
    # geometry: a frame on s1, then update + build + render on s2
    m.render(img3, w, h, spp, raw, stream=s1)
    m.update_spheres(raw, d_x1, stream=s2)
    m.build_lbvh_karas(raw, stream=s2)
    m.render(img4, w, h, spp, raw, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(img3.cpu().numpy(), want_b)                            # the old geometry
    assert np.array_equal(img4.cpu().numpy(), want_b_moved)
    assert raw.stats()["overflow_events"] == 0
    raw.close()


def test_every_slab_of_a_frame_in_flight_keeps_its_camera():
    """A call of several slabs (slab_log2 = 22: eight launches for this frame, twice round the ring of four argument slots) issued
    with camera A, then -- while it runs -- camera B and a second call on another stream: every slab's arguments were copied when
    its call was issued, so each frame is the frame of its own camera."""
    w, h, spp = 1920, 1080, 16
    stl = m.parseText(_file("tenthousand"))
    stl_b = m.parseText(_file("tenthousand") + "\n" + CAMERA_B)
    cam_b = _camera_of(stl_b.desc)
    n = w * h

    def alone(source):
        raw = _built(source)
        img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
        m.render(img, w, h, spp, raw)
        torch.cuda.synchronize()
        raw.close()
        return img.cpu().numpy()

    want_a, want_b = alone(stl), alone(stl_b)
    raw = _built(stl, slab_log2=22)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    img1 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    img2 = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    m.render(img1, w, h, spp, raw, stream=s1)
    raw.set_camera(cam_b)
    m.render(img2, w, h, spp, raw, stream=s2)
    torch.cuda.synchronize()
    st = raw.stats()
    assert st["trace_launches"] == 8 and st["overflow_events"] == 0
    assert np.array_equal(img1.cpu().numpy(), want_a)
    assert np.array_equal(img2.cpu().numpy(), want_b)
    raw.close()


# ---- 7. the hand-out order survives ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [0, 1, 2])
def test_the_measured_hand_out_order_survives_updates(sched):
    w, h, spp = 160, 90, 16
    stl = m.parseText(_file("tenthousand"))
    stl_b = m.parseText(_file("tenthousand") + "\n" + CAMERA_B)
    cam_b = _camera_of(stl_b.desc)
    sph0 = stl.array("spheres")
    x1 = _moved(sph0, seed=505)
    raw = _built(stl, sched=sched)
    n = w * h
    img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    m.render(img, w, h, spp, raw)                                                # the order is measured here
    torch.cuda.synchronize()
    first = img.cpu().numpy().copy()
    m.update_spheres(raw, torch.from_numpy(x1).to(DEV))
    raw.set_camera(cam_b)
    m.build_lbvh_karas(raw)
    fresh = _built(_fresh_source(stl, spheres=_with_xyzr(sph0, x1), cam=cam_b), sched=0)
    ref = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
    m.render(ref, w, h, spp, fresh)
    torch.cuda.synchronize()
    want = ref.cpu().numpy()
    fresh.close()
    assert not np.array_equal(want, first)
    for k in range(2):
        img.zero_()
        m.render(img, w, h, spp, raw)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy(), want), k
    assert raw.stats()["overflow_events"] == 0
    raw.close()


# ---- 8. multi ----------------------------------------------------------------------------------------------------------------
def test_multi_set_camera_gives_the_single_gpu_frame_of_the_new_camera(monkeypatch):
    w, h, spp = 200, 111, 8
    stl = m.parseText(_file("tenthousand"))
    stl_b = m.parseText(_file("tenthousand") + "\n" + CAMERA_B)
    cam_b = _camera_of(stl_b.desc)
    single = _built(stl_b)
    img = torch.empty(w * h * 4, dtype=torch.uint8, device=DEV)
    m.render(img, w, h, spp, single)
    torch.cuda.synchronize()
    want = img.cpu().numpy().reshape(h, w, 4)
    single.close()
    monkeypatch.setenv("MIRT_MULTI_GATHER", "copy")
    mg = api.MultiGpu(stl, 2, devices=[0, 0])
    frame_a, _ = mg.render_frame(w, h, spp)
    assert not np.array_equal(frame_a, want)
    mg.set_camera(cam_b)
    frame_b, st = mg.render_frame(w, h, spp)
    assert np.array_equal(frame_b, want) and st["num_gpus"] == 2
    assert mg.stats(0)["overflow_events"] == 0 and mg.stats(1)["overflow_events"] == 0
    assert m.lib().mirt_multi_set_camera(mg._h, None) == 3
    mg.close()

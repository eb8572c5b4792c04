"""GPU: ray queries (mirt_trace_rays / mirt_camera_rays).  Camera rays followed by a closest-hit query must give the CPU oracle's
primary-hit records (OracleScene.render(..., want_aov=True), the reference's own walk) word for word; random rays are checked
against a float32 brute force restated below from struct.cu:64-163 and draw.cu:292-318, 581-615."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import edge_scenes
import oracle_lib as ol
import pyscene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
f32 = np.float32
MISS = np.array([np.float32(-1.0).view(np.uint32), 0, 0, 0, 0, 0], np.uint32)


def _scene(text, **options):
    stl = m.parseText(text)
    raw = m.initRawConfigFromStl(stl, 0)
    for k, v in options.items():
        raw.set_option(k, v)
    m.build_lbvh_karas(raw)
    return stl, raw


def _primary_hits(raw, w, h, spp, params=None):
    p = params if params is not None else api.render_params(w, h, spp)
    n = api.num_pixels(p)
    rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.full((n, 6), -7, dtype=torch.int32, device=DEV)
    m.camera_rays(raw, rays, w, h, spp, params=p)
    m.trace_rays(raw, rays, hits)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32)


def _oracle_words(text, w, h, spp):
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    aov = o.render(w, h, spp, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)["aov"]
    o.close()
    return np.ascontiguousarray(aov).reshape(-1).view(np.uint32).reshape(-1, 6)


def _assert_words(got, want, w):
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, [(int(i % w), int(i // w), got[i].tolist(), want[i].tolist()) for i in bad[:5]] + [f"{bad.size} records differ"]


def _check_primary(text, w, h, spp, **options):
    stl, raw = _scene(text, **options)
    got = _primary_hits(raw, w, h, spp)
    raw.close()
    want = _oracle_words(text, w, h, spp)
    _assert_words(got, want, w)
    return got


def _file(name):
    return open(os.path.join(ROOT, "scenes", name + ".txt")).read()


# ---- 1. camera rays + closest hit == the oracle's primary-hit records --------------------------------------------------------
@pytest.mark.parametrize("name", ["tri", "spiral", "tenthousand", "redchair"])
@pytest.mark.parametrize("spp", [0, 1, 16])
def test_primary_hits_of_bundled_scenes_match_the_oracle(name, spp):
    got = _check_primary(_file(name), 96, 54, spp)
    assert np.any(got[:, 1] != 0)


EDGE = dict(edge_scenes.ALL, far_camera=edge_scenes.far_camera, far_from_origin=edge_scenes.far_from_origin)


@pytest.mark.parametrize("name", sorted(EDGE))
@pytest.mark.parametrize("spp", [0, 8])
def test_primary_hits_of_edge_scenes_match_the_oracle(name, spp):
    got = _check_primary(EDGE[name](), 64, 48, spp)
    if name in ("empty", "zero_bounces"):
        assert np.all(got == MISS)
    if name == "plane_only":
        assert set(got[:, 1].tolist()) <= {0, 3} and np.any(got[:, 1] == 3)


@pytest.mark.parametrize("lds_depth", [2, 0])
def test_deep_stack_through_the_spill_path_matches_the_oracle(lds_depth):
    _check_primary(edge_scenes.deep_stack(), 64, 48, 0, stack_lds_depth=lds_depth)


def test_primary_hits_of_a_striped_part_match_the_oracle():
    text, w, h, spp = _file("tenthousand"), 96, 54, 16
    stl, raw = _scene(text)
    p = api.render_params(w, h, spp, stripe_rows=5, num_parts=3, part=1)
    got = _primary_hits(raw, w, h, spp, params=p)
    raw.close()
    want = _oracle_words(text, w, h, spp)
    idx = [y * w + x for x, y in (api.part_pixel_xy(p, i) for i in range(api.num_pixels(p)))]
    _assert_words(got, want[idx], w)


# ---- 2..5: random rays against a float32 brute force ---------------------------------------------------------------------------
def _random_scene_text(seed=5, ns=200, nt=200):
    rng = np.random.default_rng(seed)
    out = ["png 8 8 q.png\n", "color 1 1 1\n", "sun 1 1 1\n", "plane 0 1 0 3.5\n", "plane 0.2 0.1 1 5\n"]
    for _ in range(ns):
        c = rng.uniform(-3, 3, 3)
        out.append("sphere %.5f %.5f %.5f %.5f\n" % (c[0], c[1], c[2], rng.uniform(0.1, 0.6)))
    for k in range(nt):
        c = rng.uniform(-3, 3, 3)
        for _ in range(3):
            v = c + rng.uniform(-0.7, 0.7, 3)
            out.append("xyz %.5f %.5f %.5f\n" % tuple(v))
        out.append("tri %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
    return "".join(out)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _normalize(d):
    """vec3::normalize (vec3.cuh:72-82) in float32, one rounding per operation."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    mag = np.sqrt((x * x + y * y) + z * z)
    inv = f32(1.0) / mag
    out = np.stack([x * inv, y * inv, z * inv], axis=1)
    out[np.abs(mag) < f32(1e-6)] = 0
    return out


def _sphere_t(o, d, c, r):
    """check_sphere (struct.cu:64-109) of rays [n] against spheres [k]: t [n, k] (inf: no hit) and |t| < 1e-3 flags."""
    ox, oy, oz = (o[:, None, i] for i in range(3))
    dx, dy, dz = (d[:, None, i] for i in range(3))
    cx, cy, cz = (c[None, :, i] for i in range(3))
    r = r[None, :]
    crx, cry, crz = cx - ox, cy - oy, cz - oz
    inside = _dot(crx, cry, crz, crx, cry, crz) < r * r
    tc = _dot(crx, cry, crz, dx, dy, dz)
    vx, vy, vz = (ox + tc * dx) - cx, (oy + tc * dy) - cy, (oz + tc * dz) - cz
    d2 = _dot(vx, vy, vz, vx, vy, vz)
    with np.errstate(invalid="ignore"):
        toff = np.sqrt(r * r - d2)
    t = np.where(inside, tc + toff, tc - toff)
    hit = ~(~inside & (tc < 0)) & ~(~inside & (r * r < d2)) & (t > f32(1e-6))
    return np.where(hit, t, f32(np.inf)), hit & (t < f32(1e-3))


def _triangle_t(o, d, tr):
    """check_triangle (struct.cu:111-163): t [n, k] and a flag for hits within 1e-3 of an edge (the tolerance band outside the
    triangle, where the hit may lie outside its leaf box and the reference's walk may not see it)."""
    ox, oy, oz = (o[:, None, i] for i in range(3))
    dx, dy, dz = (d[:, None, i] for i in range(3))
    p0, nor, e1, e2 = tr["p0"], tr["nor"], tr["e1"], tr["e2"]
    px, py, pz = (p0[None, :, i] for i in range(3))
    nx, ny, nz = (nor[None, :, i] for i in range(3))
    denom = _dot(dx, dy, dz, nx, ny, nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = _dot(px - ox, py - oy, pz - oz, nx, ny, nz) / denom
    ix, iy, iz = t * dx + ox, t * dy + oy, t * dz + oz
    b1 = _dot(e1[None, :, 0], e1[None, :, 1], e1[None, :, 2], ix - px, iy - py, iz - pz)
    b2 = _dot(e2[None, :, 0], e2[None, :, 1], e2[None, :, 2], ix - px, iy - py, iz - pz)
    b0 = (f32(1.0) - b1) - b2
    eps = f32(0.001)
    hit = ~(np.abs(denom) < f32(1e-9)) & ~(t <= eps) & (b0 >= -eps) & (b1 >= -eps) & (b2 >= -eps) & (t > f32(1e-6))
    fringe = hit & (np.minimum(np.minimum(b0, b1), b2) < eps)
    return np.where(hit, t, f32(np.inf)), fringe


def _plane_t(o, d, pl):
    """checkPlane (draw.cu:581-615): t [n, k] of every plane (inf: not accepted)."""
    ox, oy, oz = (o[:, None, i] for i in range(3))
    dx, dy, dz = (d[:, None, i] for i in range(3))
    n, p = pl["nor"], pl["point"]
    nx, ny, nz = (n[None, :, i] for i in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = _dot(p[None, :, 0] - ox, p[None, :, 1] - oy, p[None, :, 2] - oz, nx, ny, nz) / _dot(dx, dy, dz, nx, ny, nz)
    ok = ~(t <= f32(1e-6)) & (t > f32(0.001)) & (t < f32(2147483648.0))
    return np.where(ok, t, f32(np.inf))


def brute_force(stl, o, dirs, chunk=4096):
    """hitNearest (draw.cu:292-318) by testing every primitive: (t, kind, id, clear) per ray; clear = the two nearest candidates
    differ by more than 1e-4 relative and the nearest is not a hit the reference's box test may reject (a triangle hit in its
    edge tolerance band, a hit within 1e-3 of the origin)."""
    sph, tri, pl = stl.array("spheres"), stl.array("triangles"), stl.array("planes")
    d = _normalize(dirs)
    n = len(o)
    T = np.full(n, np.inf, f32)
    K = np.zeros(n, np.uint32)
    I = np.zeros(n, np.uint32)
    clear = np.zeros(n, bool)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        ts, ns = _sphere_t(o[a:b], d[a:b], sph["c"], sph["r"])
        tt, ft = _triangle_t(o[a:b], d[a:b], tri)
        tp = _plane_t(o[a:b], d[a:b], pl)
        allt = np.concatenate([ts, tt, tp], axis=1)
        order = np.argsort(allt, axis=1, kind="stable")
        first = np.take_along_axis(allt, order[:, :1], axis=1)[:, 0]
        second = np.take_along_axis(allt, order[:, 1:2], axis=1)[:, 0]
        # the BVH's nearest, then the plane rule: the BVH hit wins only when strictly nearer
        prim = np.concatenate([ts, tt], axis=1)
        pj = np.argmin(prim, axis=1)
        tb = prim[np.arange(b - a), pj]
        pk = np.argmin(tp, axis=1)
        tpl = tp[np.arange(b - a), pk]
        use_b = np.isfinite(tb) & ~(np.isfinite(tpl) & ~(tb < tpl))
        hit = np.isfinite(tb) | np.isfinite(tpl)
        T[a:b] = np.where(use_b, tb, np.where(hit, tpl, np.inf))
        K[a:b] = np.where(use_b, np.where(pj < len(sph), 1, 2), np.where(hit, 3, 0))
        I[a:b] = np.where(use_b, np.where(pj < len(sph), pj, pj - len(sph)), np.where(hit, pk, 0))
        risky = np.concatenate([ns, ft, np.zeros_like(tp, bool)], axis=1)
        first_risky = np.take_along_axis(risky, order[:, :1], axis=1)[:, 0]
        with np.errstate(invalid="ignore"):
            sep = ~np.isfinite(first) | (second - first > f32(1e-4) * np.abs(first))
        clear[a:b] = sep & ~first_risky & ~(np.isfinite(first) & (first < f32(1e-3)))
    return T, K, I, clear


@pytest.fixture(scope="module")
def random_case():
    text = _random_scene_text()
    stl, raw = _scene(text)
    rng = np.random.default_rng(17)
    n = 100_000
    o = rng.uniform(-3.5, 3.5, (n, 3)).astype(f32)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dirs = (u * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (n, 1)))).astype(f32)
    # a few hundred axis-parallel directions
    ax = np.zeros((600, 3), f32)
    ax[np.arange(600), np.arange(600) % 3] = np.where(np.arange(600) % 2 == 0, 1.0, -3.0)
    dirs[:600] = ax
    bf = brute_force(stl, o, dirs)
    yield dict(stl=stl, raw=raw, o=o, dirs=dirs, bf=bf)
    raw.close()


def _trace(raw, o, dirs, tmax=float("inf"), any_hit=False):
    rays = m.pack_rays(torch.from_numpy(o).to(DEV), torch.from_numpy(dirs).to(DEV), torch.as_tensor(tmax, dtype=torch.float32).to(DEV))
    hits = torch.full((len(o), 6), -7, dtype=torch.int32, device=DEV)
    m.trace_rays(raw, rays, hits, any_hit=any_hit)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32)


def _ulps(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_random_rays_match_the_brute_force(random_case):
    c = random_case
    T, K, I, clear = c["bf"]
    got = _trace(c["raw"], c["o"], c["dirs"])
    gt, gk, gi = got[:, 0].view(f32), got[:, 1], got[:, 2]
    assert clear.mean() > 0.98, clear.mean()
    assert np.count_nonzero(K == 1) > 1000 and np.count_nonzero(K == 2) > 1000 and np.count_nonzero(K == 3) > 1000
    cl = np.nonzero(clear)[0]
    bad = cl[(gk[cl] != K[cl]) | (gi[cl] != I[cl])]
    assert bad.size == 0, [(int(i), int(gk[i]), int(gi[i]), float(gt[i]), int(K[i]), int(I[i]), float(T[i])) for i in bad[:5]]
    same = cl[K[cl] != 0]
    assert np.all(_ulps(gt[same], T[same]) <= 2), float(np.max(_ulps(gt[same], T[same])))
    assert np.array_equal(gk[cl] == 0, K[cl] == 0)
    assert np.all(got[gk == 0] == MISS)
    # (the axis-parallel rays are among them)
    assert np.all(clear[:600] | (K[:600] == 0)) or clear[:600].mean() > 0.95


def test_tmax_bounds_the_closest_hit(random_case):
    c = random_case
    rng = np.random.default_rng(23)
    tmax = rng.uniform(0.0, 12.0, len(c["o"])).astype(f32)
    full = _trace(c["raw"], c["o"], c["dirs"])
    bounded = _trace(c["raw"], c["o"], c["dirs"], tmax)
    t = full[:, 0].view(f32)
    inside = (full[:, 1] != 0) & (t < tmax)
    assert 0.1 < inside.mean() < 0.9
    assert np.array_equal(bounded[inside], full[inside])
    assert np.all(bounded[~inside] == MISS)


def test_occlusion_is_the_bounded_closest_hit_boolean(random_case):
    c = random_case
    stl = c["stl"]
    rng = np.random.default_rng(29)
    tmax = rng.uniform(0.0, 12.0, len(c["o"])).astype(f32)
    tmax[:1000] = np.inf
    closest = _trace(c["raw"], c["o"], c["dirs"], tmax)
    anyh = _trace(c["raw"], c["o"], c["dirs"], tmax, any_hit=True)
    assert np.array_equal(anyh[:, 1] != 0, closest[:, 1] != 0)
    hit = np.nonzero(anyh[:, 1] != 0)[0]
    t = anyh[hit, 0].view(f32)
    assert np.all(t < tmax[hit])
    # the reported primitive is a real hit of that ray
    d = _normalize(c["dirs"][hit])
    o = c["o"][hit]
    kind, pid = anyh[hit, 1], anyh[hit, 2]
    sph, tri, pl = stl.array("spheres"), stl.array("triangles"), stl.array("planes")
    want = np.full(len(hit), np.nan, f32)
    for k, arr, fn in ((1, sph, lambda oo, dd, a: _sphere_t(oo, dd, a["c"], a["r"])[0]), (2, tri, lambda oo, dd, a: _triangle_t(oo, dd, a)[0]),
                       (3, pl, lambda oo, dd, a: _plane_t(oo, dd, a))):
        for j in np.unique(pid[kind == k]):
            sel = np.nonzero((kind == k) & (pid == j))[0]
            want[sel] = fn(o[sel], d[sel], arr[j:j + 1])[:, 0]
    assert np.all(np.isfinite(want))
    assert np.all(_ulps(t, want) <= 2), float(np.max(_ulps(t, want)))
    assert np.any(kind == 1) and np.any(kind == 2) and np.any(kind == 3)


def test_edge_rays(random_case):
    c = random_case
    raw = c["raw"]
    o, dirs = c["o"][:64].copy(), c["dirs"][:64].copy()
    for tm in (0.0, -1.0, np.nan):
        assert np.all(_trace(raw, o, dirs, tm) == MISS)
        assert np.all(_trace(raw, o, dirs, tm, any_hit=True) == MISS)
    dz = np.zeros_like(dirs)
    dz[1::2] = np.nan
    dz[2] = [np.nan, 0, 1]
    dz[3] = [1e-8, 0, 0]
    assert np.all(_trace(raw, o, dz) == MISS)
    assert np.all(_trace(raw, o, dz, any_hit=True) == MISS)
    # num_rays 0, 1, 65 (sub-batches give the rows of the whole batch)
    full = _trace(raw, c["o"][:200], c["dirs"][:200])
    for n in (1, 65):
        assert np.array_equal(_trace(raw, c["o"][:n], c["dirs"][:n]), full[:n])
    rays = m.pack_rays(torch.from_numpy(o).to(DEV), torch.from_numpy(dirs).to(DEV))
    hits = torch.full((64, 6), -7, dtype=torch.int32, device=DEV)
    assert m.lib().mirt_trace_rays(raw._h, C.c_void_p(rays.data_ptr()), 0, C.c_void_p(hits.data_ptr()), 0, None) == 0
    torch.cuda.synchronize()
    assert torch.all(hits == -7)
    m.trace_rays(raw, rays[:0], hits[:0])
    torch.cuda.synchronize()
    assert torch.all(hits == -7)


# ---- 6. isolation from a frame in flight --------------------------------------------------------------------------------------
def test_queries_on_another_stream_leave_a_render_in_flight_unchanged():
    stl, raw = _scene(_file("tenthousand"))
    w, h, spp = 320, 180, 16
    p = api.render_params(w, h, spp, counters=True)
    n = api.num_pixels(p)
    crays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keys = ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack", "rays_traversed", "overflow_events")

    def frame(queries):
        img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
        m.render(img, w, h, spp, raw, params=p, stream=s1)
        if queries:
            for k in range(6):
                m.camera_rays(raw, crays, w, h, spp, stream=s2)
                m.trace_rays(raw, crays, hits, any_hit=bool(k % 2), stream=s2)
        torch.cuda.synchronize()
        st = raw.stats()
        return img.cpu().numpy(), {k: st[k] for k in keys}

    img0, st0 = frame(False)
    img1, st1 = frame(True)
    img2, st2 = frame(False)
    raw.close()
    assert np.array_equal(img0, img1) and np.array_equal(img0, img2)
    assert st0 == st1 == st2
    assert st0["samples"] == n * spp


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------
def test_errors():
    stl = m.parseText(_random_scene_text(ns=10, nt=10))
    raw = m.initRawConfigFromStl(stl, 0)
    rays = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    rays[:, 6] = 1.0
    hits = torch.zeros((4, 6), dtype=torch.int32, device=DEV)
    with pytest.raises(m.MirtError) as e:
        m.trace_rays(raw, rays, hits)
    assert e.value.status == 6
    m.build_lbvh_karas(raw)
    L = m.lib()
    for flags in (2, 0x80000000, 3):
        assert L.mirt_trace_rays(raw._h, C.c_void_p(rays.data_ptr()), 4, C.c_void_p(hits.data_ptr()), flags, None) == 3
    assert L.mirt_trace_rays(raw._h, C.c_void_p(rays.data_ptr()), -1, C.c_void_p(hits.data_ptr()), 0, None) == 3
    assert L.mirt_trace_rays(raw._h, None, 4, C.c_void_p(hits.data_ptr()), 0, None) == 3
    assert L.mirt_trace_rays(raw._h, C.c_void_p(rays.data_ptr()), 4, None, 0, None) == 3
    m.trace_rays(raw, rays, hits)
    torch.cuda.synchronize()
    raw.close()

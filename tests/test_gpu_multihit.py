"""Multi-hit ray queries on the GPU (include/mirt_multihit.h: mirt_trace_rays_multi; multihit.trace_rays_multi, count_hits).  The
yardstick is tests/multihit_ref.py, the numpy restatement of the header, over the tree the library built (mirt_get_tree): every
word of every one of the k records and every count is compared, the outputs pre-filled with a sentinel.  Ties to code that is
verified already -- mirt_trace_rays, the oracle's primary hits -- hold on the rays the header calls regular."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api, multihit
import edge_scenes
import multihit_ref as mr
import oracle_lib as ol
import pyscene
from test_multihit_abi import IRREGULAR_CAP, INF, TWINS, case_input, dense_rays, pack, twin_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
f32 = np.float32
SENTINEL = -7


class Scene:
    """A built scene with what the reference needs: the host arrays and the library's tree."""

    def __init__(self, text, **options):
        self.stl = m.parseText(text)
        self.raw = m.initRawConfigFromStl(self.stl, 0)
        for k, v in options.items():
            self.raw.set_option(k, v)
        m.build_lbvh_karas(self.raw)
        self.arrays = {k: self.stl.array(k).copy() for k in ("spheres", "triangles", "planes")}
        nodes, _, refs, _ = self.raw.tree()
        self.nodes, self.refs = nodes, refs

    def want(self, rays, k):
        return mr.multihit(self.arrays, rays, self.nodes, self.refs, k)

    def close(self):
        self.raw.close()


def _multi(raw, rays, k, counts=True, stream=None):
    """mirt_trace_rays_multi on numpy rays: (hits uint32 [n, k, 6] or None for k = 0, counts uint32 [n] or None); the slots after
    the last ray keep their sentinel."""
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, f32)).to(DEV)
    hits = torch.full((n + 1, k, 6), SENTINEL, dtype=torch.int32, device=DEV) if k else None
    cnt = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV) if counts else None
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.trace_rays_multi(raw, d_rays, hits[:n] if k else None, cnt[:n] if counts else None, stream=stream)
    torch.cuda.synchronize()
    assert (hits is None or bool(torch.all(hits[n] == SENTINEL))) and (cnt is None or int(cnt[n]) == SENTINEL)
    return (hits[:n].cpu().numpy().view(np.uint32) if k else None), (cnt[:n].cpu().numpy().view(np.uint32) if counts else None)


def _trace(raw, rays, any_hit=False):
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, f32)).to(DEV)
    hits = torch.full((len(rays), 6), SENTINEL, dtype=torch.int32, device=DEV)
    m.trace_rays(raw, d_rays, hits, any_hit=any_hit)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32)


def _assert_equal(hits, counts, want_hits, want_counts, rays=None):
    bad = np.flatnonzero(counts != want_counts)
    assert len(bad) == 0, (len(bad), bad[:5], counts[bad[:5]], want_counts[bad[:5]], None if rays is None else rays[bad[:5]])
    if hits is not None:
        bad = np.flatnonzero(np.any(hits.reshape(len(hits), -1) != want_hits.reshape(len(hits), -1), axis=1))
        assert len(bad) == 0, (len(bad), bad[:3], hits[bad[:3]], want_hits[bad[:3]], None if rays is None else rays[bad[:3]])


def _check_all_k(sc, rays, ks=(1, 4, 8, 0)):
    """Every k against the reference, bit for bit; then, on the GPU's own outputs, the k-prefix property and the k-independence of
    the counts, and the call without d_counts.  Returns (hits of k = 8, counts, regular)."""
    want8, want_counts, regular = sc.want(rays, 8)
    got = {}
    for k in ks:
        hits, counts = _multi(sc.raw, rays, k)
        _assert_equal(hits, counts, want8[:, :k] if k else None, want_counts, rays)
        got[k] = (hits, counts)
    for k in ks:
        assert np.array_equal(got[k][1], got[ks[0]][1])
        if k and 8 in got:
            assert np.array_equal(got[k][0], got[8][0][:, :k])
    only_hits, none = _multi(sc.raw, rays, 4, counts=False)
    assert none is None and np.array_equal(only_hits, want8[:, :4])
    # a d_hits that is 4-byte aligned and no more
    n = len(rays)
    flat = torch.full((n * 3 * 6 + 2,), SENTINEL, dtype=torch.int32, device=DEV)
    odd = flat[1:-1].view(n, 3, 6)
    assert odd.data_ptr() % 8 == 4
    m.trace_rays_multi(sc.raw, torch.from_numpy(np.ascontiguousarray(rays, f32)).to(DEV), odd)
    torch.cuda.synchronize()
    assert int(flat[0]) == SENTINEL and int(flat[-1]) == SENTINEL and np.array_equal(odd.cpu().numpy().view(np.uint32), want8[:, :3])
    return want8, want_counts, regular


def _assert_ties_to_trace_rays(sc, rays, hits8, counts, regular, cap):
    """On regular rays record 0 is mirt_trace_rays' closest hit with the same tmax and count > 0 its any-hit boolean."""
    assert 1.0 - regular.mean() <= cap
    closest = _trace(sc.raw, rays)
    anyhit = _trace(sc.raw, rays, any_hit=True)
    bad = np.flatnonzero(regular & np.any(hits8[:, 0] != closest, axis=1))
    assert len(bad) == 0, (len(bad), bad[:3], hits8[bad[:3], 0], closest[bad[:3]])
    assert np.array_equal((counts > 0)[regular], (anyhit[:, 1] != 0)[regular])
    return int(np.count_nonzero(np.any(hits8[:, 0] != closest, axis=1)))


# ---- 1. scene A: dense, truncated, full and empty lists ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    sc = Scene(case_input("A_inf")[0])
    yield sc
    sc.close()


def _dense_rays(variant):
    if variant == "random":
        rays = dense_rays(INF)
        rays[:, 3] = np.random.default_rng(20).uniform(0, 12, len(rays)).astype(f32)
        return rays
    return case_input("A_inf" if variant == "inf" else "A_2.5")[1]


@pytest.mark.parametrize("variant", ["inf", "2.5", "random"])
def test_dense_scene_every_k_equals_the_reference_and_ties_to_trace_rays(dense, variant):
    rays = _dense_rays(variant)
    hits8, counts, regular = _check_all_k(dense, rays)
    assert np.mean(counts > 8) > (0.15 if variant == "inf" else 0.05) and np.mean(counts == 0) > 0.01 and np.any((counts > 0) & (counts < 4))
    assert set(hits8[:, :, 1].reshape(-1).tolist()) == {0, 1, 2, 3}
    differ = _assert_ties_to_trace_rays(dense, rays, hits8, counts, regular, 0.01)
    print(f"A {variant}: mean count {counts.mean():.2f}, max {counts.max()}, irregular {int((~regular).sum())}, record 0 differs from trace_rays on {differ} rays")
    # count_hits is the k = 0 call; unpack_hits reads the flattened records
    d_rays = torch.from_numpy(rays).to(DEV)
    c = m.count_hits(dense.raw, d_rays)
    assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy().view(np.uint32), counts)
    d_hits = torch.empty((len(rays), 8, 6), dtype=torch.float32, device=DEV)
    m.trace_rays_multi(dense.raw, d_rays, d_hits)
    t, kind, pid, nn = m.unpack_hits(d_hits.reshape(-1, 6))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), hits8[:, :, 0].reshape(-1)) and np.array_equal(kind.cpu().numpy().view(np.uint32), hits8[:, :, 1].reshape(-1))


# ---- 2. scene C: the nest, through the LDS stack and the spill path ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nest_want():
    text, rays = case_input("C")
    sc = Scene(text)
    try:
        return sc.want(rays, 8)
    finally:
        sc.close()


@pytest.mark.parametrize("depth", [None, 2, 0])
def test_deep_stack_and_the_spill_path(depth):
    text, rays = case_input("C")
    want8, want_counts, regular = _nest_want()
    sc = Scene(text)
    try:
        assert sc.raw.get_option("stack_lds_depth") not in (0, 2)
        if depth is not None:
            sc.raw.set_option("stack_lds_depth", depth)
        for k in (8, 0):
            hits, counts = _multi(sc.raw, rays, k)
            _assert_equal(hits, counts, want8 if k else None, want_counts, rays)
        assert np.all(counts == 600)
        if depth is None:
            _assert_ties_to_trace_rays(sc, rays, want8, want_counts, regular, IRREGULAR_CAP["C"])
    finally:
        sc.close()


# ---- 3. scene B: far from the origin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B_1e3", "B_1e5"])
def test_far_from_origin(name):
    text, rays = case_input(name)
    sc = Scene(text)
    try:
        hits8, counts, regular = _check_all_k(sc, rays, ks=(8, 1, 0))
        differ = _assert_ties_to_trace_rays(sc, rays, hits8, counts, regular, IRREGULAR_CAP[name])
    finally:
        sc.close()
    print(f"{name}: mean count {counts.mean():.2f}, irregular {int((~regular).sum())} of {len(rays)}, record 0 differs from trace_rays on {differ} rays")
    assert np.mean(counts > 1) > 0.2


# ---- 4. the smallest scenes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "plane_only", "single_sphere", "single_triangle"])
def test_smallest_scenes(name):
    rng = np.random.default_rng(5)
    n = 300
    o = rng.uniform(-1.5, 1.5, (n, 3))
    target = np.array([0, 0, -2.0]) + rng.normal(size=(n, 3)) * 0.6
    rays = pack(o.astype(f32), (target - o).astype(f32), INF)
    rays[:20, 0:3] = np.array([0.1, 0.2, -2.1], f32)      # from inside the sphere of single_sphere
    rays[::7, 3] = 2.0
    sc = Scene(edge_scenes.ALL[name]())
    try:
        hits8, counts, regular = _check_all_k(sc, rays)
        _assert_ties_to_trace_rays(sc, rays, hits8, counts, regular, 0.01)
    finally:
        sc.close()
    kinds = set(hits8[:, :, 1].reshape(-1).tolist())
    assert kinds == {"empty": {0}, "plane_only": {0, 3}, "single_sphere": {0, 1}, "single_triangle": {0, 2}}[name]
    assert counts.max() == (0 if name == "empty" else 1)
    if name == "single_sphere":
        inside = (rays[:20, 3] == np.inf)
        assert np.all(counts[:20][inside] == 1) and np.all(hits8[:20, 0, 1][inside] == 1)      # the far side, seen from inside


def test_a_duplicated_sphere_is_seen_twice_in_sorted_leaf_order():
    sc = Scene(TWINS)
    try:
        hits8, counts, _ = _check_all_k(sc, twin_rays())
        order = [int(i) for i in sc.refs["id"] if i in (1, 3)]
    finally:
        sc.close()
    assert counts.tolist() == [2, 2, 0]
    for r in (0, 1):
        assert hits8[r, :2, 2].tolist() == order and hits8[r, 0, 0] == hits8[r, 1, 0]


# ---- 5. row counts --------------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_a_wave_a_block_and_a_grid(dense):
    rays = case_input("A_2.5")[1]
    want8, want_counts, _ = dense.want(rays, 8)
    for n in (1, 63, 64, 65, 255, 257):
        for k in (4, 0):
            hits, counts = _multi(dense.raw, rays[:n], k)
            _assert_equal(hits, counts, want8[:n, :k] if k else None, want_counts[:n])
    # more rays than a grid's worth of lanes: every lane takes a second ray
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 8 * 256 + len(rays) + 37
    reps = -(-n // len(rays))
    tiled = np.tile(rays, (reps, 1))[:n]
    for k in (8, 1, 0):
        hits, counts = _multi(dense.raw, tiled, k)
        assert np.array_equal(counts, np.tile(want_counts, reps)[:n])
        assert hits is None or np.array_equal(hits, np.tile(want8[:, :k], (reps, 1, 1))[:n])


# ---- 6. camera rays against the oracle's primary hits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("tri", 96, 54), ("redchair", 48, 27)])
def test_camera_rays_with_k_1_equal_the_oracles_primary_hits(name, w, h):
    text = open(os.path.join(ROOT, "scenes", name + ".txt")).read()
    o = ol.OracleScene(pyscene.parse_lines(text.split("\n")), bounds_mode=0)
    aov = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)["aov"]
    o.close()
    want = np.ascontiguousarray(aov).reshape(-1).view(np.uint32).reshape(-1, 6)
    sc = Scene(text)
    try:
        d_rays = torch.empty((w * h, 8), dtype=torch.float32, device=DEV)
        m.camera_rays(sc.raw, d_rays, w, h, 0)
        torch.cuda.synchronize()
        rays = d_rays.cpu().numpy()
        hits, counts = _multi(sc.raw, rays, 1)
        want1, want_counts, regular = sc.want(rays, 1)
    finally:
        sc.close()
    _assert_equal(hits, counts, want1, want_counts, rays)
    print(f"{name}: irregular {int((~regular).sum())} of {len(rays)}, record 0 differs from the oracle on {int(np.count_nonzero(np.any(hits[:, 0] != want, axis=1)))}")
    assert 1.0 - regular.mean() <= 0.01
    bad = np.flatnonzero(regular & np.any(hits[:, 0] != want, axis=1))
    assert len(bad) == 0, (len(bad), bad[:3], hits[bad[:3], 0], want[bad[:3]])
    assert np.any(want[:, 1] != 0) and counts.max() > 1


# ---- 7. edge rays ---------------------------------------------------------------------------------------------------------------------------
def test_edge_rays_are_not_live(dense):
    base = case_input("A_inf")[1][:64].copy()
    for tm in (0.0, -1.0, np.nan):
        rays = base.copy()
        rays[:, 3] = tm
        hits, counts = _multi(dense.raw, rays, 8)
        assert np.all(hits == mr.MISS) and np.all(counts == 0)
        assert np.all(_multi(dense.raw, rays, 0)[1] == 0)
    rays = base.copy()
    rays[:, 4:7] = 0
    rays[1::2, 4:7] = np.nan
    rays[2, 4:7] = [np.nan, 0, 1]
    rays[3, 4:7] = [1e-8, 0, 0]
    hits, counts = _multi(dense.raw, rays, 4)
    assert np.all(hits == mr.MISS) and np.all(counts == 0)
    want4, want_counts, _ = dense.want(rays, 4)
    assert np.all(want4 == mr.MISS) and np.all(want_counts == 0)
    # num_rays == 0 writes nothing
    d_rays = torch.from_numpy(base).to(DEV)
    d_hits = torch.full((64, 4, 6), SENTINEL, dtype=torch.int32, device=DEV)
    d_counts = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    L = multihit.lib()
    assert L.mirt_trace_rays_multi(dense.raw._h, C.c_void_p(d_rays.data_ptr()), 0, 4, C.c_void_p(d_hits.data_ptr()), C.c_void_p(d_counts.data_ptr()), 0, None) == 0
    m.trace_rays_multi(dense.raw, d_rays[:0], d_hits[:0], d_counts[:0])
    torch.cuda.synchronize()
    assert bool(torch.all(d_hits == SENTINEL)) and bool(torch.all(d_counts == SENTINEL))


# ---- 8. after an update in place; beside a frame in flight ----------------------------------------------------------------------------------
def test_query_follows_geometry_updated_in_place():
    text = case_input("B_1e3")[0]
    rays = case_input("B_1e3")[1]
    lines = text.split("\n")
    first = next(i for i, l in enumerate(lines) if l.startswith("sphere "))
    moved_line = "sphere 1000.2 0.1 -0.3 0.4"
    moved = "\n".join(lines[:first] + [moved_line] + lines[first + 1:])
    sc = Scene(text)
    try:
        before, before_counts = _multi(sc.raw, rays, 8)
        m.update_spheres(sc.raw, torch.tensor([[1000.2, 0.1, -0.3, 0.4]], dtype=torch.float32, device=DEV), first=0)
        with pytest.raises(m.MirtError) as e:      # updated, not yet built
            m.count_hits(sc.raw, torch.from_numpy(rays).to(DEV))
        assert e.value.status == 6 and b"mirt_trace_rays_multi" in m.lib().mirt_last_error()
        m.build_lbvh_karas(sc.raw)
        hits, counts = _multi(sc.raw, rays, 8)
        on_stream, counts_s = _multi(sc.raw, rays, 8, stream=torch.cuda.Stream())
    finally:
        sc.close()
    fresh = Scene(moved)
    try:
        fresh_hits, fresh_counts = _multi(fresh.raw, rays, 8)
        want8, want_counts, _ = fresh.want(rays, 8)
    finally:
        fresh.close()
    _assert_equal(fresh_hits, fresh_counts, want8, want_counts, rays)
    assert np.array_equal(hits, fresh_hits) and np.array_equal(counts, fresh_counts) and not np.array_equal(hits, before)
    assert np.array_equal(on_stream, hits) and np.array_equal(counts_s, counts)


def test_queries_on_another_stream_leave_a_render_in_flight_unchanged():
    stl = m.parseText(open(os.path.join(ROOT, "scenes", "tenthousand.txt")).read())
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    w, h, spp = 320, 180, 16
    p = api.render_params(w, h, spp, counters=True)
    n = api.num_pixels(p)
    crays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = {k: torch.empty((n, k, 6), dtype=torch.int32, device=DEV) for k in (8, 4, 1)}
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keys = ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack", "rays_traversed", "overflow_events")

    def frame(queries):
        img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
        m.render(img, w, h, spp, raw, params=p, stream=s1)
        if queries:
            for k in (8, 4, 1, 0, 8, 0):
                m.camera_rays(raw, crays, w, h, spp, stream=s2)
                m.trace_rays_multi(raw, crays, hits.get(k), counts, stream=s2)
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
    assert int(counts.max()) > 1


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    raw = m.initRawConfigFromStl(m.parseText(TWINS), 0)
    try:
        n, k = 8, 4
        R = torch.zeros((4 * n, 8), dtype=torch.float32, device=DEV)
        Hh = torch.full((4 * n * k, 6), SENTINEL, dtype=torch.int32, device=DEV)
        Cn = torch.full((4 * n,), SENTINEL, dtype=torch.int32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.trace_rays_multi(raw, R[:n], Hh[:n * k].reshape(n, k, 6), Cn[:n])
        assert e.value.status == 6 and b"mirt_trace_rays_multi" in m.lib().mirt_last_error()
        m.build_lbvh_karas(raw)
        L = multihit.lib()
        pR, pH, pC = R.data_ptr(), Hh.data_ptr(), Cn.data_ptr()
        vp = lambda a: C.c_void_p(a) if a else None

        def call(r=pR, count=n, kk=k, h=pH, c=pC, flags=0):
            return L.mirt_trace_rays_multi(raw._h, vp(r), count, kk, vp(h), vp(c), flags, None)

        def refused(**kw):
            rc = call(**kw)
            return rc == 3 and b"mirt_trace_rays_multi" in m.lib().mirt_last_error()

        assert refused(count=-1)
        assert refused(kk=-1) and refused(kk=9) and refused(kk=1 << 30)
        for flags in (1, 2, 0x80000000):
            assert refused(flags=flags)
        assert refused(r=0) and refused(h=0) and refused(kk=0, c=0) and refused(kk=0, h=0, c=0) and refused(r=0, h=0, c=0)
        assert refused(r=pR + 4) and refused(r=pR + 8) and refused(h=pH + 2) and refused(c=pC + 2) and refused(c=pC + 1)
        assert refused(h=pR) and refused(h=pR + 32 * n - 4) and refused(r=pH + 24 * n * k - 16, h=pH)      # hits over the rays
        assert refused(c=pR) and refused(c=pR + 32 * n - 4) and refused(r=pC + 16, c=pC)   # counts over the rays
        assert refused(c=pH) and refused(c=pH + 24 * n * k - 4) and refused(h=pC + 4 * n - 4)              # counts over the hits
        assert refused(kk=0, c=pR + 16)                                                                     # ... with k = 0 too
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == SENTINEL)) and bool(torch.all(Cn == SENTINEL))      # nothing ran
        assert call(count=0) == 0 and call(r=0, count=0, h=0, c=0) == 0 and call(r=0, count=0, kk=0, h=0, c=0) == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh == SENTINEL)) and bool(torch.all(Cn == SENTINEL))
        # adjacent is not overlapping; the counts are optional with k > 0, the hits with k == 0;
        # d_hits needs 4-byte alignment only
        assert call(h=pR + 32 * n) == 0 and call(c=pR + 32 * n) == 0 and call(c=0) == 0 and call(kk=0, h=0) == 0
        assert call(h=pH + 4) == 0 and call(c=pH + 24 * n * k) == 0 and call() == 0
        torch.cuda.synchronize()
        assert bool(torch.all(Hh[:n * k, 1] == 0)) and bool(torch.all(Cn[:n] == 0))      # rows of zeros have tmax = 0: misses
    finally:
        raw.close()

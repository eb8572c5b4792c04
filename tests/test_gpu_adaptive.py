"""Adaptive sampling on the GPU (include/mirt.h: mirt_render_accumulate_pixels, mirt_select_pixels, mirt_finalize_counts;
api.render_adaptive; `raytracer --adaptive`).  The yardstick is the dense call: what a call with a pixel list adds to a listed
pixel is, bit for bit, what mirt_render_accumulate adds to it, and nothing else is touched; the second moment and the selection
are compared with == against numpy float32 restatements of their definitions."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import oracle_lib as ol
import shade_scenes
from conftest import scene_path
from gpu_case import options

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4          # test_gpu_parity.py: linear float RGBA within 1e-4 per channel and sample
PREFILL = 0.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_ray_tracer_amd", "_build", "raytracer")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def random_list(n, fraction, seed):
    """A fixed-seed random `fraction` of the pixels [0, n) that includes pixel 0 and the last one, shuffled."""
    rng = np.random.default_rng(seed)
    k = max(2, int(round(fraction * n)))
    inner = rng.choice(np.arange(1, n - 1), size=k - 2, replace=False)
    lst = np.concatenate([[0, n - 1], inner]).astype(np.int32)
    rng.shuffle(lst)
    return lst


def dense(raw, p, w, h, first, count, prefill=0.0):
    n = api.num_pixels(p)
    acc = torch.full((4 * n,), prefill, dtype=torch.float32, device=DEV)
    m.render_accumulate(acc, w, h, first, count, raw, params=p)
    torch.cuda.synchronize()
    return acc.cpu().numpy().reshape(n, 4)


def sparse(raw, p, w, h, first, count, lst, prefill=0.0, sq=True, cnt=True, extra=0):
    """render_accumulate_pixels on prefilled buffers: (accum [n, 4], accum_sq [n, 4] or None, counts [n] or None)."""
    n = api.num_pixels(p)
    acc = torch.full((4 * n,), prefill, dtype=torch.float32, device=DEV)
    asq = torch.full((4 * n,), prefill, dtype=torch.float32, device=DEV) if sq else None
    cn = torch.full((n,), 7, dtype=torch.int32, device=DEV) if cnt else None
    pixels = None if lst is None else torch.as_tensor(np.asarray(lst, dtype=np.int32), device=DEV)
    m.render_accumulate_pixels(raw, acc, w, h, first, count, pixels, asq, cn, params=p)
    torch.cuda.synchronize()
    return (acc.cpu().numpy().reshape(n, 4), asq.cpu().numpy().reshape(n, 4) if sq else None, cn.cpu().numpy() if cnt else None)


def check_sparse_equals_dense(raw, w, h, first, count, p=None, seed=1):
    p = p if p is not None else api.render_params(w, h, max(first + count, 2))
    n = api.num_pixels(p)
    lst = random_list(n, 0.3, seed)
    want = dense(raw, p, w, h, first, count, PREFILL)
    acc, asq, cn = sparse(raw, p, w, h, first, count, lst, PREFILL)
    listed = np.zeros(n, bool)
    listed[lst] = True
    assert np.array_equal(bits(acc[listed]), bits(want[listed]))
    assert np.all(acc[~listed] == PREFILL) and np.all(asq[~listed] == PREFILL) and np.all(cn[~listed] == 7)
    assert np.all(cn[listed] == 7 + count)
    # the second moment of a listed pixel is the one the call without a list (every pixel, the dense path) gives it
    _, want_sq, _ = sparse(raw, p, w, h, first, count, None, PREFILL)
    assert np.array_equal(bits(asq[listed]), bits(want_sq[listed]))


# ---- 1. sparse equals dense -------------------------------------------------------------------------------------------------
RANGES = [(0, 16), (3, 5), (0, 100)]      # the tree resolve, a count that is no power of two, the P > 64 form


@pytest.mark.parametrize("first,count", RANGES)
@pytest.mark.parametrize("name,w,h", [("tenthousand", 96, 54), ("redchair", 64, 36), ("spiral", 48, 27)])
def test_a_listed_pixel_gets_the_bits_of_the_dense_call_and_no_other_pixel_is_touched(name, w, h, first, count, gpu_scenes):
    """Quantised records (tenthousand, spiral) and exact records with triangles (redchair)."""
    stl, raw = gpu_scenes(name)
    check_sparse_equals_dense(raw, w, h, first, count)


@pytest.mark.parametrize("first,count", RANGES)
def test_sparse_equals_dense_on_a_glass_and_gi_scene(first, count):
    """The kernels with a pending-children list (refraction and gi rays)."""
    case = shade_scenes.ALL["gi_chain_g3_b4"]
    stl = m.parseText(case.text)
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        m.build_lbvh_karas(raw)
        check_sparse_equals_dense(raw, case.w, case.h, first, count)
        assert raw.stats()["overflow_events"] == 0
    finally:
        raw.close()


@pytest.mark.parametrize("opts", [dict(stack_lds_depth=2), dict(slab_log2=8), dict(specialise=0)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_sparse_equals_dense_under_scene_options(opts, gpu_scenes):
    """The global stack-spill path, a call of several slabs (2^8 samples each: the list is cut by pixel range), the general kernel."""
    stl, raw = gpu_scenes("tenthousand")
    with options(raw, **opts):
        check_sparse_equals_dense(raw, 96, 54, 0, 16, seed=2)
        if "slab_log2" in opts:
            assert raw.stats()["trace_launches"] > 1


def test_sparse_equals_dense_on_a_striped_part(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    p = api.render_params(96, 54, 16, 4, 3, 1)
    check_sparse_equals_dense(raw, 96, 54, 0, 16, p=p, seed=3)


# ---- 2. the list decides the work ----------------------------------------------------------------------------------------------
def test_only_the_listed_pixels_are_traced(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    w, h, count = 96, 54, 16
    p = api.render_params(w, h, count, counters=True)
    n = api.num_pixels(p)
    dense(raw, p, w, h, 0, count)
    full = raw.stats()
    lst = random_list(n, 0.3, 4)
    sparse(raw, p, w, h, 0, count, lst)
    st = raw.stats()
    assert full["samples"] == n * count
    assert st["samples"] == len(lst) * count
    assert 0 < st["rays"] < full["rays"]


# ---- 3. against the oracle -------------------------------------------------------------------------------------------------------
def test_two_sparse_passes_match_the_oracle(gpu_scenes, oracle_scenes):
    stl, raw = gpu_scenes("redchair")
    w, h = 48, 27
    n = w * h
    p = api.render_params(w, h, 16)
    acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    lists = [random_list(n, 0.3, 5), random_list(n, 0.5, 6)]
    added = np.zeros(n, np.int64)
    for (first, count), lst in zip([(0, 8), (8, 8)], lists):
        m.render_accumulate_pixels(raw, acc, w, h, first, count, torch.as_tensor(lst, device=DEV), params=p)
        added[lst] += count
    torch.cuda.synchronize()
    got = acc.cpu().numpy().reshape(n, 4).astype(np.float64)
    o = oracle_scenes("redchair")
    want = np.zeros((n, 4), np.float64)
    for (first, count), lst in zip([(0, 8), (8, 8)], lists):
        oacc = np.zeros((h, w, 4), np.float32)
        o.render_accumulate(oacc, w, h, first, count, flags=ol.PRODUCT_FLAGS, nthreads=8)
        want[lst] += oacc.reshape(n, 4)[lst]
    assert set(np.unique(added)) == {0, 8, 16}
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= TOL * added), float((err - TOL * added).max())
    assert np.all(got[added == 0] == 0.0)


# ---- 4. moments ------------------------------------------------------------------------------------------------------------------
def butterfly(values):
    """`for (mask = P / 2; mask > 0; mask /= 2) v += shfl_xor(v, mask)` as lane 0 sees it (draw.cu:181-189) in float32: values
    [count, ...], absent lanes 0, P the next power of two."""
    count = values.shape[0]
    P = 1
    while P < count:
        P *= 2
    v = np.zeros((P,) + values.shape[1:], np.float32)
    v[:count] = values
    mask = P // 2
    while mask > 0:
        v = (v + v[np.arange(P) ^ mask]).astype(np.float32)
        mask //= 2
    return v[0]


@pytest.mark.parametrize("count", [16, 5, 100])
def test_second_moment_is_the_butterfly_sum_of_the_squared_samples(count, gpu_scenes):
    stl, raw = gpu_scenes("tri")
    w = h = 40
    n = w * h
    p = api.render_params(w, h, max(count, 2))
    lst = random_list(n, 0.3, 7)
    first = 2
    acc, asq, cn = sparse(raw, p, w, h, first, count, lst)      # (first: the random-number tables it makes serve the single samples too)
    per_sample = np.stack([sparse(raw, p, w, h, first + s, 1, lst, sq=False, cnt=False)[0] for s in range(count)])      # [count, n, 4]
    listed = np.zeros(n, bool)
    listed[lst] = True
    assert np.array_equal(bits(acc[listed]), bits(butterfly(per_sample)[listed]))
    sq = (per_sample * per_sample).astype(np.float32)
    assert np.array_equal(bits(asq[listed]), bits(butterfly(sq)[listed]))
    assert np.all(asq[~listed] == 0) and np.all(cn[listed] == 7 + count)
    # a count-1 call adds the square itself
    one, one_sq, _ = sparse(raw, p, w, h, first, 1, lst)
    assert np.array_equal(bits(one_sq[listed]), bits((per_sample[0] * per_sample[0]).astype(np.float32)[listed]))
    # without the optional buffers only the sum is added
    only, none_sq, none_cn = sparse(raw, p, w, h, first, count, lst, sq=False, cnt=False)
    assert none_sq is None and none_cn is None and np.array_equal(bits(only), bits(acc))


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------
def test_list_edges(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    w, h, count = 48, 27, 16
    p = api.render_params(w, h, count)
    n = api.num_pixels(p)
    want = dense(raw, p, w, h, 0, count, PREFILL)
    # an empty list: nothing happens (also through the C ABI with a non-null pointer)
    acc, asq, cn = sparse(raw, p, w, h, 0, count, np.zeros(0, np.int32), PREFILL)
    assert np.all(acc == PREFILL) and np.all(asq == PREFILL) and np.all(cn == 7)
    buf = torch.full((4 * n,), PREFILL, dtype=torch.float32, device=DEV)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    import ctypes as C
    rc = api.lib().mirt_render_accumulate_pixels(raw._h, C.byref(p), C.c_void_p(one.data_ptr()), 0, C.c_void_p(buf.data_ptr()), None, None, 0, count, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(buf == PREFILL))
    # one pixel
    acc, asq, cn = sparse(raw, p, w, h, 0, count, [n // 2 + 5], PREFILL)
    k = n // 2 + 5
    assert np.array_equal(bits(acc[k]), bits(want[k])) and cn[k] == 7 + count
    assert np.all(np.delete(acc, k, axis=0) == PREFILL) and np.all(np.delete(cn, k) == 7)
    # no list: the dense call, plus counts for every pixel
    acc, asq, cn = sparse(raw, p, w, h, 0, count, None, PREFILL)
    assert np.array_equal(bits(acc), bits(want)) and np.all(cn == 7 + count) and np.any(asq != PREFILL)
    # a permutation of all pixels
    perm = np.random.default_rng(8).permutation(n).astype(np.int32)
    acc2, asq2, cn2 = sparse(raw, p, w, h, 0, count, perm, PREFILL)
    assert np.array_equal(bits(acc2), bits(want)) and np.array_equal(bits(asq2), bits(asq)) and np.all(cn2 == 7 + count)


def test_an_entry_past_the_end_is_skipped(gpu_scenes):
    """All three buffers are one pixel longer than the part and the extra element holds a sentinel: a missing bound would change
    the sentinel (never read or write outside an allocation)."""
    import ctypes as C
    stl, raw = gpu_scenes("tenthousand")
    w, h, count = 48, 27, 16
    p = api.render_params(w, h, count)
    n = api.num_pixels(p)
    want = dense(raw, p, w, h, 0, count, PREFILL)
    acc = torch.full((4 * (n + 1),), PREFILL, dtype=torch.float32, device=DEV)
    asq = torch.full((4 * (n + 1),), PREFILL, dtype=torch.float32, device=DEV)
    cn = torch.full((n + 1,), 7, dtype=torch.int32, device=DEV)
    lst = torch.as_tensor(np.array([3, n, n - 1, 10], np.int32), device=DEV)
    rc = api.lib().mirt_render_accumulate_pixels(raw._h, C.byref(p), C.c_void_p(lst.data_ptr()), 4, C.c_void_p(acc.data_ptr()), C.c_void_p(asq.data_ptr()),
                                                 C.c_void_p(cn.data_ptr()), 0, count, api._stream_ptr(None))
    assert rc == 0
    torch.cuda.synchronize()
    a, c = acc.cpu().numpy().reshape(n + 1, 4), cn.cpu().numpy()
    assert np.all(a[n] == PREFILL) and np.all(asq.cpu().numpy().reshape(n + 1, 4)[n] == PREFILL) and c[n] == 7
    for k in (3, n - 1, 10):
        assert np.array_equal(bits(a[k]), bits(want[k])) and c[k] == 7 + count
    assert c.sum() == 7 * (n + 1) + 3 * count


def test_errors(gpu_scenes):
    stl = m.parseInput(scene_path("tri"))
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        acc = torch.zeros(4 * 64, dtype=torch.float32, device=DEV)
        lst = torch.zeros(3, dtype=torch.int32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.render_accumulate_pixels(raw, acc, 8, 8, 0, 4, lst)
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        with options(raw, wavefront=1):
            with pytest.raises(m.MirtError) as e:
                m.render_accumulate_pixels(raw, acc, 8, 8, 0, 4, lst)
            assert e.value.status == 3
            m.render_accumulate_pixels(raw, acc, 8, 8, 0, 4, None)      # the dense call works on the wavefront pair
        with pytest.raises(m.MirtError) as e:
            m.render_accumulate_pixels(raw, acc, 8, 8, 4090, 16, lst)      # the 4096 cap
        assert e.value.status == 3
        torch.cuda.synchronize()
    finally:
        raw.close()


# ---- 6. select ---------------------------------------------------------------------------------------------------------------------
def select_restatement(S, Q, n, min_samples, max_samples, max_variance):
    """include/mirt.h, mirt_select_pixels, in numpy float32: one rounding per operation."""
    f = np.float32
    with np.errstate(all="ignore"):
        nf = n.astype(f)[:, None]
        mean = (S[:, :3] / nf).astype(f)
        q = (Q[:, :3] / nf).astype(f)
        v = (q - (mean * mean).astype(f)).astype(f)
        v = np.where(v > 0, v, f(0))
        e = np.fmax.reduce((v / (nf - f(1))).astype(f), axis=1)
        noisy = e > f(max_variance)
    return np.nonzero((n < max_samples) & ((n < min_samples) | noisy))[0]


def run_select(S, Q, n, min_samples, max_samples, max_variance):
    npix = len(n)
    p = api.render_params(npix, 1, 2)
    out = torch.full((npix,), -1, dtype=torch.int32, device=DEV)
    num = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    m.select_pixels(torch.as_tensor(S.reshape(-1), device=DEV), torch.as_tensor(Q.reshape(-1), device=DEV), torch.as_tensor(n.astype(np.int32), device=DEV),
                    npix, 1, min_samples, max_samples, max_variance, out, num, params=p)
    torch.cuda.synchronize()
    k = int(num.item())
    out = out.cpu().numpy()
    assert np.all(out[k:] == -1)
    return out[:k]


@pytest.mark.parametrize("npix", [1, 63, 64, 65, 4097, 1_000_003])
def test_select_equals_its_restatement_on_synthetic_moments(npix):
    """Wave, block and scan boundaries; counts 0, 1, min - 1, min, max - 1, max; NaN and infinite sums."""
    rng = np.random.default_rng(npix)
    mn, mx, maxv = 4, 36, 2e-3
    n = rng.choice(np.array([0, 1, mn - 1, mn, 12, mx - 1, mx]), size=npix).astype(np.int64)
    mean = rng.random((npix, 4), dtype=np.float32)
    spread = (rng.random((npix, 4), dtype=np.float32) * np.float32(0.3)) ** 2
    S = (mean * n[:, None]).astype(np.float32)
    Q = ((mean * mean + spread) * n[:, None]).astype(np.float32)
    bad = rng.random(npix) < 0.05
    S[bad, 0] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(bad.sum()))
    bad = rng.random(npix) < 0.05
    Q[bad, 1] = rng.choice(np.array([np.nan, np.inf], np.float32), size=int(bad.sum()))
    want = select_restatement(S, Q, n, mn, mx, maxv)
    got = run_select(S, Q, n, mn, mx, maxv)
    assert len(got) == len(want) and np.array_equal(got, want)
    assert np.all(np.diff(got) > 0)
    if npix > 64:
        noisy_only = select_restatement(S, Q, np.where(n < mn, mx, n), mn, mx, maxv)
        assert 0 < len(noisy_only) < npix and 0 < len(want) < npix      # the threshold decides something


def test_select_on_the_moments_of_a_real_frame(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    w, h = 96, 54
    p = api.render_params(w, h, 16)
    acc, asq, cn = sparse(raw, p, w, h, 0, 8, None)
    cn = cn - 7
    for maxv in (1e-4, 1e-3, 1e-2):
        want = select_restatement(acc, asq, cn.astype(np.int64), 4, 64, maxv)
        got = run_select(acc, asq, cn, 4, 64, maxv)
        assert np.array_equal(got, want)
    assert 0 < len(select_restatement(acc, asq, cn.astype(np.int64), 4, 64, 1e-3)) < w * h


def test_select_rejects_bad_arguments():
    z = torch.zeros(4 * 8, dtype=torch.float32, device=DEV)
    c = torch.zeros(8, dtype=torch.int32, device=DEV)
    num = torch.zeros(1, dtype=torch.int32, device=DEV)
    for mn, mx in ((1, 8), (4, 3)):
        with pytest.raises(m.MirtError) as e:
            m.select_pixels(z, z, c, 8, 1, mn, mx, 0.1, c.clone(), num)
        assert e.value.status == 3


# ---- 7. finalize_counts ------------------------------------------------------------------------------------------------------------
def test_finalize_counts_is_finalize_with_each_pixels_own_count(gpu_scenes):
    stl, raw = gpu_scenes("redchair")
    w, h = 64, 36
    n = w * h
    acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    m.render_accumulate(acc, w, h, 0, 12, raw)

    def fin(total):
        img = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
        m.finalize(img, acc, w, h, total)
        torch.cuda.synchronize()
        return img.cpu().numpy().reshape(n, 4)

    def fin_counts(counts):
        img = torch.full((4 * n,), 99, dtype=torch.uint8, device=DEV)
        m.finalize_counts(img, acc, torch.as_tensor(counts.astype(np.int32), device=DEV), w, h)
        torch.cuda.synchronize()
        return img.cpu().numpy().reshape(n, 4)

    assert np.array_equal(fin_counts(np.full(n, 12)), fin(12))
    assert np.all(fin_counts(np.zeros(n)) == 0)
    mixed = np.random.default_rng(9).choice(np.array([0, 1, 5, 12, 40]), size=n)
    got = fin_counts(mixed)
    for c in (1, 5, 12, 40):
        assert np.array_equal(got[mixed == c], fin(c)[mixed == c])
    assert np.all(got[mixed == 0] == 0)


# ---- 8. the driver -----------------------------------------------------------------------------------------------------------------
# redchair.txt at 64 x 36: the oracle's samples 0..3 of every pixel (orc_render_accumulate, one sample per call), put through the
# formula of mirt_select_pixels, give an estimated variance of the mean of 0 for 24 % of the pixels (four equal samples), a
# median of 6.7e-4, a 90th percentile of 1.7e-2 and a maximum of 0.14.  At 1e-3 the first round selects 39 % of the frame (893 of
# 2304 pixels) on the oracle's values: neither nothing nor everything.
DRIVER_MAX_VARIANCE = 1e-3


def test_render_adaptive_equals_a_hand_written_loop(gpu_scenes):
    stl, raw = gpu_scenes("redchair")
    w, h, mn, mx, step, maxv = 64, 36, 4, 36, 8, DRIVER_MAX_VARIANCE
    n = w * h
    img, counts, rounds = m.render_adaptive(raw, w, h, mn, mx, step, maxv)
    torch.cuda.synchronize()
    img, counts = img.cpu().numpy(), counts.cpu().numpy()
    assert set(np.unique(counts)) <= {mn + step * k for k in range(5)} and counts.max() <= mx and 1 <= rounds <= 4
    # the loop by hand over the three primitives
    p = api.render_params(w, h, mx)
    acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    asq = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    cn = torch.zeros(n, dtype=torch.int32, device=DEV)
    pix = torch.empty(n, dtype=torch.int32, device=DEV)
    num = torch.zeros(1, dtype=torch.int32, device=DEV)
    m.render_accumulate_pixels(raw, acc, w, h, 0, mn, None, asq, cn, params=p)
    first_round = None
    for r in range(4):
        m.select_pixels(acc, asq, cn, w, h, mn, mx, maxv, pix, num, params=p)
        k = int(num.item())
        if first_round is None:
            first_round = k
        if k == 0:
            break
        m.render_accumulate_pixels(raw, acc, w, h, mn + r * step, step, pix[:k], asq, cn, params=p)
    assert 0 < first_round < n, first_round
    out = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
    m.finalize_counts(out, acc, cn, w, h, params=p)
    torch.cuda.synchronize()
    assert np.array_equal(cn.cpu().numpy(), counts) and np.array_equal(out.cpu().numpy(), img)
    # every pixel that stopped below the cap is quiet by the restatement
    left = select_restatement(acc.cpu().numpy().reshape(n, 4), asq.cpu().numpy().reshape(n, 4), counts.astype(np.int64), mn, mx, maxv)
    assert len(left) == 0
    assert np.any(counts == mn) and np.any(counts > mn)


# ---- 9. dense frames are untouched -------------------------------------------------------------------------------------------------
def test_sparse_calls_leave_dense_frames_as_they_were(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    w, h, spp = 96, 54, 16
    n = w * h
    p = api.render_params(w, h, spp)

    images = [torch.zeros(4 * n, dtype=torch.uint8, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()

    def frame(stream=None):
        img = images.pop()
        m.render(img, w, h, spp, raw, params=p, stream=stream)
        return img

    before = frame()
    torch.cuda.synchronize()
    acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    for k in range(5):
        lst = torch.as_tensor(random_list(n, 0.1 + 0.15 * k, 20 + k), device=DEV)
        m.render_accumulate_pixels(raw, acc, w, h, 0, 16, lst, params=p)
    after = frame()
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    # a dense frame in flight on one stream, a sparse call issued meanwhile on another
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    lst = random_list(n, 0.3, 30)
    alone = sparse(raw, p, w, h, 0, 16, lst, cnt=False)
    pixels = torch.as_tensor(lst, device=DEV)
    acc2 = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    asq2 = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    flying = frame(s1)
    m.render_accumulate_pixels(raw, acc2, w, h, 0, 16, pixels, asq2, params=p, stream=s2)
    flying2 = frame(s1)
    torch.cuda.synchronize()
    assert torch.equal(flying, before) and torch.equal(flying2, before)
    assert np.array_equal(bits(acc2.cpu().numpy().reshape(n, 4)), bits(alone[0])) and np.array_equal(bits(asq2.cpu().numpy().reshape(n, 4)), bits(alone[1]))
    assert raw.stats()["overflow_events"] == 0


# ---- 10. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_adaptive_writes_the_drivers_image(tmp_path, gpu_scenes):
    from PIL import Image
    maxv = 1e-3
    out = tmp_path / "adaptive.png"
    r = subprocess.run([CLI, scene_path("tri"), "--adaptive", str(maxv), "--min-spp", "4", "--spp", "20", "--width", "64", "--height", "64", "--out", str(out)],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    stl, raw = gpu_scenes("tri")
    img, counts, rounds = m.render_adaptive(raw, 64, 64, 4, 20, 4, maxv)
    torch.cuda.synchronize()
    line = re.search(r"Adaptive sampling: (\d+) samples used \(min-spp x pixels: (\d+), spp x pixels: (\d+)\)", r.stdout)
    assert line, r.stdout
    assert [int(g) for g in line.groups()] == [int(counts.sum().item()), 4 * 64 * 64, 20 * 64 * 64]
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")).reshape(-1), img.cpu().numpy())
    r = subprocess.run([CLI, scene_path("tri"), "--adaptive", str(maxv), "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--adaptive" in r.stderr

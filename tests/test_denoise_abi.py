"""Denoising (mirt_hit_features / mirt_denoise / mirt_denoise_work_bytes): the C ABI, the argument checks the host makes before any
device work, the Python plumbing, the command line's usage check, and self-checks of the numpy restatement the GPU tests compare
the kernels with (tests/denoise_ref.py).  No compute calls are made here (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
from conftest import scene_path
import denoise_ref as dr
import oracle_lib as ol
import pyscene
import shade_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_ray_tracer_amd", "_build", "raytracer")
SYMBOLS = ("mirt_hit_features", "mirt_denoise", "mirt_denoise_work_bytes")
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "mirt.h")).read()


def _declared():
    return set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))


def test_header_declares_and_library_exports_the_denoise_entry_points():
    L = m.lib()
    for s in SYMBOLS:
        assert s in _declared(), s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3
    for f in ("hit_features", "denoise", "denoise_work_bytes", "denoise_frame"):
        assert f in m.__all__ and callable(getattr(m, f))
    # the drivers' default scales are the header's
    for name, value in (("C", api.DENOISE_SIGMA_C), ("N", api.DENOISE_SIGMA_N), ("P", api.DENOISE_SIGMA_P)):
        assert float(re.search(r"#define MIRT_DENOISE_SIGMA_%s ([0-9.eE+-]+)f" % name, _header()).group(1)) == value


# fake device addresses: the checks below are host pointer arithmetic, nothing is dereferenced
W, H = 16, 8
N = W * H
BASE = 0x7000_0000_0000
ACC, ASQ, CNT, FEAT, WORK, OUT = (BASE + k * 0x10000 for k in range(6))      # 64 KiB apart: 40 N = 5120 bytes is the largest range


def _denoise(p=None, acc=ACC, asq=ASQ, cnt=CNT, feat=FEAT, iterations=5, sc=4.0, sn=0.1, sp=0.3, work=WORK, out=OUT):
    p = p if p is not None else api.render_params(W, H, 8)
    v = lambda a: C.c_void_p(a) if a else None
    return m.lib().mirt_denoise(C.byref(p) if p != "null" else None, v(acc), v(asq), v(cnt), v(feat), iterations, sc, sn, sp, v(work), v(out), None)


def test_denoise_argument_errors_are_found_on_the_host():
    L = m.lib()
    assert _denoise(p="null") == 3
    assert _denoise(p=api.render_params(W, H, 8, stripe_rows=2, num_parts=2, part=0)) == 3
    assert b"num_parts" in L.mirt_last_error()
    assert _denoise(p=api.render_params(-1, H, 8)) == 3
    for it in (-1, 9, 100):
        assert _denoise(iterations=it) == 3
    assert b"iterations" in L.mirt_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan"), -0.0):
        for key in ("sc", "sn", "sp"):
            assert _denoise(**{key: bad}) == 3, (key, bad)
    assert b"sigma" in L.mirt_last_error()
    for key in ("acc", "asq", "cnt", "feat", "work", "out"):
        assert _denoise(**{key: 0}) == 3, key
    assert b"null" in L.mirt_last_error()
    # misaligned
    assert _denoise(out=OUT + 4) == 3 and _denoise(work=WORK + 8) == 3 and _denoise(feat=FEAT + 4) == 3 and _denoise(cnt=CNT + 2) == 3
    # overlaps: d_out and d_work against every input range (16 N, 16 N, 4 N, 32 N bytes), and against each other
    for inp, size in ((ACC, 16 * N), (ASQ, 16 * N), (CNT, 4 * N), (FEAT, 32 * N)):
        assert _denoise(out=inp) == 3
        assert _denoise(out=inp + size - 16) == 3           # the last 16 bytes of the input
        assert _denoise(out=inp - 16 * N + 16) == 3         # the output's last 16 bytes
        assert _denoise(work=inp + size - 16) == 3
        assert _denoise(work=inp - 40 * N + 16) == 3
    assert b"overlap" in L.mirt_last_error()
    assert _denoise(out=WORK) == 3 and _denoise(out=WORK + 40 * N - 16) == 3 and _denoise(work=OUT + 16 * N - 16) == 3
    # in-place filtering is an overlap too
    assert _denoise(out=ACC) == 3
    assert _denoise(p=api.render_params(0, H, 8)) == 3         # (no such frame: mirt_render_num_pixels refuses it too)
    assert L.mirt_hit_features(None, C.c_void_p(FEAT), C.c_void_p(CNT), 4, C.c_void_p(OUT), None) == 3


def test_work_bytes_is_forty_bytes_per_pixel():
    L = m.lib()
    for w, h in ((1, 1), (16, 8), (1920, 1080), (3840, 2160), (65, 5)):
        p = api.render_params(w, h, 8)
        assert L.mirt_denoise_work_bytes(C.byref(p)) == 40 * w * h == m.denoise_work_bytes(w, h)
    assert L.mirt_denoise_work_bytes(None) == 0
    assert L.mirt_denoise_work_bytes(C.byref(api.render_params(16, 8, 8, stripe_rows=2, num_parts=2, part=1))) == 0
    assert L.mirt_denoise_work_bytes(C.byref(api.render_params(-3, 8, 8))) == 0


def _fake_scene():
    return types.SimpleNamespace(device=0, _h=None)


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    raw = _fake_scene()
    rays, hits, feat = torch.zeros((5, 8)), torch.zeros((5, 6), dtype=torch.int32), torch.zeros((5, 8))
    with pytest.raises(ValueError, match="dtype"):
        m.hit_features(raw, rays.double(), hits, feat)
    with pytest.raises(ValueError, match="shape"):
        m.hit_features(raw, rays, hits[:4], feat)
    with pytest.raises(ValueError, match="shape"):
        m.hit_features(raw, rays, hits, torch.zeros((5, 6)))
    with pytest.raises(ValueError, match="dtype"):
        m.hit_features(raw, rays, hits.to(torch.int64), feat)
    with pytest.raises(ValueError, match="contiguous"):
        m.hit_features(raw, rays, hits, torch.zeros((10, 8))[::2])
    with pytest.raises(ValueError, match="torch tensor"):
        m.hit_features(raw, rays, hits, None)
    with pytest.raises(ValueError, match="cuda"):
        m.hit_features(raw, rays, hits, feat)
    acc, cnt, F = torch.zeros(4 * N), torch.zeros(N, dtype=torch.int32), torch.zeros((N, 8))
    work, out = torch.zeros(10 * N), torch.zeros(4 * N)
    with pytest.raises(ValueError, match="dtype"):
        m.denoise(out.double(), acc, acc, cnt, F, W, H, work)
    with pytest.raises(ValueError, match="shape"):
        m.denoise(out, acc[:-4], acc, cnt, F, W, H, work)
    with pytest.raises(ValueError, match="dtype"):
        m.denoise(out, acc, acc, cnt.float(), F, W, H, work)
    with pytest.raises(ValueError, match="shape"):
        m.denoise(out, acc, acc, cnt, F.reshape(-1), W, H, work)
    with pytest.raises(ValueError, match="shape"):
        m.denoise(out, acc, acc, cnt, F, W, H, work[:-1])
    with pytest.raises(ValueError, match="contiguous"):
        m.denoise(out, acc, torch.zeros(8 * N)[::2], cnt, F, W, H, work)
    with pytest.raises(ValueError, match="iterations"):
        m.denoise(out, acc, acc, cnt, F, W, H, work, iterations=9)
    with pytest.raises(ValueError, match="sigma_n"):
        m.denoise(out, acc, acc, cnt, F, W, H, work, sigma_n=0.0)
    with pytest.raises(ValueError, match="sigma_p"):
        m.denoise(out, acc, acc, cnt, F, W, H, work, sigma_p=float("nan"))
    with pytest.raises(ValueError, match="num_parts"):
        m.denoise(out, acc, acc, cnt, F, W, H, work, params=api.render_params(W, H, 8, stripe_rows=2, num_parts=2, part=0))
    with pytest.raises(ValueError, match="cuda"):
        m.denoise(out, acc, acc, cnt, F, W, H, work)


def test_cli_refuses_denoise_on_several_gpus_before_it_touches_a_device(tmp_path):
    r = subprocess.run([CLI, scene_path("tri"), "--denoise", "5", "--gpus", "2"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--denoise" in r.stderr and "--gpus" in r.stderr
    r = subprocess.run([CLI, scene_path("tri"), "--denoise", "9"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 2 and "--denoise" in r.stderr
    assert not list(tmp_path.iterdir())


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_with_no_iterations_is_the_sample_mean():
    rng = np.random.default_rng(1)
    k = rng.choice(np.array([0, 1, 2, 7, 64]), size=N)
    S = rng.random((N, 4), dtype=f32) * k[:, None].astype(f32)
    Q = rng.random((N, 4), dtype=f32)
    out, stats = dr.denoise(S, Q, k, np.zeros((N, 8), f32), W, H, 0, 4.0, 0.1, 0.3)
    with np.errstate(all="ignore"):
        want = np.where(k[:, None] != 0, S / k[:, None].astype(f32), f32(0)).astype(f32)
    assert dr.same_bits(out, want) and stats == dict(kept=0, skipped=0)
    assert np.all(out[k == 0] == 0)


def test_restatement_keeps_a_flat_frame_of_misses():
    """Zero variance, one colour, no geometry: every weight is h, and sum(h c) / sum(h) must give c back within the rounding of
    25 additions (the colour is chosen so that every partial sum is exact: the result is c itself)."""
    k = np.full(N, 4)
    colour = np.array([0.5, 0.25, 2.0, 1.0], f32)
    S = np.tile(colour * f32(4), (N, 1))
    Q = np.tile(colour * colour * f32(4), (N, 1))
    out, stats = dr.denoise(S, Q, k, np.zeros((N, 8), f32), W, H, 5, 4.0, 0.1, 0.3)
    assert np.array_equal(out, np.tile(colour, (N, 1)))
    assert stats["kept"] > 0 and stats["skipped"] == 0


def _pinhole_rays(sc, w, h):
    """The un-jittered primary rays of a pinhole camera (shade_common.h primary_dir): stand-ins, on the CPU, for sample 0's rays."""
    Y, X = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    md = f32(max(w, h))
    sx, sy = (f32(2) * X - f32(w)) / md, (f32(h) - f32(2) * Y) / md
    fw, rt, up = (np.asarray(v, f32) for v in (sc.forward, sc.right, sc.up))
    rays = np.zeros((h * w, 8), f32)
    rays[:, 0:3] = np.asarray(sc.eye, f32)
    rays[:, 3] = np.inf
    rays[:, 4:7] = ((fw[None, None, :] + sx[..., None] * rt) + sy[..., None] * up).reshape(-1, 3)
    return rays


QUALITY_CASE, QUALITY_W, QUALITY_H, QUALITY_SPP, QUALITY_REF_SPP = "closed_box_b2_g1", 64, 64, 8, 2048


def test_restatement_lowers_the_error_of_a_noisy_gi_frame_on_oracle_samples():
    """The quality condition of tests/test_gpu_denoise.py, on the CPU: the oracle's samples 0..7 of closed_box (gi) at 64 x 64,
    one orc_render_accumulate per sample for the sums and the sums of squares, filtered by the restatement with the default
    scales, against the oracle's 2048-sample mean.  The condition is MSE(denoised) < MSE(noisy) over the pixels finite in all
    three images; no margin can be derived, so none is asked."""
    sc = pyscene.parse_lines(shade_scenes.ALL[QUALITY_CASE].text.split("\n"))
    w, h, n = QUALITY_W, QUALITY_H, QUALITY_W * QUALITY_H
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        ref = np.zeros((h, w, 4), np.float64)
        for first in range(0, QUALITY_REF_SPP, 512):
            part = np.zeros((h, w, 4), f32)
            o.render_accumulate(part, w, h, first, 512, nthreads=8)
            ref += part
        ref = (ref / QUALITY_REF_SPP).reshape(n, 4)
        S, Q = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
        for s in range(QUALITY_SPP):
            one = np.zeros((h, w, 4), f32)
            o.render_accumulate(one, w, h, s, 1, nthreads=8)
            one = one.reshape(n, 4)
            S, Q = S + one, Q + one * one
        aov = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)["aov"]
    finally:
        o.close()
    F = dr.features(_pinhole_rays(sc, w, h), np.ascontiguousarray(aov).reshape(-1).view(np.uint32).reshape(-1, 6))
    assert 0 < np.count_nonzero(F[:, 3]) <= n
    noisy = S / f32(QUALITY_SPP)
    out, stats = dr.denoise(S, Q, np.full(n, QUALITY_SPP), F, w, h, 5, api.DENOISE_SIGMA_C, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)
    ok = np.all(np.isfinite(noisy[:, :3]), axis=1) & np.all(np.isfinite(out[:, :3]), axis=1) & np.all(np.isfinite(ref[:, :3]), axis=1)
    assert ok.mean() > 0.99
    mse_noisy = float(np.mean((noisy[ok, :3].astype(np.float64) - ref[ok, :3]) ** 2))
    mse_out = float(np.mean((out[ok, :3].astype(np.float64) - ref[ok, :3]) ** 2))
    print(f"closed_box 64x64 8 spp: MSE noisy {mse_noisy:.4e}, denoised {mse_out:.4e}, ratio {mse_out / mse_noisy:.3f}")
    assert mse_out < mse_noisy, (mse_out, mse_noisy)
    assert stats["kept"] > 0

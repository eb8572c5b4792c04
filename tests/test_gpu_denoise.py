"""Denoising on the GPU (include/mirt.h: mirt_hit_features, mirt_denoise; api.denoise_frame; `raytracer --denoise`).  The yardstick
is tests/denoise_ref.py, the numpy float32 restatement of the header's text: features and filtered frames are compared with it on
bit patterns (a NaN matching a NaN: the sign and payload of a NaN that an operation produces are not IEEE's to fix).  The quality
test asks only what can be asked without a fitted number: the filtered 8-spp frame is nearer to a 2048-spp frame than the
unfiltered one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import denoise_ref as dr
import shade_scenes
from conftest import scene_path

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cuda_ray_tracer_amd", "_build", "raytracer")
SIGMAS = (api.DENOISE_SIGMA_C, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)
BOX = "closed_box_b2_g1"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def gpu_denoise(S, Q, k, F, w, h, iterations, sigmas=SIGMAS, stream=None, sync=True):
    """mirt_denoise on copies of the inputs: the output [N, 4]; asserts that no input byte changed and that the words next to
    the output and the workspace kept their sentinel."""
    n = w * h
    tS, tQ, tk, tF = dev(S.reshape(-1), f32), dev(Q.reshape(-1), f32), dev(k, np.int32), dev(F.reshape(n, 8), f32)
    out = torch.full((4 * n + 4,), -7.0, dtype=torch.float32, device=DEV)
    work = torch.full((10 * n + 4,), -7.0, dtype=torch.float32, device=DEV)
    if stream is not None:
        torch.cuda.current_stream().synchronize()      # the fills above ran on the current stream
    m.denoise(out[:4 * n], tS, tQ, tk, tF, w, h, work[:10 * n], iterations, *sigmas, stream=stream)
    if not sync:
        return out, (tS, tQ, tk, tF, work)
    torch.cuda.synchronize()
    for t, a in ((tS, S), (tQ, Q), (tF, F)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1))
    assert np.array_equal(tk.cpu().numpy(), np.asarray(k, np.int32))
    assert bool(torch.all(out[4 * n:] == -7.0)) and bool(torch.all(work[10 * n:] == -7.0))
    return out[:4 * n].cpu().numpy().reshape(n, 4)


# ---- 1. features ------------------------------------------------------------------------------------------------------------------
FEATURE_SCENE = """png 33 17 f.png
color 1 1 1
sun 1 1 1
color 0.8 0.3 0.2
plane 0 1 0 1
color 0.2 0.8 0.3
sphere -0.7 0 -2 0.5
xyz 0.2 -0.6 -3
xyz 1.6 -0.6 -3
xyz 0.9 0.8 -2.5
color 0.3 0.3 0.9
tri 1 2 3
"""


def _rays_hits_features(raw, w, h, spp):
    n = w * h
    rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.full((n, 6), -7, dtype=torch.int32, device=DEV)
    feat = torch.full((n + 1, 8), -7.0, dtype=torch.float32, device=DEV)
    m.camera_rays(raw, rays, w, h, spp)
    m.trace_rays(raw, rays, hits)
    m.hit_features(raw, rays, hits, feat[:n])
    torch.cuda.synchronize()
    assert bool(torch.all(feat[n] == -7.0))
    return rays.cpu().numpy(), hits.cpu().numpy().view(np.uint32), feat[:n].cpu().numpy()


@pytest.mark.parametrize("camera,spp", [("", 0), ("", 8), ("fisheye\n", 0)])
def test_features_equal_the_restatement(camera, spp):
    stl = m.parseText(FEATURE_SCENE.replace("color 1 1 1\n", camera + "color 1 1 1\n", 1))
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        m.build_lbvh_karas(raw)
        rays, hits, feat = _rays_hits_features(raw, 33, 17, spp)
    finally:
        raw.close()
    want = dr.features(rays, hits)
    assert np.array_equal(feat.view(np.uint32), want.view(np.uint32))
    kinds = set(hits[:, 1].tolist())
    if camera:
        assert np.any(np.isnan(rays[:, 4:7])) and 0 in kinds and len(kinds) > 1      # the corners of a fisheye frame: NaN directions, misses
        assert np.all(feat[np.isnan(rays[:, 4])] == 0)
    else:
        assert kinds == {0, 1, 2, 3}
    assert np.all(feat[hits[:, 1] == 0] == 0) and np.all(feat[hits[:, 1] != 0, 3] == 1) and np.all(feat[:, 7] == 0)


def test_hit_features_edges_and_errors():
    stl = m.parseText(FEATURE_SCENE)
    raw = m.initRawConfigFromStl(stl, 0)
    try:
        rays = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
        hits = torch.zeros((4, 6), dtype=torch.int32, device=DEV)
        feat = torch.full((4, 8), -7.0, dtype=torch.float32, device=DEV)
        with pytest.raises(m.MirtError) as e:
            m.hit_features(raw, rays, hits, feat)
        assert e.value.status == 6
        m.build_lbvh_karas(raw)
        L = m.lib()
        r, hh, ff = (C.c_void_p(t.data_ptr()) for t in (rays, hits, feat))
        assert L.mirt_hit_features(raw._h, None, hh, 4, ff, None) == 3
        assert L.mirt_hit_features(raw._h, r, None, 4, ff, None) == 3
        assert L.mirt_hit_features(raw._h, r, hh, 4, None, None) == 3
        assert L.mirt_hit_features(raw._h, r, hh, -1, ff, None) == 3
        assert L.mirt_hit_features(raw._h, r, hh, 0, ff, None) == 0
        m.hit_features(raw, rays[:0], hits[:0], feat[:0])
        torch.cuda.synchronize()
        assert bool(torch.all(feat == -7.0))
    finally:
        raw.close()


# ---- 2. the filter on synthetic inputs --------------------------------------------------------------------------------------------
def synthetic(w, h, seed, coincident=False):
    """Moments and features that reach every rule: counts from {0, 1, 2, 7, 64}; 5 % of the pixels with NaN or an infinity in a
    colour sum and 5 % in a square sum; a tilted plane of hit points with a position step through the middle column, the normals
    flipped in a band of rows, a region of misses in one corner and single misses elsewhere."""
    rng = np.random.default_rng(seed)
    n = w * h
    k = rng.choice(np.array([0, 1, 2, 7, 64]), size=n)
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(X / 7.0), 0.5 + 0.4 * np.cos(Y / 5.0), 0.3 + 0.01 * (X + Y), np.ones_like(X, float)], axis=-1).reshape(n, 4)
    mean = (base + rng.normal(0, 0.05, (n, 4))).astype(f32)
    spread = ((rng.random((n, 4), dtype=f32) * f32(0.3)) ** 2).astype(f32)
    S = (mean * k[:, None]).astype(f32)
    Q = ((mean * mean + spread) * k[:, None]).astype(f32)
    bad = rng.random(n) < 0.05
    S[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), size=int(bad.sum()))
    bad = rng.random(n) < 0.05
    Q[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf], f32), size=int(bad.sum()))
    F = np.zeros((h, w, 8), f32)
    F[..., 0] = X * 0.1 + rng.normal(0, 1e-3, (h, w))
    F[..., 1] = Y * 0.1
    F[..., 2] = -3 - 0.02 * X - 1.5 * (X >= w // 2)
    F[..., 3] = 1
    nrm = np.array([0.19611613, 0.0, 0.98058068], f32)
    F[..., 4:7] = nrm
    F[(Y >= h // 3) & (Y < h // 3 + 2), 4:7] = -nrm
    if coincident:
        F[..., 0:3] = F[0, 0, 0:3]                      # every hit point is one point: length(D) == 0 on every tap
    miss = ((X < w // 4) & (Y < h // 4)) | (rng.random((h, w)) < 0.03)
    F[miss] = 0
    return S, Q, k, F.reshape(n, 8)


FRAMES = [(1, 1), (1, 130), (130, 3), (67, 41), (64, 4), (65, 5)]      # tile and wave edges; steps of 16 and 32 larger than the frame


def check_against_restatement(S, Q, k, F, w, h, iterations, sigmas=SIGMAS, vacuous_ok=False):
    want, stats = dr.denoise(S, Q, k, F, w, h, iterations, *sigmas)
    got = gpu_denoise(S, Q, k, F, w, h, iterations, sigmas)
    bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
    assert bad[0].size == 0, [(int(i), int(c), float(got[i, c]), float(want[i, c])) for i, c in zip(bad[0][:5], bad[1][:5])] + [f"{bad[0].size} values differ"]
    if not vacuous_ok:
        assert stats["kept"] > 0 and stats["skipped"] > 0, stats      # the rules decided something
    return got, stats


@pytest.mark.parametrize("iterations", [0, 1, 3, 5, 8])
@pytest.mark.parametrize("w,h", FRAMES)
def test_denoise_equals_the_restatement_on_synthetic_frames(w, h, iterations):
    S, Q, k, F = synthetic(w, h, 100 * w + h)
    # (a frame of one pixel has no tap but the centre's, and no iteration has no tap at all: nothing to count there)
    got, stats = check_against_restatement(S, Q, k, F, w, h, iterations, vacuous_ok=(w * h == 1 or iterations == 0))
    assert np.any(~np.isfinite(got)) or w * h == 1      # the planted non-finite pixels come through as they are


def test_denoise_equals_the_restatement_when_all_hit_points_coincide():
    S, Q, k, F = synthetic(67, 41, 5, coincident=True)
    check_against_restatement(S, Q, k, F, 67, 41, 3)


@pytest.mark.parametrize("sigmas", [(0.5, 0.01, 0.02), (16.0, 2.0, 5.0)])
def test_denoise_equals_the_restatement_under_other_scales(sigmas):
    S, Q, k, F = synthetic(67, 41, 6)
    check_against_restatement(S, Q, k, F, 67, 41, 3, sigmas)


# ---- 3. a real frame ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    stl = m.parseText(shade_scenes.ALL[BOX].text)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    yield raw
    raw.close()


def moments(raw, w, h, spp):
    n = w * h
    acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    asq = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    m.render_accumulate_pixels(raw, acc, w, h, 0, spp, None, asq, cnt)
    torch.cuda.synchronize()
    return acc, asq, cnt


def test_denoise_equals_the_restatement_on_a_rendered_frame(box):
    w = h = 48
    acc, asq, cnt = moments(box, w, h, 8)
    rays, hits, feat = _rays_hits_features(box, w, h, 8)
    assert np.array_equal(feat.view(np.uint32), dr.features(rays, hits).view(np.uint32))
    S, Q, k = acc.cpu().numpy().reshape(-1, 4), asq.cpu().numpy().reshape(-1, 4), cnt.cpu().numpy()
    assert np.all(k == 8)
    got, stats = check_against_restatement(S, Q, k, feat, w, h, 5, vacuous_ok=True)
    assert stats["kept"] > 0
    assert not np.array_equal(got, (S / f32(8)).astype(f32))      # the filter changed the frame


# ---- 4. quality ---------------------------------------------------------------------------------------------------------------------
def test_the_denoised_frame_is_nearer_to_a_converged_one(box):
    """closed_box (gi) at 64 x 64: the 8-spp mean and its filtered image (5 iterations, default scales) against the float image of
    mirt_render at 2048 spp.  Asked: MSE(denoised) < MSE(noisy) over r, g, b of the pixels finite in all three.  No margin: none
    can be derived.  (The restatement meets the condition on the oracle's samples: tests/test_denoise_abi.py.)"""
    w = h = 64
    n = w * h
    acc, asq, cnt = moments(box, w, h, 8)
    img, out = m.denoise_frame(box, acc, asq, cnt, w, h, 8)
    ref = torch.empty(4 * n, dtype=torch.float32, device=DEV)
    ref8 = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
    m.render(ref8, w, h, 2048, box, d_float=ref)
    torch.cuda.synchronize()
    assert box.stats()["overflow_events"] == 0
    noisy = acc.cpu().numpy().reshape(n, 4).astype(np.float64) / 8
    den, ref = out.cpu().numpy().reshape(n, 4).astype(np.float64), ref.cpu().numpy().reshape(n, 4).astype(np.float64)
    ok = np.all(np.isfinite(noisy[:, :3]), axis=1) & np.all(np.isfinite(den[:, :3]), axis=1) & np.all(np.isfinite(ref[:, :3]), axis=1)
    assert ok.mean() > 0.99
    mse_noisy = float(np.mean((noisy[ok, :3] - ref[ok, :3]) ** 2))
    mse_den = float(np.mean((den[ok, :3] - ref[ok, :3]) ** 2))
    print(f"closed_box 64x64 8 spp: MSE noisy {mse_noisy:.4e}, denoised {mse_den:.4e}, ratio {mse_den / mse_noisy:.3f}")
    assert mse_den < mse_noisy, (mse_den, mse_noisy)


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------
def test_denoise_on_another_stream_leaves_a_render_in_flight_unchanged(gpu_scenes):
    stl, raw = gpu_scenes("tenthousand")
    w, h, spp = 320, 180, 16
    p = api.render_params(w, h, spp, counters=True)
    n = api.num_pixels(p)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keys = ("samples", "rays", "shadow_rays", "internal_visits", "sphere_tests", "tri_tests", "mat_fetches", "max_stack", "rays_traversed", "overflow_events")
    S, Q, k, F = synthetic(130, 67, 9)
    alone = gpu_denoise(S, Q, k, F, 130, 67, 5)

    def frame(denoise):
        img = torch.zeros(n * 4, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        m.render(img, w, h, spp, raw, params=p, stream=s1)
        outs = [gpu_denoise(S, Q, k, F, 130, 67, 5, stream=s2, sync=False) for _ in range(4)] if denoise else []
        torch.cuda.synchronize()
        st = raw.stats()
        return img.cpu().numpy(), {key: st[key] for key in keys}, [o[0][:4 * 130 * 67].cpu().numpy().reshape(-1, 4) for o in outs]

    img0, st0, _ = frame(False)
    img1, st1, outs = frame(True)
    img2, st2, _ = frame(False)
    assert np.array_equal(img0, img1) and np.array_equal(img0, img2)
    assert st0 == st1 == st2 and st0["samples"] == n * spp
    for o in outs:
        assert dr.same_bits(o, alone)


def test_two_calls_with_their_own_workspace_on_two_streams_equal_the_serial_results():
    a = synthetic(130, 67, 10)
    b = synthetic(130, 67, 11)
    serial = [gpu_denoise(*x, 130, 67, 5) for x in (a, b)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    pending = []
    for _ in range(3):
        pending.append((0, gpu_denoise(*a, 130, 67, 5, stream=s1, sync=False)))
        pending.append((1, gpu_denoise(*b, 130, 67, 5, stream=s2, sync=False)))
    torch.cuda.synchronize()
    for which, (out, keep) in pending:
        assert dr.same_bits(out[:4 * 130 * 67].cpu().numpy().reshape(-1, 4), serial[which])
    assert not dr.same_bits(serial[0], serial[1])


# ---- 6. the driver and the command line ---------------------------------------------------------------------------------------------
def test_denoise_frame_equals_the_hand_written_sequence(box):
    w, h, spp = 48, 40, 8
    n = w * h
    acc, asq, cnt = moments(box, w, h, spp)
    img, out = m.denoise_frame(box, acc, asq, cnt, w, h, spp, iterations=4)
    torch.cuda.synchronize()
    p = api.render_params(w, h, spp)
    rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    feat = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    work = torch.empty(m.denoise_work_bytes(w, h) // 4, dtype=torch.float32, device=DEV)
    mean = torch.empty(4 * n, dtype=torch.float32, device=DEV)
    img2 = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
    m.camera_rays(raw=box, d_rays=rays, img_width=w, img_height=h, aa=spp, params=p)
    m.trace_rays(box, rays, hits)
    m.hit_features(box, rays, hits, feat)
    m.denoise(mean, acc, asq, cnt, feat, w, h, work, 4, *SIGMAS, params=p)
    m.finalize(img2, mean, w, h, 1, params=p)
    torch.cuda.synchronize()
    assert torch.equal(img, img2) and dr.same_bits(out.cpu().numpy(), mean.cpu().numpy())
    assert img.dtype == torch.uint8 and img.numel() == 4 * n and int(img.view(n, 4)[:, 3].max()) == 255


@pytest.mark.parametrize("adaptive", [False, True])
def test_cli_denoise_writes_the_drivers_image(tmp_path, gpu_scenes, adaptive):
    from PIL import Image
    w = h = 64
    out = tmp_path / "denoised.png"
    extra = ["--adaptive", "0.001", "--min-spp", "4"] if adaptive else []
    r = subprocess.run([CLI, scene_path("redchair"), "--denoise", "5", "--spp", "12", "--width", str(w), "--height", str(h), "--out", str(out)] + extra,
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Denoise: 5 iterations" in r.stdout and ("Adaptive sampling:" in r.stdout) == adaptive
    stl, raw = gpu_scenes("redchair")
    n = w * h
    if adaptive:
        # render_adaptive's loop, keeping the moments (min 4, max 12, step 4)
        acc = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
        asq = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
        cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
        pix = torch.empty(n, dtype=torch.int32, device=DEV)
        num = torch.zeros(1, dtype=torch.int32, device=DEV)
        p = api.render_params(w, h, 12)
        m.render_accumulate_pixels(raw, acc, w, h, 0, 4, None, asq, cnt, params=p)
        for rnd in range(2):
            m.select_pixels(acc, asq, cnt, w, h, 4, 12, 0.001, pix, num, params=p)
            kk = int(num.item())
            if kk == 0:
                break
            m.render_accumulate_pixels(raw, acc, w, h, 4 + 4 * rnd, 4, pix[:kk], asq, cnt, params=p)
        assert 4 <= int(cnt.min()) and int(cnt.max()) <= 12
    else:
        acc, asq, cnt = moments(raw, w, h, 12)
    img, _ = m.denoise_frame(raw, acc, asq, cnt, w, h, 12)
    torch.cuda.synchronize()
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")).reshape(-1), img.cpu().numpy())

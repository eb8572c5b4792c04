"""Temporal accumulation (mirt_scene_get_spheres / mirt_scene_get_triangles / mirt_prev_features / mirt_temporal_accumulate): the C
ABI, the argument checks the host makes before any device work, the Python plumbing, and self-checks of the numpy restatement the
GPU tests compare the kernels with (tests/temporal_ref.py).  No compute calls are made here (no GPU needed)."""
import copy
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

import cuda_ray_tracer_amd as m
from cuda_ray_tracer_amd import api
import denoise_ref as dr
import oracle_lib as ol
import pyscene
import shade_scenes
import temporal_ref as tr
from test_denoise_abi import _pinhole_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mirt_scene_get_spheres", "mirt_scene_get_triangles", "mirt_prev_features", "mirt_temporal_accumulate")
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "mirt.h")).read()


def _declared():
    return set(re.findall(r"\b(mirt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))


def test_header_declares_and_library_exports_the_temporal_entry_points():
    L = m.lib()
    for s in SYMBOLS:
        assert s in _declared(), s
        assert s in api.EXPORTS, s
        assert hasattr(L, s), s
    assert L.mirt_version() == 3
    assert re.search(r"#define MIRT_VERSION 3\b", _header())
    for f in ("get_spheres", "get_triangles", "prev_features", "temporal_accumulate", "TemporalAccumulator"):
        assert f in m.__all__ and callable(getattr(m, f))
    # the fifth symbol of the feature is the driver class; its default scales are the denoiser's, no new constant
    import inspect
    sig = inspect.signature(m.TemporalAccumulator.__init__).parameters
    assert sig["max_history"].default == 32 and sig["sigma_n"].default == api.DENOISE_SIGMA_N and sig["sigma_p"].default == api.DENOISE_SIGMA_P
    sig = inspect.signature(m.temporal_accumulate).parameters
    assert sig["sigma_n"].default == api.DENOISE_SIGMA_N and sig["sigma_p"].default == api.DENOISE_SIGMA_P


# Fake device addresses: the checks below are host pointer arithmetic, nothing is dereferenced -- and nothing may be launched on
# them.  So every call here must END in an error: the frame is one no launch can cover (more rows than the grid has tiles), which
# the library finds last, after every pointer check.  "frame too large" therefore means: all the checks before it passed.
W, H = 1, 65535 * 4 + 4
N = W * H
BASE = 0x7000_0000_0000
NAMES = ("acc", "asq", "cnt", "G", "hacc", "hasq", "hcnt", "hF", "oacc", "oasq", "ocnt")
ADDR = {name: BASE + k * 0x1000000 for k, name in enumerate(NAMES)}      # 16 MiB apart: 32 N = 8 MiB is the largest range
SIZE = dict(acc=16 * N, asq=16 * N, cnt=4 * N, G=32 * N, hacc=16 * N, hasq=16 * N, hcnt=4 * N, hF=32 * N, oacc=16 * N, oasq=16 * N, ocnt=4 * N)
OWN = dict(oacc="acc", oasq="asq", ocnt="cnt")


def pinhole(**fields):
    cam = api.Camera()
    cam.eye, cam.forward, cam.right, cam.up = api.Vec3(0, 0, 0), api.Vec3(0, 0, -1), api.Vec3(1, 0, 0), api.Vec3(0, 1, 0)
    return api._camera_with(cam, fields)


def _ta(p=None, cam=None, max_history=32, sn=0.03, sp=0.1, **addr):
    """(status, message) of mirt_temporal_accumulate on the fake addresses; never MIRT_OK."""
    p = p if p is not None else api.render_params(W, H, 8)
    cam = cam if cam is not None else pinhole()
    a = dict(ADDR)
    a.update(addr)
    v = lambda x: C.c_void_p(x) if x else None
    rc = m.lib().mirt_temporal_accumulate(C.byref(p) if p != "null" else None, C.byref(cam) if cam != "null" else None, v(a["acc"]), v(a["asq"]),
                                          v(a["cnt"]), v(a["G"]), v(a["hacc"]), v(a["hasq"]), v(a["hcnt"]), v(a["hF"]), max_history, sn, sp,
                                          v(a["oacc"]), v(a["oasq"]), v(a["ocnt"]), None)
    assert rc == 3, rc
    return m.lib().mirt_last_error().decode()


def passes(**kw):
    return "frame too large" in _ta(**kw)


def test_temporal_accumulate_argument_errors_are_found_on_the_host():
    assert passes()
    assert "null" in _ta(p="null") and "null" in _ta(cam="null")
    for name in NAMES:
        assert "null pointer" in _ta(**{name: 0}), name
    for name in NAMES:
        assert "aligned" in _ta(**{name: ADDR[name] + 2}), name      # misaligned for a float buffer and for the counts
    for name in ("acc", "asq", "G", "hacc", "hasq", "hF", "oacc", "oasq"):
        assert "aligned" in _ta(**{name: ADDR[name] + 4}), name
        assert "aligned" in _ta(**{name: ADDR[name] + 8}), name
    assert "num_parts" in _ta(p=api.render_params(W, H, 8, stripe_rows=2, num_parts=2, part=0))
    assert "bad render parameters" in _ta(p=api.render_params(-1, H, 8)) and "bad render parameters" in _ta(p=api.render_params(0, H, 8))
    for cam in (pinhole(fisheye=1), pinhole(panorama=1), pinhole(dof_focus=2.0), pinhole(dof_focus=float("nan")), pinhole(fisheye=1, panorama=1)):
        assert "pinhole" in _ta(cam=cam)
    assert passes(cam=pinhole(dof_lens=0.5))                    # (a lens radius without a focus distance is not depth of field: shade_common.h)
    for bad in (0, -1, -2 ** 31):
        assert "max_history" in _ta(max_history=bad)
    assert passes(max_history=1) and passes(max_history=2 ** 31 - 1)
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan"), -0.0):
        for key in ("sn", "sp"):
            assert "sigma" in _ta(**{key: bad}), (key, bad)


def test_temporal_accumulate_refuses_every_forbidden_overlap_and_allows_in_place():
    # in place: each output exactly its own current-frame buffer, one at a time and all three
    for out, own in OWN.items():
        assert passes(**{out: ADDR[own]}), out
    assert passes(oacc=ADDR["acc"], oasq=ADDR["asq"], ocnt=ADDR["cnt"])
    for out, own in OWN.items():
        size = SIZE[out]
        step = 16 if size == 16 * N else 4
        # its own current-frame buffer, but shifted
        assert "overlap" in _ta(**{out: ADDR[own] + step}) and "overlap" in _ta(**{out: ADDR[own] - step}), out
        # any other input: at its start, over its last bytes, and with the output's last bytes over its first
        for inp in ("acc", "asq", "cnt", "G", "hacc", "hasq", "hcnt", "hF"):
            if inp == own:
                continue
            assert "overlap" in _ta(**{out: ADDR[inp]}), (out, inp)
            assert "overlap" in _ta(**{out: ADDR[inp] + SIZE[inp] - 16}), (out, inp)
            assert "overlap" in _ta(**{out: ADDR[inp] - size + 16}), (out, inp)
        # the other outputs
        for other in OWN:
            if other == out:
                continue
            assert "overlap" in _ta(**{out: ADDR[other]}), (out, other)
            assert "overlap" in _ta(**{out: ADDR[other] + SIZE[other] - 16}), (out, other)
            assert "overlap" in _ta(**{out: ADDR[other] - size + 16}), (out, other)
    # in place on two buffers does not excuse the third
    assert "overlap" in _ta(oacc=ADDR["acc"], oasq=ADDR["asq"], ocnt=ADDR["hcnt"])
    # a history buffer is never an output, in place or not
    assert "overlap" in _ta(oacc=ADDR["hacc"], oasq=ADDR["hasq"], ocnt=ADDR["hcnt"])
    # adjacent ranges do not overlap
    assert passes(oacc=ADDR["hacc"] + 16 * N) and passes(ocnt=ADDR["hF"] - 4 * N)


def test_get_and_prev_features_argument_errors_need_no_device():
    L = m.lib()
    out = C.c_void_p(BASE)
    assert L.mirt_scene_get_spheres(None, 0, 1, out, None) == 3
    assert L.mirt_scene_get_triangles(None, 0, 1, out, None) == 3
    assert L.mirt_prev_features(None, out, out, 1, None, None, out, None) == 3
    assert b"null scene" in L.mirt_last_error()


def _fake_scene(cam=None, ns=2, nt=1):
    return types.SimpleNamespace(device=0, _h=None, desc=types.SimpleNamespace(num_spheres=ns, num_triangles=nt), camera=lambda: cam)


def test_wrappers_check_their_tensors_before_calling_the_library():
    import torch
    W, H = 16, 8
    N = W * H
    raw = _fake_scene()
    with pytest.raises(ValueError, match="shape"):
        m.get_spheres(raw, torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="dtype"):
        m.get_spheres(raw, torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="cuda"):
        m.get_spheres(raw, torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="shape"):
        m.get_triangles(raw, torch.zeros((1, 12)))
    with pytest.raises(ValueError, match="contiguous"):
        m.get_triangles(raw, torch.zeros((4, 9))[::2])
    with pytest.raises(ValueError, match="cuda"):
        m.get_triangles(raw, torch.zeros((1, 9)))
    rays, hits, feat = torch.zeros((5, 8)), torch.zeros((5, 6), dtype=torch.int32), torch.zeros((5, 8))
    with pytest.raises(ValueError, match="shape"):
        m.prev_features(raw, rays, hits[:4], feat)
    with pytest.raises(ValueError, match="shape"):
        m.prev_features(raw, rays, hits, feat, d_prev_xyzr=torch.zeros((3, 4)))      # the whole array: num_spheres rows
    with pytest.raises(ValueError, match="shape"):
        m.prev_features(raw, rays, hits, feat, d_prev_verts=torch.zeros((1, 3, 3)))
    with pytest.raises(ValueError, match="dtype"):
        m.prev_features(raw, rays, hits, feat, d_prev_xyzr=torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="cuda"):
        m.prev_features(raw, rays, hits, feat, torch.zeros((2, 4)), torch.zeros((1, 9)))
    acc, cnt, F = torch.zeros(4 * N), torch.zeros(N, dtype=torch.int32), torch.zeros((N, 8))
    good = dict(d_out_accum=acc.clone(), d_out_accum_sq=acc.clone(), d_out_counts=cnt.clone(), d_accum=acc, d_accum_sq=acc.clone(), d_counts=cnt,
                d_prev_features=F, d_hist_accum=acc.clone(), d_hist_accum_sq=acc.clone(), d_hist_counts=cnt.clone(), d_hist_features=F.clone(),
                prev_camera=pinhole(), img_width=W, img_height=H)
    call = lambda **kw: m.temporal_accumulate(**{**good, **kw})
    for name in ("d_out_accum", "d_accum_sq", "d_hist_accum"):
        with pytest.raises(ValueError, match="dtype"):
            call(**{name: acc.double()})
        with pytest.raises(ValueError, match="shape"):
            call(**{name: acc[:-4]})
    for name in ("d_out_counts", "d_counts", "d_hist_counts"):
        with pytest.raises(ValueError, match="dtype"):
            call(**{name: cnt.float()})
    for name in ("d_prev_features", "d_hist_features"):
        with pytest.raises(ValueError, match="shape"):
            call(**{name: F.reshape(-1)})
    with pytest.raises(ValueError, match="contiguous"):
        call(d_accum=torch.zeros(8 * N)[::2])
    with pytest.raises(ValueError, match="pinhole"):
        call(prev_camera=pinhole(fisheye=1))
    with pytest.raises(ValueError, match="Camera"):
        call(prev_camera=None)
    with pytest.raises(ValueError, match="max_history"):
        call(max_history=0)
    with pytest.raises(ValueError, match="sigma_n"):
        call(sigma_n=0.0)
    with pytest.raises(ValueError, match="sigma_p"):
        call(sigma_p=float("inf"))
    with pytest.raises(ValueError, match="num_parts"):
        call(params=api.render_params(W, H, 8, stripe_rows=2, num_parts=2, part=0))
    with pytest.raises(ValueError, match="cuda"):
        call()


@pytest.mark.parametrize("fields", [dict(fisheye=1), dict(panorama=1), dict(dof_focus=3.0)])
def test_the_driver_refuses_a_camera_that_is_not_a_pinhole(fields):
    with pytest.raises(ValueError, match="pinhole"):
        m.TemporalAccumulator(_fake_scene(pinhole(**fields)), 33, 17, 8)
    with pytest.raises(ValueError, match="spp"):
        m.TemporalAccumulator(_fake_scene(pinhole()), 33, 17, 0)
    with pytest.raises(ValueError, match="max_history"):
        m.TemporalAccumulator(_fake_scene(pinhole()), 33, 17, 8, max_history=0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
FW, FH = 33, 17
CAMERA = ((0.25, -0.5, 1.0), (0, 0, -1), (1, 0, 0), (0, 1, 0))


def wall(w, h, camera=CAMERA, depth=4.0):
    """Features of a wall `depth` in front of an axis-aligned pinhole, facing it: the hit points of the pixel centres."""
    eye = np.asarray(camera[0], f32)
    Y, X = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    md = f32(max(w, h))
    sx, sy = (f32(2) * X - f32(w)) / md, (f32(h) - f32(2) * Y) / md
    F = np.zeros((h, w, 8), f32)
    F[..., 0], F[..., 1], F[..., 2] = eye[0] + f32(depth) * sx, eye[1] + f32(depth) * sy, eye[2] - f32(depth)
    F[..., 3] = 1
    F[..., 6] = 1
    return F.reshape(-1, 8)


def moments(n, seed, counts):
    rng = np.random.default_rng(seed)
    k = rng.choice(np.asarray(counts), size=n).astype(np.uint32)
    mean = rng.random((n, 4), dtype=f32)
    S = (mean * k[:, None].astype(f32)).astype(f32)
    Q = (mean * mean * k[:, None].astype(f32) + rng.random((n, 4), dtype=f32)).astype(f32)
    return S, Q, k


def run(S, Q, k, G, hS, hQ, hk, hF, max_history=32, camera=CAMERA, w=FW, h=FH):
    return tr.temporal_accumulate(S, Q, k, G, hS, hQ, hk, hF, camera, w, h, max_history, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)


def test_restatement_identity_adds_the_history_bit_for_bit():
    n = FW * FH
    F = wall(FW, FH)
    S, Q, k = moments(n, 1, [8])
    hS, hQ, hk = moments(n, 2, [1, 8, 31, 32])
    oS, oQ, ok, stats = run(S, Q, k, F, hS, hQ, hk, F)
    assert np.array_equal(oS.view(np.uint32), (S + hS).view(np.uint32)) and np.array_equal(oQ.view(np.uint32), (Q + hQ).view(np.uint32))
    assert np.array_equal(ok, k + hk)
    assert stats == dict(valid=n, rejected=0, merged=n, exact=n, capped=0, outside=[0, 0, 0, 0])


def test_restatement_rejects_a_history_that_faces_the_other_way():
    n = FW * FH
    F = wall(FW, FH)
    back = F.copy()
    back[:, 4:7] = -back[:, 4:7]
    S, Q, k = moments(n, 3, [8])
    hS, hQ, hk = moments(n, 4, [8, 16])
    oS, oQ, ok, stats = run(S, Q, k, F, hS, hQ, hk, back)
    assert np.array_equal(oS.view(np.uint32), S.view(np.uint32)) and np.array_equal(oQ.view(np.uint32), Q.view(np.uint32)) and np.array_equal(ok, k)
    assert stats["valid"] == 0 and stats["rejected"] == n and stats["merged"] == 0
    # and a history a depth step behind the surface: the plane term alone
    far = wall(FW, FH, depth=4.5)
    far[:, 0:2] = F[:, 0:2]
    oS, oQ, ok, stats = run(S, Q, k, F, hS, hQ, hk, far)
    assert np.array_equal(oS.view(np.uint32), S.view(np.uint32)) and np.array_equal(ok, k) and stats["rejected"] == n


def test_restatement_caps_the_history_as_stated():
    n = FW * FH
    F = wall(FW, FH)
    S, Q, k = moments(n, 5, [8])
    hS, hQ, hk = moments(n, 6, [4, 32, 33, 100, 4096])
    for cap in (1, 32):
        oS, oQ, ok, stats = run(S, Q, k, F, hS, hQ, hk, F, max_history=cap)
        over = hk > cap
        c = (f32(cap) / hk.astype(f32))[:, None]
        want_S = np.where(over[:, None], S + hS * c, S + hS)
        want_Q = np.where(over[:, None], Q + hQ * c, Q + hQ)
        assert np.array_equal(oS.view(np.uint32), want_S.view(np.uint32)) and np.array_equal(oQ.view(np.uint32), want_Q.view(np.uint32))
        assert np.array_equal(ok, k + np.minimum(hk, cap)) and stats["capped"] == int(over.sum()) > 0
        assert int(ok.max()) == 8 + cap


def test_restatement_gives_a_miss_no_history():
    n = FW * FH
    F = wall(FW, FH)
    G = F.copy()
    miss = np.zeros(n, bool)
    miss[::5] = True
    G[miss] = 0
    hit_hist = F.copy()
    hist_miss = np.zeros(n, bool)
    hist_miss[1::5] = True
    hit_hist[hist_miss] = 0
    S, Q, k = moments(n, 7, [8])
    hS, hQ, hk = moments(n, 8, [8])
    hk[2::10] = 0                                     # a history pixel without samples is no history either
    hS[7::10, 1] = np.inf                             # nor one that is not finite
    hQ[3::20, 2] = np.nan
    oS, oQ, ok, stats = run(S, Q, k, G, hS, hQ, hk, hit_hist)
    none = miss | hist_miss | (hk == 0) | ~np.all(np.isfinite(hS[:, :3]), axis=1) | ~np.all(np.isfinite(hQ[:, :3]), axis=1)
    assert 0 < none.sum() < n
    assert np.array_equal(oS[none].view(np.uint32), S[none].view(np.uint32)) and np.array_equal(ok[none], k[none])
    assert np.array_equal(oS[~none].view(np.uint32), (S + hS)[~none].view(np.uint32)) and np.array_equal(ok[~none], (k + hk)[~none])
    assert stats["merged"] == int((~none).sum())


def test_restatement_blends_four_taps_of_a_shifted_camera():
    """The camera moved a third of a pixel to the right and a quarter of one down: every pixel's history is four taps, the
    weights renormalised, the smallest count; a constant history comes back as that constant (times the count) within rounding."""
    n = FW * FH
    px = f32(4.0) * f32(2) / f32(FW)                 # a pixel's width on the wall
    prev_cam = ((CAMERA[0][0] - float(px) / 3, CAMERA[0][1] + float(px) / 4, CAMERA[0][2]),) + CAMERA[1:]
    G = wall(FW, FH)                                 # this frame's points (nothing moved but the camera)
    hF = wall(FW, FH, camera=prev_cam)
    S, Q, k = moments(n, 9, [8])
    colour = np.array([0.5, 0.25, 0.75, 1.0], f32)
    hk = np.random.default_rng(10).choice(np.array([8, 16], np.uint32), size=n)
    hS = colour[None, :] * hk[:, None].astype(f32)
    hQ = (colour * colour)[None, :] * hk[:, None].astype(f32)
    oS, oQ, ok, stats = run(S, Q, k, G, hS, hQ, hk, hF, camera=prev_cam)
    assert stats["exact"] == 0 and stats["rejected"] == 0 and stats["merged"] == n and stats["valid"] > 3 * n
    kh = ok - k
    assert set(kh.tolist()) <= {8, 16} and np.any(kh == 8)
    # the smallest of the four taps' counts: the taps are (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
    grid = hk.reshape(FH, FW)
    want = np.minimum(np.minimum(grid[:-1, :-1], grid[:-1, 1:]), np.minimum(grid[1:, :-1], grid[1:, 1:]))
    assert np.array_equal(kh.reshape(FH, FW)[:-1, :-1], want)
    got = (oS - S) / kh[:, None].astype(f32)
    assert np.max(np.abs(got - colour[None, :])) < 1e-5


# ---- the two conditions the GPU tests ask of rendered frames, for the restatement alone -------------------------------------------------
# A sphere of radius 1 on a floor, seen from 88 units away through a long lens (|forward| = 32: its silhouette is 6 pixels in radius
# on a 33 x 17 frame and its depth varies by 1 % of the distance, so a sideways move shifts its whole image by nearly one amount).
MOVING_SPHERE = """png 33 17 s.png
forward 0 -8.2822 -30.9096
color 1 1 1
sun 1 1 1
color 0.8 0.3 0.2
plane 0 1 0 23.776
color 0.2 0.8 0.3
sphere %r -22.776 -85.0015 1
"""
# The sphere's x before and after: 1.25 units = 7.5 pixels (6 pixels per unit at that distance).  Chosen with the oracle's primary hits
# (the test below): whole-pixel moves of 5 to 9 pixels meet both conditions too; 7.5 is kept because it lands between pixel
# centres, where the history is a blend of taps.
MOVING_SPHERE_X = (-0.6, 0.65)


def core_of(mask, w, h):
    """The pixels of `mask` ([h * w] bool) whose whole 3 x 3 neighbourhood is in it (none at the frame's border)."""
    padded = np.pad(np.asarray(mask, bool).reshape(h, w), 1)
    out = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out &= padded[dy:dy + h, dx:dx + w]
    return out.reshape(-1)


def _oracle_primary(text, w, h):
    """(scene, un-jittered pinhole rays [n, 8], the oracle's primary hit records [n, 6] as 4-byte words)."""
    sc = pyscene.parse_lines(text.split("\n"))
    o = ol.OracleScene(sc, bounds_mode=0)
    try:
        aov = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=4, want_aov=True)["aov"]
    finally:
        o.close()
    return sc, _pinhole_rays(sc, w, h), np.ascontiguousarray(aov).reshape(-1).view(np.uint32).reshape(-1, 6)


def test_restatement_follows_the_moving_sphere_and_restarts_the_disoccluded_floor():
    w, h, spp = 33, 17, 2
    n = w * h
    sc0, rays0, hits0 = _oracle_primary(MOVING_SPHERE % MOVING_SPHERE_X[0], w, h)
    sc1, rays1, hits1 = _oracle_primary(MOVING_SPHERE % MOVING_SPHERE_X[1], w, h)
    sphere = lambda x: np.array([[x, -22.776, -85.0015, 1]], f32)
    G = tr.prev_features(rays1, hits1, sphere(MOVING_SPHERE_X[1]), np.zeros((0, 9), f32), sphere(MOVING_SPHERE_X[0]), None)
    zero, k = np.zeros((n, 4), f32), np.full(n, spp, np.uint32)      # the two conditions are about counts: any finite moments serve
    _, _, out_k, stats = tr.temporal_accumulate(zero, zero, k, G, zero, zero, k, dr.features(rays0, hits0), (sc0.eye, sc0.forward, sc0.right, sc0.up),
                                                w, h, 32, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)
    kind0, kind1 = hits0[:, 1], hits1[:, 1]
    assert set(kind0.tolist()) == {1, 3} and set(kind1.tolist()) == {1, 3}
    vacated, arrived = core_of((kind0 == 1) & (kind1 == 3), w, h), core_of(kind1 == 1, w, h)
    still = core_of((kind0 == 3) & (kind1 == 3), w, h)
    print(f"moving sphere: {int((kind1 == 1).sum())} sphere pixels, vacated core {int(vacated.sum())}, arrived core {int(arrived.sum())}, {stats}")
    assert vacated.sum() >= 9 and arrived.sum() >= 9
    assert np.all(out_k[vacated] == spp) and np.all(out_k[arrived] > spp) and np.all(out_k[still] == 2 * spp)
    assert 0 < stats["exact"] < stats["merged"]      # the floor's history is single taps, the sphere's a blend


QUALITY = dict(case="closed_box_b2_g1", w=64, h=64, spp=8, frames=4, step_degrees=1.0, ref_spp=2048, centre=(0.0, 0.0, -0.6))


def orbit_fields(eye, forward, right, up, degrees, centre=QUALITY["centre"]):
    """Camera fields turned about the vertical axis through `centre` (tools/anim_bench.py's orbit)."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    rot = lambda v: (c * float(v[0]) + s * float(v[2]), float(v[1]), -s * float(v[0]) + c * float(v[2]))
    rel = rot([float(eye[i]) - centre[i] for i in range(3)])
    return dict(eye=tuple(rel[i] + centre[i] for i in range(3)), forward=rot(forward), right=rot(right), up=rot(up))


def test_restatement_merging_four_frames_lowers_the_error_on_oracle_samples():
    """The quality conditions of tests/test_gpu_temporal.py, on the CPU: the oracle's samples 8 f .. 8 f + 7 of closed_box (gi) at
    64 x 64 for frames f = 0 .. 3, the camera orbiting by 1 degree per frame, merged by the restatement (default scales, max_history
    32; un-jittered pinhole rays and the oracle's primary hits for the features), against the oracle's 2048-sample mean from the
    last camera.  Asked, over r, g, b of the pixels finite in all images, with no margin (none can be derived):
        MSE(merged mean) < MSE(the last frame's own 8 samples);  MSE(merged, 5 denoise iterations) < MSE(last frame, 5 iterations).
    Both hold at the first step tried (1 degree), so that is the step the GPU test uses."""
    q = QUALITY
    w, h, spp, n = q["w"], q["h"], q["spp"], q["w"] * q["h"]
    base = pyscene.parse_lines(shade_scenes.ALL[q["case"]].text.split("\n"))
    hist = None
    for f in range(q["frames"]):
        sc = copy.copy(base)
        for name, v in orbit_fields(base.eye, base.forward, base.right, base.up, q["step_degrees"] * f).items():
            setattr(sc, name, np.array(v, f32))
        o = ol.OracleScene(sc, bounds_mode=0)
        try:
            S, Q = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
            for s in range(spp * f, spp * f + spp):
                one = np.zeros((h, w, 4), f32)
                o.render_accumulate(one, w, h, s, 1, nthreads=8)
                one = one.reshape(n, 4)
                S, Q = S + one, Q + one * one
            aov = o.render(w, h, 0, flags=ol.REFERENCE_WALK, nthreads=8, want_aov=True)["aov"]
            if f == q["frames"] - 1:
                ref = np.zeros((h, w, 4), np.float64)
                for first in range(0, q["ref_spp"], 512):
                    part = np.zeros((h, w, 4), f32)
                    o.render_accumulate(part, w, h, first, 512, nthreads=8)
                    ref += part
                ref = (ref / q["ref_spp"]).reshape(n, 4)
        finally:
            o.close()
        F = dr.features(_pinhole_rays(sc, w, h), np.ascontiguousarray(aov).reshape(-1).view(np.uint32).reshape(-1, 6))
        k = np.full(n, spp, np.uint32)
        if hist is None:
            mS, mQ, mk = S, Q, k
        else:
            # (nothing but the camera moves: the reprojected features are the features)
            mS, mQ, mk, stats = tr.temporal_accumulate(S, Q, k, F, *hist, w, h, 32, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)
            assert stats["merged"] > 0.9 * n and stats["rejected"] > 0
        hist = (mS, mQ, mk, F, (sc.eye, sc.forward, sc.right, sc.up))
    sig = (api.DENOISE_SIGMA_C, api.DENOISE_SIGMA_N, api.DENOISE_SIGMA_P)
    plain, merged = S / f32(spp), mS / mk[:, None].astype(f32)
    alone, _ = dr.denoise(S, Q, k, F, w, h, 5, *sig)
    both, _ = dr.denoise(mS, mQ, mk, F, w, h, 5, *sig)
    ok = np.ones(n, bool)
    for a in (plain, merged, alone, both, ref):
        ok &= np.all(np.isfinite(a[:, :3]), axis=1)
    assert ok.mean() > 0.99 and mk.max() == spp * q["frames"]
    mse = lambda a: float(np.mean((a[ok, :3].astype(np.float64) - ref[ok, :3]) ** 2))
    print(f"closed_box 64x64, 4 frames of 8 spp, 1 degree per frame: MSE plain {mse(plain):.4e}, temporal {mse(merged):.4e}, "
          f"denoised alone {mse(alone):.4e}, temporal + denoise {mse(both):.4e}")
    assert mse(merged) < mse(plain), (mse(merged), mse(plain))
    assert mse(both) < mse(alone), (mse(both), mse(alone))

#!/usr/bin/env python3
"""Temporal accumulation (mirt_prev_features / mirt_temporal_accumulate / api.TemporalAccumulator) measured, DESIGN.md section 6g.

    python tools/temporal_bench.py [--repeats 5] [--min-seconds 0.5] [--frames 8] [--mse-width 960] [--mse-height 540]
                                   [--reference-spp 4096] [--only i,ii]

  (i)   ms per call of mirt_prev_features and of mirt_temporal_accumulate on an 8-spp frame of scenes/tenthousand.txt at 1920 x 1080
        and 3840 x 2160 (its depth of field switched off: a pinhole), the camera one degree further round its orbit than the
        history's (so the taps are blends, not single pixels): a timed window repeats the call until it has lasted --min-seconds, between two HIP events; --repeats windows:
        median, min, max.  Beside them, from the same run, the 8-spp render of that frame and the feature pass (camera rays +
        closest hit + hit_features), and the byte models of the two kernels over their time:
          temporal, per pixel: 104 B of its own (S, Q 16 B each, k 4 B and G 32 B in; S, Q, k 36 B out) plus four taps x (4 + 16
              + 16 + 32) B = 272 B of history through the caches ("cache model", 376 B); a history pixel read once from memory
              is 68 B ("memory model", 172 B)
          prev_features, per ray: 32 B ray + 24 B hit in, 32 B out = 88 B, plus the records of the primitives hit
  (ii)  tools/anim_bench.py's sequences `camera` (the camera orbiting by 1 degree per frame) and `spheres` (and every sphere
        displaced per frame: update + build) at 8 spp and --mse-width x --mse-height, --frames frames: per frame the mean squared
        error of the linear RGB mean against a --reference-spp accumulate of the same camera and geometry, for the frame as
        sampled (plain), merged with its history (temporal), and merged then filtered with five iterations (temporal + denoise;
        beside it the filter on the plain frame alone).
Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402
from cuda_ray_tracer_amd import api  # noqa: E402

DEV = "cuda"
SPP = 8


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def summary(v, digits=4):
    s = sorted(v)
    return dict(median=round(s[len(s) // 2], digits), min=round(s[0], digits), max=round(s[-1], digits))


def window_ms(fn, min_seconds):
    """Device ms per call of one timed window: fn repeated until the window has lasted min_seconds, between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    e0.record()
    while True:
        fn()
        n += 1
        if n % 4 == 0 or n == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def orbit(cam, centre, degrees):
    """`cam` turned about the vertical axis through `centre` (tools/anim_bench.py)."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)

    def rot(v):
        return (c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2])

    eye = cam.eye.tolist()
    rel = rot([eye[k] - centre[k] for k in range(3)])
    return api._camera_with(cam, dict(eye=[rel[k] + centre[k] for k in range(3)], forward=rot(cam.forward.tolist()),
                                      right=rot(cam.right.tolist()), up=rot(cam.up.tolist())))


def load():
    stl = m.parseInput(os.path.join(ROOT, "scenes", "tenthousand.txt"))
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    raw.set_camera(dof_focus=0.0, dof_lens=0.0)      # the scene's depth of field off: reprojection is for pinhole cameras (section 6g)
    bounds = raw.tree()[3]
    return stl, raw, [0.5 * float(bounds[k] + bounds[3 + k]) for k in range(3)]


def timing(a):
    stl, raw, centre = load()
    cam0 = raw.camera()
    res = {}
    for w, h in ((1920, 1080), (3840, 2160)):
        n = w * h
        raw.set_camera(cam0)
        acc = m.TemporalAccumulator(raw, w, h, SPP)
        acc.frame()
        raw.set_camera(orbit(cam0, centre, 1.0))
        acc.frame()                                              # leaves this frame's rays, hits and moments, and the history it used
        old = 1 - acc.slot
        hS, hQ, hk = acc.hist[old]
        S, Q, k = acc.cur
        out = [torch.empty_like(t) for t in (S, Q, k)]
        scratch = torch.zeros(4 * n, device=DEV)
        prev = lambda: m.prev_features(raw, acc.rays, acc.hits, acc.reprojected, acc.prev_xyzr, None)      # noqa: E731
        merge = lambda: m.temporal_accumulate(out[0], out[1], out[2], S, Q, k, acc.reprojected, hS, hQ, hk, acc.features[old], cam0, w, h)      # noqa: E731
        render = lambda: m.render_accumulate(scratch, w, h, 0, SPP, raw)      # noqa: E731

        def features():
            m.camera_rays(raw, acc.rays, w, h, 0, params=api.render_params(w, h, 0))
            m.trace_rays(raw, acc.rays, acc.hits)
            m.hit_features(raw, acc.rays, acc.hits, acc.features[acc.slot])

        for fn in (prev, merge, render, features):
            for _ in range(3):
                fn()
        t_prev = [window_ms(prev, a.min_seconds) for _ in range(a.repeats)]
        t_merge = [window_ms(merge, a.min_seconds) for _ in range(a.repeats)]
        t_feat = [window_ms(features, a.min_seconds) for _ in range(a.repeats)]
        t_render = [window_ms(render, a.min_seconds) for _ in range(a.repeats)]
        took = float((out[2] > k).float().mean())
        med_p, med_m, med_r = (summary(t, 6)["median"] for t in (t_prev, t_merge, t_render))
        row = dict(prev_features_ms=summary(t_prev), temporal_accumulate_ms=summary(t_merge), features_ms=summary(t_feat), render_8spp_ms=summary(t_render),
                   temporal_share_of_render=round((med_p + med_m) / med_r, 5), pixels_with_history=round(took, 4),
                   temporal_cache_model_bytes=376 * n, temporal_cache_model_gb_per_s=round(376 * n / (1e6 * med_m), 1),
                   temporal_memory_model_bytes=172 * n, temporal_memory_model_gb_per_s=round(172 * n / (1e6 * med_m), 1),
                   prev_features_model_bytes=88 * n, prev_features_model_gb_per_s=round(88 * n / (1e6 * med_p), 1))
        res[f"{w}x{h}"] = row
        log(w, h, row)
        del acc, out, scratch
    raw.set_camera(cam0)
    res["overflow_events"] = raw.stats()["overflow_events"]
    raw.close()
    return res


def mse_of(x, ref, n):
    x, ref = x.view(n, 4)[:, :3].double(), ref.view(n, 4)[:, :3].double()
    ok = torch.isfinite(x).all(dim=1) & torch.isfinite(ref).all(dim=1)
    return float(((x[ok] - ref[ok]) ** 2).mean())


def sequence(a, move_spheres):
    stl, raw, centre = load()
    w, h = a.mse_width, a.mse_height
    n = w * h
    cam0 = raw.camera()
    sph = stl.array("spheres")
    base = torch.from_numpy(np.concatenate([sph["c"], sph["r"][:, None]], axis=1).astype(np.float32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1234)
    phase = torch.rand((base.shape[0], 3), generator=g, device="cuda") * (2 * math.pi)
    amp = 0.25 * base[:, 3:4]
    xyzr = base.clone()
    acc = m.TemporalAccumulator(raw, w, h, SPP)
    ref = torch.zeros(4 * n, device=DEV)
    frames = []
    for f in range(a.frames):
        raw.set_camera(orbit(cam0, centre, f + 1.0))
        if move_spheres:
            xyzr[:, :3] = base[:, :3] + amp * torch.sin(phase + 0.1 * (f + 1))
            m.update_spheres(raw, xyzr)
            m.build_lbvh_karas(raw)
        _, S, Q, k = acc.frame(denoise_iterations=5)
        plain = acc.cur[0] / float(SPP)
        merged = S.view(n, 4) / k.view(n, 1).float()
        _, alone = m.denoise_frame(raw, *acc.cur, w, h, SPP)
        ref.zero_()
        done = 0
        while done < a.reference_spp:
            c = min(256, a.reference_spp - done)
            m.render_accumulate(ref, w, h, done, c, raw)
            done += c
        ref /= float(a.reference_spp)
        row = dict(frame=f, mse_plain=mse_of(plain, ref, n), mse_temporal=mse_of(merged.reshape(-1), ref, n), mse_denoise_alone=mse_of(alone, ref, n),
                   mse_temporal_denoise=mse_of(acc.filtered, ref, n), mean_count=round(float(k.float().mean()), 2),
                   pixels_with_history=round(float((k > SPP).float().mean()), 4))
        frames.append(row)
        log("spheres" if move_spheres else "camera", row)
    out = dict(width=w, height=h, spp=SPP, reference_spp=a.reference_spp, max_history=acc.max_history, frames=frames,
               overflow_events=raw.stats()["overflow_events"])
    raw.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--mse-width", type=int, default=960)
    ap.add_argument("--mse-height", type=int, default=540)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--only", default="i,ii")
    a = ap.parse_args()
    only = set(a.only.split(","))
    out = dict(metric="temporal", repeats=a.repeats, min_seconds=a.min_seconds, spp=SPP, sigma_n=api.DENOISE_SIGMA_N, sigma_p=api.DENOISE_SIGMA_P)
    if "i" in only:
        out["timing_tenthousand"] = timing(a)
    if "ii" in only:
        out["sequences"] = dict(camera=sequence(a, False), spheres=sequence(a, True))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

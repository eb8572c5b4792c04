#!/usr/bin/env python3
"""Denoising (mirt_hit_features / mirt_denoise) measured, DESIGN.md section 6f.

    python tools/denoise_bench.py [--repeats 5] [--min-seconds 0.5] [--iterations 5] [--reference-spp 4096] [--sigma-c 1,4] [--only i,ii,iii]

  (i)   ms per mirt_denoise call on an 8-spp frame of scenes/redchair.txt at 1920 x 1080 and 3840 x 2160: a timed window repeats
        the call until it has lasted --min-seconds, between two HIP events; --repeats windows: median, min, max.  Beside it the
        two byte models of the iteration kernel over that time -- per pixel and iteration 25 taps x (16 B colour + 4 B variance +
        32 B features) through the caches, 72 B (colour and variance in and out, features in) that must come from and go to
        memory -- plus the prepare kernel's 36 B in and 20 B out; the time of the feature pass (camera rays + closest hit +
        hit_features) and of the 8-spp render of the same frame, so that the cost reads as a share of a frame.
  (ii)  mean squared error of the linear RGB mean against a --reference-spp accumulate of redchair.txt at 1920 x 1080, for 8, 16
        and 64 spp: the frame as sampled and as filtered, with the default scales and with every --sigma-c.
  (iii) the ratio tests/test_gpu_denoise.py asks to be below 1: closed_box (gi) at 64 x 64, 8 spp against mirt_render at 2048 spp.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402
from cuda_ray_tracer_amd import api  # noqa: E402

DEV = "cuda"


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


def load(name):
    stl = m.parseInput(os.path.join(ROOT, "scenes", name + ".txt"))
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    return stl, raw


class Frame:
    """The moments of an spp-sample frame and the buffers of its denoise pass."""

    def __init__(self, raw, w, h, spp):
        n = w * h
        self.raw, self.w, self.h, self.n, self.spp = raw, w, h, n, spp
        self.acc, self.asq = torch.zeros(4 * n, device=DEV), torch.zeros(4 * n, device=DEV)
        self.cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.rays = torch.empty((n, 8), device=DEV)
        self.hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
        self.feat = torch.empty((n, 8), device=DEV)
        self.work = torch.empty(m.denoise_work_bytes(w, h) // 4, device=DEV)
        self.out = torch.empty(4 * n, device=DEV)
        self.add(0, spp)
        self.features()

    def add(self, first, count):
        m.render_accumulate_pixels(self.raw, self.acc, self.w, self.h, first, count, None, self.asq, self.cnt)

    def features(self):
        m.camera_rays(self.raw, self.rays, self.w, self.h, max(self.spp, 2))
        m.trace_rays(self.raw, self.rays, self.hits)
        m.hit_features(self.raw, self.rays, self.hits, self.feat)

    def denoise(self, iterations, sigma_c=api.DENOISE_SIGMA_C):
        m.denoise(self.out, self.acc, self.asq, self.cnt, self.feat, self.w, self.h, self.work, iterations, sigma_c)
        return self.out


def timing(a):
    stl, raw = load("redchair")
    res = {}
    for w, h in ((1920, 1080), (3840, 2160)):
        fr = Frame(raw, w, h, 8)
        scratch = torch.zeros(4 * w * h, device=DEV)
        render = lambda: m.render_accumulate(scratch, w, h, 0, 8, raw)      # noqa: E731
        for _ in range(3):
            fr.denoise(a.iterations)
            render()
        dn = [window_ms(lambda: fr.denoise(a.iterations), a.min_seconds) for _ in range(a.repeats)]
        ft = [window_ms(fr.features, a.min_seconds) for _ in range(a.repeats)]
        rd = [window_ms(render, a.min_seconds) for _ in range(a.repeats)]
        n = w * h
        cache_bytes = n * (a.iterations * 25 * 52 + 56)
        memory_bytes = n * (a.iterations * 72 + 56)
        med = summary(dn, 6)["median"]
        row = dict(denoise_ms=summary(dn), features_ms=summary(ft), render_8spp_ms=summary(rd),
                   denoise_share_of_render=round(med / summary(rd, 6)["median"], 4),
                   cache_model_bytes=cache_bytes, cache_model_gb_per_s=round(cache_bytes / (1e6 * med), 1),
                   memory_model_bytes=memory_bytes, memory_model_gb_per_s=round(memory_bytes / (1e6 * med), 1))
        res[f"{w}x{h}"] = row
        log(w, h, row)
        del fr, scratch
    res["overflow_events"] = raw.stats()["overflow_events"]
    raw.close()
    return res


def mse_of(x, ref, n):
    x, ref = x.view(n, 4)[:, :3].double(), ref.view(n, 4)[:, :3].double()
    ok = torch.isfinite(x).all(dim=1) & torch.isfinite(ref).all(dim=1)
    return float(((x[ok] - ref[ok]) ** 2).mean())


def quality(a):
    stl, raw = load("redchair")
    w, h = a.mse_width, a.mse_height
    n = w * h
    ref = torch.zeros(4 * n, device=DEV)
    done = 0
    while done < a.reference_spp:
        c = min(256, a.reference_spp - done)
        m.render_accumulate(ref, w, h, done, c, raw)
        done += c
    ref /= float(a.reference_spp)
    sigmas = [api.DENOISE_SIGMA_C] + [s for s in a.sigma_c if s != api.DENOISE_SIGMA_C]
    res = dict(width=w, height=h, reference_spp=a.reference_spp, iterations=a.iterations, sigma_n=api.DENOISE_SIGMA_N, sigma_p=api.DENOISE_SIGMA_P, runs={})
    fr = Frame(raw, w, h, 8)
    have = 8
    for spp in (8, 16, 64):
        if spp > have:
            fr.add(have, spp - have)
            have = spp
        noisy = mse_of(fr.acc / float(spp), ref, n)
        row = dict(mse_noisy=noisy)
        for s in sigmas:
            d = mse_of(fr.denoise(a.iterations, s), ref, n)
            row[f"sigma_c_{s:g}"] = dict(mse_denoised=d, ratio=round(d / noisy, 4))
        res["runs"][f"{spp}spp"] = row
        log(spp, row)
    res["overflow_events"] = raw.stats()["overflow_events"]
    raw.close()
    return res


def test_ratio(a):
    import shade_scenes
    stl = m.parseText(shade_scenes.ALL["closed_box_b2_g1"].text)
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    w = h = 64
    n = w * h
    fr = Frame(raw, w, h, 8)
    ref, ref8 = torch.empty(4 * n, device=DEV), torch.empty(4 * n, dtype=torch.uint8, device=DEV)
    m.render(ref8, w, h, 2048, raw, d_float=ref)
    noisy = mse_of(fr.acc / 8.0, ref, n)
    den = mse_of(fr.denoise(5), ref, n)
    raw.close()
    return dict(scene="closed_box_b2_g1", width=w, height=h, spp=8, reference_spp=2048, mse_noisy=noisy, mse_denoised=den, ratio=round(den / noisy, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--mse-width", type=int, default=1920)
    ap.add_argument("--mse-height", type=int, default=1080)
    ap.add_argument("--sigma-c", default="1,4")
    ap.add_argument("--only", default="i,ii,iii")
    a = ap.parse_args()
    a.sigma_c = [float(s) for s in a.sigma_c.split(",") if s]
    only = set(a.only.split(","))
    out = dict(metric="denoise", iterations=a.iterations, repeats=a.repeats, min_seconds=a.min_seconds, form="direct global loads",
               sigma_c=api.DENOISE_SIGMA_C, sigma_n=api.DENOISE_SIGMA_N, sigma_p=api.DENOISE_SIGMA_P)
    if "i" in only:
        out["timing_redchair"] = timing(a)
    if "ii" in only:
        out["mse_redchair"] = quality(a)
    if "iii" in only:
        out["test_ratio"] = test_ratio(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

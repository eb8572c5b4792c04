#!/usr/bin/env python3
"""Throughput of the ray-query kernel (mirt_trace_rays), closest hit and occlusion, in G rays/s.

    python tools/query_bench.py [--repeats 5] [--min-seconds 0.5] [--skip-synthetic]

Workloads (1920 x 1080 camera rays at spp 0 unless stated):
  tenthousand   camera rays of scenes/tenthousand.txt (coherent primary rays)
  incoherent    4 M rays from the hit points of `tenthousand`, seeded uniform random directions
  redchair      camera rays of scenes/redchair.txt
  synthetic     camera rays of the 1 M sphere + 1 M triangle synthetic scene (BASELINE config 5)
Each figure is timed with HIP events over back-to-back launches totalling at least --min-seconds of device time after a warm-up,
repeated --repeats times (median, min, max).  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402


def timed(raw, rays, hits, any_hit, repeats, min_seconds):
    n = rays.shape[0]
    for _ in range(3):
        m.trace_rays(raw, rays, hits, any_hit=any_hit)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.trace_rays(raw, rays, hits, any_hit=any_hit)
    e1.record()
    torch.cuda.synchronize()
    one = max(e0.elapsed_time(e1) * 1e-3, 1e-6)
    reps = max(1, int(math.ceil(min_seconds / one)))
    rates = []
    for _ in range(repeats):
        e0.record()
        for _ in range(reps):
            m.trace_rays(raw, rays, hits, any_hit=any_hit)
        e1.record()
        torch.cuda.synchronize()
        s = e0.elapsed_time(e1) * 1e-3
        rates.append(n * reps / s * 1e-9)
    rates.sort()
    return dict(grays_per_s=round(rates[len(rates) // 2], 4), min=round(rates[0], 4), max=round(rates[-1], 4), rays=n, launches=reps,
                ms_per_launch=round(1e3 * n / (rates[len(rates) // 2] * 1e9), 4))


def camera(raw, w, h, spp=0):
    n = m.num_pixels(m.render_params(w, h, spp))
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    m.camera_rays(raw, rays, w, h, spp)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--skip-synthetic", action="store_true")
    a = ap.parse_args()
    w, h = a.width, a.height
    out = dict(metric="query_grays_per_s", width=w, height=h, repeats=a.repeats, min_seconds=a.min_seconds, results={})

    def run(name, raw, rays):
        hits = torch.empty((rays.shape[0], 6), dtype=torch.int32, device="cuda")
        res = {}
        for mode, anyh in (("closest", False), ("occlusion", True)):
            res[mode] = timed(raw, rays, hits, anyh, a.repeats, a.min_seconds)
        m.trace_rays(raw, rays, hits)
        torch.cuda.synchronize()
        t, kind, _, _ = m.unpack_hits(hits)
        res["hit_fraction"] = round(float((kind != 0).float().mean()), 4)
        out["results"][name] = res
        return hits

    for name in ("tenthousand", "redchair"):
        stl = m.parseInput(os.path.join(ROOT, "scenes", name + ".txt"))
        raw = m.initRawConfigFromStl(stl, 0)
        m.build_lbvh_karas(raw)
        rays = camera(raw, w, h)
        hits = run(name, raw, rays)
        if name == "tenthousand":
            # incoherent: seeded uniform random directions from the primary hit points
            t, kind, _, _ = m.unpack_hits(hits)
            sel = torch.nonzero(kind != 0).squeeze(1)
            d = rays[sel, 4:7]
            d = d / torch.linalg.norm(d, dim=1, keepdim=True)
            p = rays[sel, 0:3] + t[sel, None] * d
            g = torch.Generator(device="cuda").manual_seed(1234)
            pick = torch.randint(0, p.shape[0], (a.incoherent,), generator=g, device="cuda")
            dirs = torch.randn((a.incoherent, 3), generator=g, device="cuda")
            run("incoherent", raw, m.pack_rays(p[pick], dirs))
        raw.close()
    if not a.skip_synthetic:
        stl = m.syntheticScene()
        raw = m.initRawConfigFromStl(stl, 0)
        m.build_lbvh_karas(raw)
        run("synthetic", raw, camera(raw, w, h))
        raw.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

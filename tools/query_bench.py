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
import torch

import bench_common as bc
from bench_common import m


def main():
    ap = bc.parser()
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--skip-synthetic", action="store_true")
    a = ap.parse_args()
    w, h = a.width, a.height
    out = dict(metric="query_grays_per_s", **bc.settings(a), results={})

    def run(name, raw, rays):
        hits = torch.empty((rays.shape[0], 6), dtype=torch.int32, device="cuda")
        res = {}
        for mode, anyh in (("closest", False), ("occlusion", True)):
            r = bc.timed(lambda: m.trace_rays(raw, rays, hits, any_hit=anyh), rays.shape[0], a.repeats, a.min_seconds, "grays_per_s", 1e-9, 4)
            res[mode] = dict(grays_per_s=r["grays_per_s"], min=r["min"], max=r["max"], rays=rays.shape[0], launches=r["repetitions"],
                             ms_per_launch=r["ms_per_call"])
        m.trace_rays(raw, rays, hits)
        torch.cuda.synchronize()
        t, kind, _, _ = m.unpack_hits(hits)
        res["hit_fraction"] = round(float((kind != 0).float().mean()), 4)
        out["results"][name] = res

    for name in ("tenthousand", "redchair"):
        raw = bc.built(m.parseInput(bc.scene_path(name)))
        rays = bc.camera(raw, w, h)
        run(name, raw, rays)
        if name == "tenthousand":
            run("incoherent", raw, bc.incoherent_rays(raw, rays, a.incoherent))
        raw.close()
    if not a.skip_synthetic:
        raw = bc.built(m.syntheticScene())
        run("synthetic", raw, bc.camera(raw, w, h))
        raw.close()
    bc.emit(out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the multi-hit ray query (mirt_trace_rays_multi), beside closest hit and beside a peel of closest-hit calls.

    python tools/multihit_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--out profiles/multihit_bench.json]

Workloads (1920 x 1080 camera rays at spp 0 unless stated), those of tools/query_bench.py:
  tenthousand   camera rays of scenes/tenthousand.txt (coherent primary rays)
  incoherent    4 M rays from the hit points of `tenthousand`, seeded uniform random directions
  redchair      camera rays of scenes/redchair.txt
For each: the count-only call and k = 1, 4, 8 (records and counts); mirt_trace_rays (closest hit) on the same rays; and, for
k = 1, 4, 8, the only way to such lists without the call: k rounds of mirt_trace_rays with torch between them, which moves every
live ray's origin to its hit and shortens its tmax.  The peel's lists are compared with the call's once: the share of rays whose
(kind, id) sequence differs, and the share whose records differ in any bit (the moved origin changes the later hits' t and normals).
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up, repeated
--repeats times (median, min, max).  Prints one JSON line and, with --out, writes it to a file.
"""
import torch

import bench_common as bc
from bench_common import DEV, m


class Peel:
    """k rounds of closest hit.  After a round a ray that hit starts again from its hit point, t d + o (d normalised as the kernel
    normalises it), with tmax shortened by t; a ray that missed is switched off (tmax = 0).  The records' t is the sum along the
    ray.  The reference's acceptance thresholds keep a ray from finding the surface it stands on -- and anything within them."""

    def __init__(self, raw, rays, k):
        n = rays.shape[0]
        self.raw, self.rays, self.k = raw, rays, k
        self.cur = torch.empty_like(rays)
        self.hits = torch.empty((n, 6), dtype=torch.float32, device=DEV)
        self.out = torch.empty((n, k, 6), dtype=torch.float32, device=DEV)
        d = rays[:, 4:7]
        self.d = d / torch.linalg.norm(d, dim=1, keepdim=True)

    def __call__(self):
        cur, hits = self.cur, self.hits
        cur.copy_(self.rays)
        travelled = torch.zeros(cur.shape[0], dtype=torch.float32, device=DEV)
        for j in range(self.k):
            m.trace_rays(self.raw, cur, hits)
            t = hits[:, 0]
            hit = t > 0
            self.out[:, j] = hits
            self.out[:, j, 0] = torch.where(hit, travelled + t, t)
            if j + 1 < self.k:
                step = torch.where(hit, t, torch.zeros_like(t))
                travelled += step
                cur[:, 0:3] += step[:, None] * self.d
                cur[:, 3] = torch.where(hit, cur[:, 3] - t, torch.zeros_like(t))
        return self.out


def main():
    ap = bc.parser()
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = a.width, a.height
    out = dict(metric="multihit_grays_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), results={})

    def timed(fn, n):
        return bc.timed(fn, n, a.repeats, a.min_seconds, "grays_per_s", 1e-9, 4)

    def run(name, raw, rays):
        if a.only and a.only != name:
            return
        n = rays.shape[0]
        res = {}
        counts = torch.empty(n, dtype=torch.int32, device=DEV)
        hits1 = torch.empty((n, 6), dtype=torch.int32, device=DEV)
        res["closest_hit"] = timed(lambda: m.trace_rays(raw, rays, hits1), n)
        res["count_only"] = timed(lambda: m.trace_rays_multi(raw, rays, None, counts), n)
        res["hits_per_ray"] = dict(mean=round(float(counts.float().mean()), 3), max=int(counts.max()),
                                   share_above_8=round(float((counts > 8).float().mean()), 4), share_none=round(float((counts == 0).float().mean()), 4))
        for k in (1, 4, 8):
            hits = torch.empty((n, k, 6), dtype=torch.int32, device=DEV)
            res[f"k{k}"] = timed(lambda: m.trace_rays_multi(raw, rays, hits, counts), n)
            peel = Peel(raw, rays, k)
            res[f"peel{k}"] = timed(peel, n)
            res[f"peel{k}"]["times_k_call"] = round(res[f"peel{k}"]["ms_per_call"] / res[f"k{k}"]["ms_per_call"], 2)
            peeled = peel().view(torch.int32)
            torch.cuda.synchronize()
            names_differ = torch.any((peeled[:, :, 1:3] != hits[:, :, 1:3]).reshape(n, -1), dim=1)
            bits_differ = torch.any((peeled != hits).reshape(n, -1), dim=1)
            res[f"peel{k}"]["share_of_rays_with_other_primitives"] = round(float(names_differ.float().mean()), 5)
            res[f"peel{k}"]["share_of_rays_with_other_bits"] = round(float(bits_differ.float().mean()), 5)
            del peel, peeled, hits
        res["k8_over_closest_hit"] = round(res["k8"]["ms_per_call"] / res["closest_hit"]["ms_per_call"], 2)
        out["results"][name] = res

    for name in ("tenthousand", "redchair"):
        raw = bc.built(m.parseInput(bc.scene_path(name)))
        rays = bc.camera(raw, w, h)
        run(name, raw, rays)
        if name == "tenthousand":
            run("incoherent", raw, bc.incoherent_rays(raw, rays, a.incoherent))
        raw.close()
    bc.emit(out, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the closest-point query (mirt_closest_points), and of a torch brute force beside it.

    python tools/closest_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--no-brute-force] [--label TEXT] [--out profiles/closest_bench.json]

Scenes: scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene (--synthetic spheres and as many triangles).  Point
sets, each at R = inf and at R = 1 % of the scene box's diagonal; a workload's name is SCENE/POINTS/inf or SCENE/POINTS/near:
  surface   the first-hit points of the 1920 x 1080 camera rays (spp 0), moved 0.05 along the hit's normal
  uniform   as many points drawn uniformly (seeded) from the scene's box
closest      one mirt_closest_points call over the rows, with the feature rows.
brute force  on tenthousand (spheres and planes only): every point against every sphere in torch, n x N in chunks of rows -- the
             push-out step a caller had to write before.  Its ids are compared with the call's once and the rows that differ
             counted: torch rounds its own way, so near-ties may fall to another sphere.
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up, repeated
--repeats times (median, min, max).  Prints one JSON line and, with --out, writes it to a file.
"""
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, INF, m


class BruteForce:
    """The nearest sphere or plane of every row in torch: rows in chunks against all spheres at once."""

    def __init__(self, spheres, planes, rows, chunk):
        self.c, self.r = spheres[:, 0:3].contiguous(), spheres[:, 3].contiguous()
        self.planes, self.rows, self.chunk = planes, rows, chunk
        self.dist = torch.empty(rows.shape[0], dtype=torch.float32, device=DEV)
        self.idx = torch.empty(rows.shape[0], dtype=torch.int64, device=DEV)

    def __call__(self):
        for i in range(0, self.rows.shape[0], self.chunk):
            q, R = self.rows[i:i + self.chunk, 0:3], self.rows[i:i + self.chunk, 3]
            d = (torch.cdist(q, self.c) - self.r[None, :]).abs()
            best, j = d.min(dim=1)
            for k, (nor, point) in enumerate(self.planes):
                dp = ((q - point[None, :]) * nor[None, :]).sum(dim=1).abs()
                closer = dp < best
                best = torch.where(closer, dp, best)
                j = torch.where(closer, -1 - k, j)
            self.dist[i:i + self.chunk] = torch.where(best < R, best, -1.0)
            self.idx[i:i + self.chunk] = j
        return self.dist, self.idx


def measure(raw, rows, a, brute=None):
    n = rows.shape[0]
    hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    feat = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    res = dict(points=n)
    res["closest"] = bc.timed(lambda: m.closest_points(raw, rows, hits, feat), n, a.repeats, a.min_seconds, "mpoints_per_s", 1e-6)
    t, kind, pid, _ = m.unpack_hits(hits)
    found = kind != 0
    res["found_fraction"] = round(float(found.float().mean()), 4)
    res["mean_distance_of_found"] = round(float(t[found].mean()), 5) if bool(found.any()) else None
    res["kinds"] = {str(k): int((kind == k).sum()) for k in range(4)}
    if brute is not None:
        sub = rows[:a.brute_rows].contiguous()
        bf = BruteForce(brute[0], brute[1], sub, a.brute_chunk)
        dist, idx = bf()
        torch.cuda.synchronize()
        s_kind, s_pid = kind[:sub.shape[0]], pid[:sub.shape[0]].to(torch.int64)
        want = torch.where(s_kind == 3, -1 - s_pid, s_pid)
        both = (s_kind != 0) & (dist >= 0)
        res["brute_force"] = bc.timed(bf, sub.shape[0], a.repeats, a.min_seconds, "mpoints_per_s", 1e-6)
        res["brute_force"]["points"] = sub.shape[0]
        res["brute_force"]["rows_naming_another_primitive"] = int((want != idx)[both].sum())
        res["brute_force"]["rows_found_by_one_only"] = int(((s_kind != 0) != (dist >= 0)).sum())
        res["closest_over_brute_force"] = round(res["closest"]["mpoints_per_s"] / res["brute_force"]["mpoints_per_s"], 1)
    return res


def main():
    ap = bc.parser()
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--brute-rows", type=int, default=1 << 18)
    ap.add_argument("--brute-chunk", type=int, default=1 << 14)
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand/surface/near")
    ap.add_argument("--no-brute-force", action="store_true", help="skip the torch brute force")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=None, help="also write the JSON here, e.g. profiles/closest_bench.json")
    a = ap.parse_args()
    w, h = a.width, a.height
    result = dict(metric="closest_points_mpoints_per_s", **bc.settings(a), label=a.label, results={})
    for name in ("tenthousand", "redchair", "synthetic"):
        wanted = [(pts, tag) for pts in ("surface", "uniform") for tag in ("inf", "near") if a.only in (None, f"{name}/{pts}/{tag}")]
        if not wanted:
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if name == "synthetic" else m.parseInput(bc.scene_path(name))
        raw = bc.built(stl)
        box, diagonal = bc.box_diagonal(raw)
        near = 0.01 * diagonal
        F = bc.first_hit_features(raw, w, h)
        on = F[F[:, 3] != 0]
        surface = (on[:, 0:3] + on[:, 4:7] * 0.05).contiguous()
        g = torch.Generator(device=DEV).manual_seed(1234)
        lo, hi = (torch.tensor(box[k:k + 3], dtype=torch.float32, device=DEV) for k in (0, 3))
        uniform = lo + (hi - lo) * torch.rand((surface.shape[0], 3), generator=g, device=DEV)
        brute = None
        if name == "tenthousand" and raw.desc.num_triangles == 0 and not a.no_brute_force:
            xyzr = torch.empty((raw.desc.num_spheres, 4), dtype=torch.float32, device=DEV)
            m.get_spheres(raw, xyzr)
            planes = [(torch.tensor(np.array(p["nor"]), device=DEV), torch.tensor(np.array(p["point"]), device=DEV)) for p in stl.array("planes")]
            brute = (xyzr, planes)
        for pts, tag in wanted:
            rows = m.pack_points(surface if pts == "surface" else uniform, INF if tag == "inf" else near)
            r = measure(raw, rows, a, brute)
            r["radius"] = "inf" if tag == "inf" else round(near, 5)
            r["primitives"] = int(raw.desc.num_prims)
            result["results"][f"{name}/{pts}/{tag}"] = r
            print(f"{name}/{pts}/{tag} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

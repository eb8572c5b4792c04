#!/usr/bin/env python3
"""Throughput of the contact query (mirt_closest_points_multi), beside mirt_closest_points on the same rows and a torch brute force.

    python tools/contacts_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--no-brute-force] [--label TEXT] [--out profiles/contacts_bench.json]

Scenes and point sets are those of tools/closest_bench.py: scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene;
`surface` (the first-hit points of the 1920 x 1080 camera rays, moved 0.05 along the normal) and `uniform` points; a workload's
name is SCENE/POINTS.  Per workload, with `near` = 1 % of the scene box's diagonal:
  counted/count_only, counted/k1, k4, k8   R = near, with d_counts (the bound stays R) and, for k > 0, the feature rows
  near/k1, k4, k8                          R = near, without d_counts (the bound follows the list)
  inf/k1, k4, k8                           R = inf, without d_counts (a count at R = inf visits every leaf: not timed)
  closest/near, closest/inf                mirt_closest_points on the same rows, with its feature rows
  k1_over_closest                          the rate of k1 without counts over mirt_closest_points', at near and at inf: the same walk,
                                           so the ratio prices the list and the id of every candidate that reaches it
brute force  on tenthousand (spheres and planes only), R = near: every row against every sphere in torch (cdist, then topk of the 8
             nearest and the count below R), in chunks of rows -- what a caller had to write before.
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up, repeated
--repeats times (median, min, max).  Prints one JSON line and, with --out, writes it to a file.
"""
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, INF, m


class BruteForce:
    """The 8 nearest spheres or planes of every row and the number within R, in torch: rows in chunks against all spheres at once."""

    def __init__(self, spheres, planes, rows, chunk):
        self.c, self.r = spheres[:, 0:3].contiguous(), spheres[:, 3].contiguous()
        self.planes, self.rows, self.chunk = planes, rows, chunk
        self.dist = torch.empty((rows.shape[0], 8), dtype=torch.float32, device=DEV)
        self.idx = torch.empty((rows.shape[0], 8), dtype=torch.int64, device=DEV)
        self.count = torch.empty(rows.shape[0], dtype=torch.int64, device=DEV)

    def __call__(self):
        for i in range(0, self.rows.shape[0], self.chunk):
            q, R = self.rows[i:i + self.chunk, 0:3], self.rows[i:i + self.chunk, 3]
            d = (torch.cdist(q, self.c) - self.r[None, :]).abs()
            dp = [((q - point[None, :]) * nor[None, :]).sum(dim=1).abs()[:, None] for nor, point in self.planes]
            d = torch.cat([d] + dp, dim=1)
            self.count[i:i + self.chunk] = (d < R[:, None]).sum(dim=1)
            best, j = torch.topk(d, 8, dim=1, largest=False)
            self.dist[i:i + self.chunk] = torch.where(best < R[:, None], best, -1.0)
            self.idx[i:i + self.chunk] = j
        return self.dist, self.idx, self.count


def measure(raw, points, near, a, brute=None):
    n = points.shape[0]
    rows = {"near": m.pack_points(points, near), "inf": m.pack_points(points, INF)}
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    hits1 = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    feat1 = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    res = dict(points=n, radius=round(near, 5), primitives=int(raw.desc.num_prims))
    timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, "mpoints_per_s", 1e-6)
    res["counted/count_only"] = timed(lambda: m.closest_points_multi(raw, rows["near"], None, counts))
    for tag in ("near", "inf"):
        res[f"closest/{tag}"] = timed(lambda: m.closest_points(raw, rows[tag], hits1, feat1))
    for k in (1, 4, 8):
        hits = torch.empty((n, k, 6), dtype=torch.int32, device=DEV)
        feat = torch.empty((n, k, 8), dtype=torch.float32, device=DEV)
        res[f"counted/k{k}"] = timed(lambda: m.closest_points_multi(raw, rows["near"], hits, counts, feat))
        for tag in ("near", "inf"):
            res[f"{tag}/k{k}"] = timed(lambda: m.closest_points_multi(raw, rows[tag], hits, None, feat))
        if k == 1:
            # the relation the header states, at the size timed: record 0 is mirt_closest_points' record
            m.closest_points(raw, rows["inf"], hits1, feat1)
            res["k1_rows_differing_from_closest"] = int((hits[:, 0] != hits1).any(dim=1).sum() + (feat[:, 0].view(torch.int32) != feat1.view(torch.int32)).any(dim=1).sum())
    res["k1_over_closest"] = {tag: round(res[f"{tag}/k1"]["mpoints_per_s"] / res[f"closest/{tag}"]["mpoints_per_s"], 3) for tag in ("near", "inf")}
    m.closest_points_multi(raw, rows["near"], None, counts)
    res["mean_count_near"] = round(float(counts.float().mean()), 3)
    res["rows_with_more_than_8_near"] = round(float((counts > 8).float().mean()), 4)
    if brute is not None:
        sub = rows["near"][:a.brute_rows].contiguous()
        bf = BruteForce(brute[0], brute[1], sub, a.brute_chunk)
        _, _, bcount = bf()
        torch.cuda.synchronize()
        res["brute_force"] = bc.timed(bf, sub.shape[0], a.repeats, a.min_seconds, "mpoints_per_s", 1e-6)
        res["brute_force"]["points"] = sub.shape[0]
        res["brute_force"]["rows_with_another_count"] = int((bcount != counts[:sub.shape[0]].to(torch.int64)).sum())
        res["counted_k8_over_brute_force"] = round(res["counted/k8"]["mpoints_per_s"] / res["brute_force"]["mpoints_per_s"], 1)
    return res


def main():
    ap = bc.parser()
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--brute-rows", type=int, default=1 << 18)
    ap.add_argument("--brute-chunk", type=int, default=1 << 13)
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand/surface")
    ap.add_argument("--no-brute-force", action="store_true", help="skip the torch brute force")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=None, help="also write the JSON here, e.g. profiles/contacts_bench.json")
    a = ap.parse_args()
    w, h = a.width, a.height
    result = dict(metric="contacts_mpoints_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), label=a.label, results={})
    for name in ("tenthousand", "redchair", "synthetic"):
        wanted = [pts for pts in ("surface", "uniform") if a.only in (None, f"{name}/{pts}")]
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
            planes = [(nor / nor.norm(), point) for nor, point in planes]
            brute = (xyzr, planes)
        for pts in wanted:
            result["results"][f"{name}/{pts}"] = measure(raw, surface if pts == "surface" else uniform, near, a, brute)
            print(f"{name}/{pts} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

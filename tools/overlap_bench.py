#!/usr/bin/env python3
"""Throughput of the box overlap query (mirt_overlap_boxes) on voxel grids, beside what a caller had before it: count_within with
each voxel's circumscribed ball, and a torch brute force.

    python tools/overlap_bench.py [--grids 128 256] [--only NAME] [--no-brute-force] [--label TEXT] [--out profiles/overlap_bench.json]

Scenes: scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene (1 M spheres and 1 M triangles).  Per scene the box of its
primitives is cut into G x G x G voxels (overlap.voxel_rows: x fastest, neighbours sharing their faces' bit patterns); a workload's
name is SCENE/G.  Per workload:
  any                   count_overlaps with any_overlap (the occupancy grid's call): the walk ends at the first surface found
  count_only            count_overlaps
  k1, k4, k8            overlap_boxes with that many records, counts and feature rows
  ball                  contacts.count_within on the rows (m, |h| (1 + 2^-20)): the ball around the voxel, the query of the parent commit
  occupied              the share of voxels a surface touches; mean_count and rows_with_more_than_8
  ball_marks_too_many   of the voxels the ball marks (count > 0), the share the exact query leaves empty
brute force  on tenthousand (spheres and planes only): --brute-rows voxels against every sphere and plane in torch, the header's two
             tests in chunks of rows; rows_with_another_count compares its counts with the kernel's.
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds (0.3) of device time after a warm-up, repeated
--repeats (3) times: median, min, max.  Prints one JSON line and writes it to --out.
"""
import os
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, m


class BruteForce:
    """The number of spheres and planes every voxel touches, in torch: rows in chunks against all spheres at once."""

    def __init__(self, spheres, planes, rows, chunk):
        self.c, self.rr = spheres[:, 0:3].contiguous(), (spheres[:, 3] * spheres[:, 3]).contiguous()
        self.planes, self.rows, self.chunk = planes, rows, chunk
        self.count = torch.empty(rows.shape[0], dtype=torch.int64, device=DEV)

    def __call__(self):
        zero = torch.zeros((), dtype=torch.float32, device=DEV)
        for i in range(0, self.rows.shape[0], self.chunk):
            lo, hi = self.rows[i:i + self.chunk, None, 0:3], self.rows[i:i + self.chunk, None, 4:7]
            c = self.c[None, :, :]
            dn = torch.maximum(torch.maximum(lo - c, c - hi), zero)
            df = torch.maximum((c - lo).abs(), (hi - c).abs())
            touch = ((dn * dn).sum(dim=2) <= self.rr[None, :]) & ((df * df).sum(dim=2) >= self.rr[None, :])
            n = touch.sum(dim=1)
            mid, half = (lo[:, 0] + hi[:, 0]) * 0.5, (hi[:, 0] - lo[:, 0]) * 0.5
            for nor, point in self.planes:
                n = n + (((mid - point[None, :]) * nor[None, :]).sum(dim=1).abs() <= (half * nor.abs()[None, :]).sum(dim=1))
            self.count[i:i + self.chunk] = n
        return self.count


def measure(raw, box, G, a, brute=None):
    rows = m.voxel_rows(box[0:3], box[3:6], (G, G, G), device=DEV)
    n = rows.shape[0]
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    res = dict(voxels=n, primitives=int(raw.desc.num_prims))
    timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, "mboxes_per_s", 1e-6)
    res["any"] = timed(lambda: m.count_overlaps(raw, rows, counts, any_overlap=True))
    res["count_only"] = timed(lambda: m.count_overlaps(raw, rows, counts))
    for k in (1, 4, 8):
        hits = torch.empty((n, k, 6), dtype=torch.int32, device=DEV)
        feat = torch.empty((n, k, 8), dtype=torch.float32, device=DEV)
        res[f"k{k}"] = timed(lambda: m.overlap_boxes(raw, rows, hits, counts, feat))
        del hits, feat
    m.count_overlaps(raw, rows, counts)
    exact = counts.clone()
    res["occupied"] = round(float((exact > 0).float().mean()), 5)
    res["mean_count"] = round(float(exact.float().mean()), 4)
    res["rows_with_more_than_8"] = round(float((exact > 8).float().mean()), 5)
    some = m.count_overlaps(raw, rows, any_overlap=True)
    res["any_rows_differing_from_count"] = int(((some != 0) != (exact > 0)).sum())
    # what the parent commit offers: the ball around the voxel
    mid, half = (rows[:, 0:3] + rows[:, 4:7]) * 0.5, (rows[:, 4:7] - rows[:, 0:3]) * 0.5
    balls = m.pack_points(mid, torch.linalg.norm(half, dim=1) * (1.0 + 2.0 ** -20))
    res["ball"] = timed(lambda: m.count_within(raw, balls, counts))
    m.count_within(raw, balls, counts)
    marked = counts > 0
    res["ball_occupied"] = round(float(marked.float().mean()), 5)
    res["ball_marks_too_many"] = round(float((marked & (exact == 0)).sum()) / max(int(marked.sum()), 1), 5)
    res["exact_rows_the_ball_misses"] = int(((exact > 0) & ~marked).sum())
    res["count_only_over_ball"] = round(res["count_only"]["mboxes_per_s"] / res["ball"]["mboxes_per_s"], 3)
    if brute is not None:
        g = torch.Generator(device=DEV).manual_seed(1234)
        pick = torch.randint(0, n, (a.brute_rows,), generator=g, device=DEV)
        sub = rows[pick].contiguous()
        bf = BruteForce(brute[0], brute[1], sub, a.brute_chunk)
        bcount = bf().clone()
        torch.cuda.synchronize()
        res["brute_force"] = bc.timed(bf, sub.shape[0], a.repeats, a.min_seconds, "mboxes_per_s", 1e-6)
        res["brute_force"]["voxels"] = sub.shape[0]
        res["brute_force"]["rows_with_another_count"] = int((bcount != exact[pick].to(torch.int64)).sum())
        res["count_only_over_brute_force"] = round(res["count_only"]["mboxes_per_s"] / res["brute_force"]["mboxes_per_s"], 1)
    return res


def main():
    ap = bc.parser()
    ap.set_defaults(repeats=3, min_seconds=0.3)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256], help="voxels per axis")
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--brute-rows", type=int, default=1 << 16)
    ap.add_argument("--brute-chunk", type=int, default=1 << 10)
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand/128")
    ap.add_argument("--no-brute-force", action="store_true", help="skip the torch brute force")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "overlap_bench.json"))
    a = ap.parse_args()
    result = dict(metric="overlap_mboxes_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), label=a.label, results={})
    for name in ("tenthousand", "redchair", "synthetic"):
        wanted = [G for G in a.grids if a.only in (None, f"{name}/{G}")]
        if not wanted:
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if name == "synthetic" else m.parseInput(bc.scene_path(name))
        raw = bc.built(stl)
        box, _ = bc.box_diagonal(raw)
        brute = None
        if name == "tenthousand" and raw.desc.num_triangles == 0 and not a.no_brute_force:
            xyzr = torch.empty((raw.desc.num_spheres, 4), dtype=torch.float32, device=DEV)
            m.get_spheres(raw, xyzr)
            planes = [(torch.tensor(np.array(p["nor"]), device=DEV), torch.tensor(np.array(p["point"]), device=DEV)) for p in stl.array("planes")]
            planes = [(nor / nor.norm(), point) for nor, point in planes]
            brute = (xyzr, planes)
        for G in wanted:
            result["results"][f"{name}/{G}"] = measure(raw, box, G, a, brute)
            print(f"{name}/{G} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the overlap lists (mirt_list_offsets, mirt_overlap_list) on voxel grids: the three steps of a list one by one and
together, beside the record call that loses the rows past eight and a torch brute force.

    python tools/overlap_list_bench.py [--grids 128 256] [--only NAME] [--no-brute-force] [--once] [--label TEXT] [--out profiles/overlap_list_bench.json]

Scenes and grids are tools/overlap_bench.py's: scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene (1 M spheres and
1 M triangles), the box of the primitives cut into G x G x G voxels; a workload's name is SCENE/G.  Per workload:
  count                 count_overlaps (the count-only call)
  offsets               list_offsets of those counts (its workspace allocated once, outside the timed region)
  fill                  overlap_list into an array of exactly the total; words_per_s beside the boxes per second
  count_offsets_fill    the three back to back, the array sized beforehand (the host read of the total is not in it)
  overlap_lists         the wrapper as a caller uses it: the three, the host read of the total and the allocation
  k8                    overlap_boxes with 8 records, counts and feature rows -- it loses the rows past eight: rows_truncated_by_k8
  mean_list, max_list   list lengths over all voxels; mean_list_nonempty over the occupied ones
brute force  on tenthousand (spheres and planes only): tools/overlap_bench.py's, --brute-rows voxels against every sphere and plane
             in torch, made into lists by torch.nonzero; same_lists compares every row's sorted words with the kernel's.
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds (0.3) of device time after a warm-up, repeated
--repeats (3) times: median, min, max.  --once: every step once, untimed (for a kernel trace).  Prints one JSON line and writes it
to --out.
"""
import importlib
import os
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, m
from overlap_bench import BruteForce
from cuda_ray_tracer_amd import api, binding

OL = importlib.import_module("cuda_ray_tracer_amd.overlap_list")      # (the package's attribute of that name is the function)


class BruteLists(BruteForce):
    """The brute force's lists: (row, word) pairs of every touching sphere and plane, rows ascending and words ascending in a row."""

    def __call__(self):
        zero = torch.zeros((), dtype=torch.float32, device=DEV)
        out = []
        for i in range(0, self.rows.shape[0], self.chunk):
            lo, hi = self.rows[i:i + self.chunk, None, 0:3], self.rows[i:i + self.chunk, None, 4:7]
            c = self.c[None, :, :]
            dn = torch.maximum(torch.maximum(lo - c, c - hi), zero)
            df = torch.maximum((c - lo).abs(), (hi - c).abs())
            touch = ((dn * dn).sum(dim=2) <= self.rr[None, :]) & ((df * df).sum(dim=2) >= self.rr[None, :])
            mid, half = (lo[:, 0] + hi[:, 0]) * 0.5, (hi[:, 0] - lo[:, 0]) * 0.5
            pl = [((mid - point[None, :]) * nor[None, :]).sum(dim=1).abs() <= (half * nor.abs()[None, :]).sum(dim=1) for nor, point in self.planes]
            both = torch.cat([touch] + [p[:, None] for p in pl], dim=1)      # columns: the spheres, then the planes -- ascending words
            rc = torch.nonzero(both)
            ns = touch.shape[1]
            word = torch.where(rc[:, 1] < ns, rc[:, 1] + (1 << 30), rc[:, 1] - ns + (3 << 30))
            out.append(((rc[:, 0] + i) << 32) | word)
        return torch.cat(out)


def measure(raw, box, G, a, brute=None):
    rows = m.voxel_rows(box[0:3], box[3:6], (G, G, G), device=DEV)
    n = rows.shape[0]
    res = dict(voxels=n, primitives=int(raw.desc.num_prims))
    if a.once:
        timed = lambda fn, items=n: (fn(), torch.cuda.synchronize(), None)[2]
    else:
        timed = lambda fn, items=n: bc.timed(fn, items, a.repeats, a.min_seconds, "mboxes_per_s", 1e-6)
    counts = m.count_overlaps(raw, rows)
    offsets = m.list_offsets(raw, counts)
    total = int(offsets[-1])
    words = torch.empty(total, dtype=torch.int32, device=DEV)
    work_bytes = m.list_offsets_work_bytes(n)
    work = torch.empty(max(work_bytes // 8, 1), dtype=torch.int64, device=DEV)
    L, P, S = OL.lib(), api._ptr, api._stream_ptr

    def scan():
        binding._check(L.mirt_list_offsets(raw._h, P(counts), n, P(offsets), P(work) if work_bytes else None, S(None)))

    def all_three():
        m.count_overlaps(raw, rows, counts)
        scan()
        m.overlap_list(raw, rows, offsets, words)

    res["count"] = timed(lambda: m.count_overlaps(raw, rows, counts))
    res["offsets"] = timed(scan)
    res["fill"] = timed(lambda: m.overlap_list(raw, rows, offsets, words))
    res["count_offsets_fill"] = timed(all_three)
    res["overlap_lists"] = timed(lambda: m.overlap_lists(raw, rows))
    hits = torch.empty((n, 8, 6), dtype=torch.int32, device=DEV)
    feat = torch.empty((n, 8, 8), dtype=torch.float32, device=DEV)
    res["k8"] = timed(lambda: m.overlap_boxes(raw, rows, hits, counts, feat))
    del hits, feat
    lens = counts.to(torch.int64)
    res["total_words"] = total
    res["mean_list"] = round(total / n, 4)
    res["mean_list_nonempty"] = round(total / max(int((lens > 0).sum()), 1), 3)
    res["max_list"] = int(lens.max())
    res["occupied"] = round(float((lens > 0).float().mean()), 5)
    res["rows_truncated_by_k8"] = round(float((lens > 8).float().mean()), 5)
    res["words_lost_by_k8"] = round(float((lens - 8).clamp(min=0).sum()) / max(total, 1), 5)
    if not a.once:
        res["fill"]["mwords_per_s"] = round(total / (res["fill"]["ms_per_call"] * 1e-3) * 1e-6, 1)
        res["count_offsets_fill"]["mwords_per_s"] = round(total / (res["count_offsets_fill"]["ms_per_call"] * 1e-3) * 1e-6, 1)
        res["fill_over_count"] = round(res["fill"]["ms_per_call"] / res["count"]["ms_per_call"], 3)
        res["count_offsets_fill_over_count"] = round(res["count_offsets_fill"]["ms_per_call"] / res["count"]["ms_per_call"], 3)
    if brute is not None and not a.once:
        g = torch.Generator(device=DEV).manual_seed(1234)
        pick = torch.randint(0, n, (a.brute_rows,), generator=g, device=DEV)
        sub = rows[pick].contiguous()
        bf = BruteLists(brute[0], brute[1], sub, a.brute_chunk)
        keys = bf().clone()
        sub_off, sub_words = m.overlap_lists(raw, sub, sort=True)
        row = torch.repeat_interleave(torch.arange(sub.shape[0], dtype=torch.int64, device=DEV), sub_off[1:] - sub_off[:-1])
        mine = (row << 32) | (sub_words.to(torch.int64) & 0xffffffff)
        same = keys.shape == mine.shape and bool(torch.equal(keys, mine))
        res["brute_force"] = bc.timed(bf, sub.shape[0], a.repeats, a.min_seconds, "mboxes_per_s", 1e-6)
        res["brute_force"]["voxels"] = sub.shape[0]
        res["brute_force"]["same_lists"] = same
        res["count_offsets_fill_over_brute_force"] = round(res["count_offsets_fill"]["mboxes_per_s"] / res["brute_force"]["mboxes_per_s"], 1)
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
    ap.add_argument("--once", action="store_true", help="every step once, untimed")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "overlap_list_bench.json"))
    a = ap.parse_args()
    result = dict(metric="overlap_list_mboxes_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), label=a.label, results={})
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

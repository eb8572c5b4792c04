#!/usr/bin/env python3
"""Throughput of the cast lists (mirt_cast_counts, mirt_cast_list): the three steps of a list one by one and together, beside
mirt_cast_spheres (first contact, any contact) on the same rows.

    python tools/cast_lists_bench.py [--rays 1048576] [--only NAME] [--once] [--label TEXT] [--out profiles/cast_lists_bench.json]

Workloads: those of tools/spherecast_bench.py -- scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene; `--rays`
incoherent casts from lifted first-hit points in uniform random directions, the ball's radius in the classes r0, r1, r10, tmax = inf
(--tmax-diagonals X: tmax = X diagonals of the scene's box instead, a sweep over a step and not to the end of the scene).  A workload
whose lists hold more than --max-words words in all is counted only.
Per workload:
  count                 mirt_cast_counts
  offsets               list_offsets of those counts (its workspace allocated once, outside the timed region)
  fill                  mirt_cast_list with the value array, into arrays of exactly the total; mwords_per_s beside the rows per second
  fill_words            the same without the value array (the other instance of the kernel)
  count_offsets_fill    the three back to back, the arrays sized beforehand (the host read of the total is not in it)
  lists                 the wrapper as a caller uses it: the three, the host read of the total and the allocations
  first, any            mirt_cast_spheres on the same rows without feature rows: the yardstick, code the lists do not touch
  count_over_first, fill_over_count, fill_words_over_count, count_offsets_fill_over_count    ms per call over ms per call
  words_per_row, longest_row, rows_with_a_list, rows_with_more_than_one
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds (0.3) of device time after a warm-up, repeated
--repeats (3) times: median, min, max.  --once: every step once, untimed (for a kernel trace).  Prints one JSON line and writes it
to --out.
"""
import importlib
import os
import sys

import torch

import bench_common as bc
import spherecast_bench as sb
from bench_common import DEV, INF, m
from cuda_ray_tracer_amd import api, binding

OL = importlib.import_module("cuda_ray_tracer_amd.overlap_list")      # (the package's attribute of that name is the function)


def measure(raw, casts, a):
    n = casts.shape[0]
    res = dict(rows=n)
    if a.once:
        timed = lambda fn: (fn(), torch.cuda.synchronize(), None)[2]
    else:
        timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, "mcasts_per_s", 1e-6)
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    count_into = lambda: m.count_casts(raw, casts, counts)
    count_into()
    offsets = m.list_offsets(raw, counts)
    total = int(offsets[-1])
    lens = counts.to(torch.int64)
    res["total_words"] = total
    res["words_per_row"] = round(total / n, 4)
    res["longest_row"] = int(lens.max())
    res["rows_with_a_list"] = round(float((lens > 0).float().mean()), 5)
    res["rows_with_more_than_one"] = round(float((lens > 1).float().mean()), 5)
    hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    res["count"] = timed(count_into)
    res["first"] = timed(lambda: m.cast_spheres(raw, casts, hits))
    res["any"] = timed(lambda: m.cast_spheres(raw, casts, hits, any_hit=True))
    if not a.once:
        res["count_over_first"] = round(res["count"]["ms_per_call"] / res["first"]["ms_per_call"], 3)
        res["count_over_any"] = round(res["count"]["ms_per_call"] / res["any"]["ms_per_call"], 3)
    if total > a.max_words:
        res["fills_skipped"] = True
        return res
    words = torch.empty(total, dtype=torch.int32, device=DEV)
    vals = torch.empty(total, dtype=torch.float32, device=DEV)
    work_bytes = m.list_offsets_work_bytes(n)
    work = torch.empty(max(work_bytes // 8, 1), dtype=torch.int64, device=DEV)
    L, P, S = OL.lib(), api._ptr, api._stream_ptr

    def scan():
        binding._check(L.mirt_list_offsets(raw._h, P(counts), n, P(offsets), P(work) if work_bytes else None, S(None)))

    def all_three():
        count_into()
        scan()
        m.cast_list(raw, casts, offsets, words, vals)

    res["offsets"] = timed(scan)
    res["fill"] = timed(lambda: m.cast_list(raw, casts, offsets, words, vals))
    res["fill_words"] = timed(lambda: m.cast_list(raw, casts, offsets, words))
    res["count_offsets_fill"] = timed(all_three)
    res["lists"] = timed(lambda: m.cast_lists(raw, casts))
    if not a.once:
        for step in ("fill", "fill_words", "count_offsets_fill"):
            res[step]["mwords_per_s"] = round(total / (res[step]["ms_per_call"] * 1e-3) * 1e-6, 1)
            res[step + "_over_count"] = round(res[step]["ms_per_call"] / res["count"]["ms_per_call"], 3)
    return res


def main():
    ap = bc.parser()
    ap.set_defaults(repeats=3, min_seconds=0.3)
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--tmax-diagonals", type=float, default=0.0, help="tmax of every row, in diagonals of the scene's box (0: inf)")
    ap.add_argument("--max-words", type=int, default=1 << 31, help="a workload with more words in all is counted, not filled")
    ap.add_argument("--only", default=None, help="one scene, e.g. tenthousand")
    ap.add_argument("--once", action="store_true", help="every step once, untimed")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "cast_lists_bench.json"))
    a = ap.parse_args()
    result = dict(metric="cast_lists_ms_per_call", device=torch.cuda.get_device_name(0), **bc.settings(a), rays=a.rays, tmax_diagonals=a.tmax_diagonals,
                  label=a.label, results={})
    for name in ("tenthousand", "redchair", "synthetic"):
        if a.only not in (None, name):
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if name == "synthetic" else m.parseInput(bc.scene_path(name))
        raw = bc.built(stl)
        _, diagonal = bc.box_diagonal(raw)
        prim = sb.primitive_size(raw)
        p, nn, dirs = sb.surface_points(raw, a.width, a.height, a.rays)
        result["results"][name] = dict(primitives=int(raw.desc.num_prims), primitive_size=round(prim, 6), diagonal=round(diagonal, 4))
        for tag, radius in (("r0", 0.0), ("r1", prim), ("r10", 10.0 * prim)):
            casts = m.pack_casts(p + nn * (1.5 * radius + 1e-3 * diagonal), dirs, a.tmax_diagonals * diagonal if a.tmax_diagonals > 0 else INF, radius)
            result["results"][name][tag] = dict(radius=round(radius, 6), **measure(raw, casts, a))
            print(f"{name}/{tag} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

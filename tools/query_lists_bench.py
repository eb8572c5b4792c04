#!/usr/bin/env python3
"""Throughput of the ray and ball lists (mirt_ray_list, mirt_ball_list): the three steps of a list one by one and together, beside
the record call that loses the rows past eight.

    python tools/query_lists_bench.py [--scenes NAME ...] [--only NAME] [--once] [--label TEXT] [--out profiles/query_lists_bench.json]

Ray workloads (rays/NAME): the 1920 x 1080 camera rays of scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene (1 M
spheres and 1 M triangles), all with tmax = inf, and `dense`: the dense test scene and rays of tests/test_multihit_abi.py
(dense_scene_text, dense_rays), the 4000 rays tiled to --dense-rays (2^20).
Ball workloads (balls/SCENE/POINTS): the point sets and the radius of tools/contacts_bench.py -- `surface` (the first-hit points of the
camera rays, moved 0.05 along the normal) and `uniform` points, R = 1 % of the scene box's diagonal.
Per workload:
  count                 the count-only call (count_hits / count_within): the yardstick, code the lists do not touch
  offsets               list_offsets of those counts (its workspace allocated once, outside the timed region)
  fill                  ray_list / ball_list with the value array, into arrays of exactly the total; words_per_s beside the rows per second
  fill_words            the same without the value array (the other instance of the kernel)
  count_offsets_fill    the three back to back, the arrays sized beforehand (the host read of the total is not in it)
  lists                 the wrapper as a caller uses it: the three, the host read of the total and the allocations
  k8                    the record call with 8 records and counts -- it loses the rows past eight: rows_truncated_by_k8
  fill_over_count, fill_words_over_count, count_offsets_fill_over_count   ms per call over the count-only call's
  mean_list, max_list   list lengths over all rows; mean_list_nonempty over the rows with a list
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
from bench_common import DEV, INF, m
from cuda_ray_tracer_amd import api, binding

OL = importlib.import_module("cuda_ray_tracer_amd.overlap_list")      # (the package's attribute of that name is the function)


def measure(raw, kind, rows, a):
    n = rows.shape[0]
    count, fill, lists = (m.count_hits, m.ray_list, m.ray_lists) if kind == "rays" else (m.count_within, m.ball_list, m.ball_lists)
    unit = "mrays_per_s" if kind == "rays" else "mpoints_per_s"
    res = dict(rows=n, primitives=int(raw.desc.num_prims))
    if a.once:
        timed = lambda fn: (fn(), torch.cuda.synchronize(), None)[2]
    else:
        timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, unit, 1e-6)
    counts = torch.empty(n, dtype=torch.int32, device=DEV)
    if kind == "rays":
        count_into = lambda: m.trace_rays_multi(raw, rows, None, counts)
    else:
        count_into = lambda: m.count_within(raw, rows, counts)
    count_into()
    offsets = m.list_offsets(raw, counts)
    total = int(offsets[-1])
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
        fill(raw, rows, offsets, words, vals)

    res["count"] = timed(count_into)
    res["offsets"] = timed(scan)
    res["fill"] = timed(lambda: fill(raw, rows, offsets, words, vals))
    res["fill_words"] = timed(lambda: fill(raw, rows, offsets, words))
    res["count_offsets_fill"] = timed(all_three)
    res["lists"] = timed(lambda: lists(raw, rows))
    hits = torch.empty((n, 8, 6), dtype=torch.int32, device=DEV)
    if kind == "rays":
        res["k8"] = timed(lambda: m.trace_rays_multi(raw, rows, hits, counts))
    else:
        res["k8"] = timed(lambda: m.closest_points_multi(raw, rows, hits, counts))
    del hits
    lens = counts.to(torch.int64)
    res["total_words"] = total
    res["mean_list"] = round(total / n, 4)
    res["mean_list_nonempty"] = round(total / max(int((lens > 0).sum()), 1), 3)
    res["max_list"] = int(lens.max())
    res["rows_with_a_list"] = round(float((lens > 0).float().mean()), 5)
    res["rows_truncated_by_k8"] = round(float((lens > 8).float().mean()), 5)
    res["words_lost_by_k8"] = round(float((lens - 8).clamp(min=0).sum()) / max(total, 1), 5)
    if not a.once:
        for step in ("fill", "fill_words", "count_offsets_fill"):
            res[step]["mwords_per_s"] = round(total / (res[step]["ms_per_call"] * 1e-3) * 1e-6, 1)
            res[step + "_over_count"] = round(res[step]["ms_per_call"] / res["count"]["ms_per_call"], 3)
        res["k8_over_count"] = round(res["k8"]["ms_per_call"] / res["count"]["ms_per_call"], 3)
    return res


def dense_workload(count):
    """(the dense test scene parsed, its rays tiled to `count`): the inputs tests/test_multihit_abi.py checks the restatement on."""
    sys.path.insert(0, os.path.join(bc.ROOT, "tests"))
    import test_multihit_abi as tma
    base = tma.dense_rays(INF)
    rays = np.tile(base, (-(-count // len(base)), 1))[:count]
    return m.parseText(tma.dense_scene_text()), torch.from_numpy(np.ascontiguousarray(rays)).to(DEV)


def main():
    ap = bc.parser()
    ap.set_defaults(repeats=3, min_seconds=0.3)
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--scenes", nargs="+", default=["tenthousand", "redchair", "synthetic", "dense"], help="the scenes measured")
    ap.add_argument("--dense-rays", type=int, default=1 << 20)
    ap.add_argument("--only", default=None, help="one workload, e.g. rays/tenthousand or balls/redchair/surface")
    ap.add_argument("--once", action="store_true", help="every step once, untimed")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "query_lists_bench.json"))
    a = ap.parse_args()
    w, h = a.width, a.height
    wanted = lambda name: a.only in (None, name)
    result = dict(metric="query_lists_ms_per_call", device=torch.cuda.get_device_name(0), **bc.settings(a), label=a.label, results={})

    def run(name, raw, kind, rows):
        result["results"][name] = measure(raw, kind, rows, a)
        print(f"{name} done", file=sys.stderr, flush=True)

    for scene in ("tenthousand", "redchair", "synthetic"):
        names = [f"rays/{scene}", f"balls/{scene}/surface", f"balls/{scene}/uniform"]
        if scene not in a.scenes or not any(wanted(x) for x in names):
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if scene == "synthetic" else m.parseInput(bc.scene_path(scene))
        raw = bc.built(stl)
        if wanted(names[0]):
            rays = bc.camera(raw, w, h)
            rays[:, 3] = INF
            run(names[0], raw, "rays", rays)
            del rays
        if wanted(names[1]) or wanted(names[2]):
            box, diagonal = bc.box_diagonal(raw)
            near = 0.01 * diagonal
            F = bc.first_hit_features(raw, w, h)
            on = F[F[:, 3] != 0]
            surface = (on[:, 0:3] + on[:, 4:7] * 0.05).contiguous()
            g = torch.Generator(device=DEV).manual_seed(1234)
            lo, hi = (torch.tensor(box[k:k + 3], dtype=torch.float32, device=DEV) for k in (0, 3))
            uniform = lo + (hi - lo) * torch.rand((surface.shape[0], 3), generator=g, device=DEV)
            for name, points in ((names[1], surface), (names[2], uniform)):
                if wanted(name):
                    run(name, raw, "balls", m.pack_points(points, near))
        raw.close()
    if "dense" in a.scenes and wanted("rays/dense"):
        stl, rays = dense_workload(a.dense_rays)
        raw = bc.built(stl)
        run("rays/dense", raw, "rays", rays)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

"""What the query benches share (query_bench, light_bench, visibility_bench, indirect_bench, closest_bench, multihit_bench, contacts_bench, spherecast_bench, overlap_bench,
overlap_list_bench, query_lists_bench):
the timing loop, the scenes, the rays and rows they start from, and the JSON line they end with.  Imported by them, not run."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402

DEV = "cuda"
INF = float("inf")


def timed(fn, items, repeats, min_seconds, unit, scale, digits=3):
    """fn() handles `items` items (rays, rows, points).  After a warm-up, HIP events around back-to-back calls totalling at least
    min_seconds of device time, `repeats` times: the median, min and max rate in `unit` (items per second times `scale`)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    one = max(e0.elapsed_time(e1) * 1e-3, 1e-6)
    reps = max(1, int(math.ceil(min_seconds / one)))
    rates = []
    for _ in range(repeats):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        rates.append(items * reps / (e0.elapsed_time(e1) * 1e-3))
    rates.sort()
    med = rates[len(rates) // 2]
    return {unit: round(med * scale, digits), "min": round(rates[0] * scale, digits), "max": round(rates[-1] * scale, digits), "repetitions": reps,
            "ms_per_call": round(1e3 * items / med, 4)}


def parser():
    """The options every bench has."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    return ap


def settings(a):
    """The parsed options a result records."""
    return dict(width=a.width, height=a.height, repeats=a.repeats, min_seconds=a.min_seconds)


def scene_path(name):
    return os.path.join(ROOT, "scenes", name + ".txt")


def built(stl):
    """A parsed scene on device 0 with its tree built."""
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    return raw


def camera(raw, w, h, spp=0):
    """The camera rays of a w x h frame, float32 [n, 8]."""
    n = m.num_pixels(m.render_params(w, h, spp))
    rays = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    m.camera_rays(raw, rays, w, h, spp)
    return rays


def incoherent_rays(raw, rays, count):
    """`count` rays from the hit points of `rays`, picked and given uniform random directions by one seeded generator."""
    hits = torch.empty((rays.shape[0], 6), dtype=torch.int32, device=DEV)
    m.trace_rays(raw, rays, hits)
    t, kind, _, _ = m.unpack_hits(hits)
    sel = torch.nonzero(kind != 0).squeeze(1)
    d = rays[sel, 4:7]
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    p = rays[sel, 0:3] + t[sel, None] * d
    g = torch.Generator(device=DEV).manual_seed(1234)
    pick = torch.randint(0, p.shape[0], (count,), generator=g, device=DEV)
    dirs = torch.randn((count, 3), generator=g, device=DEV)
    return m.pack_rays(p[pick], dirs)


def first_hit_features(raw, w, h):
    """The feature rows of the first hits of the camera rays of a w x h frame (spp 0), float32 [n, 8]."""
    _, _, F = m.ambient_occlusion_frame(raw, w, h, 0, directions=1)
    return F


def incoherent_rows(rows, count):
    """`count` of `rows` drawn at random (seeded): neighbouring lanes, far-apart points."""
    g = torch.Generator(device=DEV).manual_seed(1234)
    return rows[torch.randint(0, rows.shape[0], (count,), generator=g, device=DEV)].contiguous()


def box_diagonal(raw):
    """(the scene box as float64 [6], the length of its diagonal)"""
    import numpy as np
    box = raw.tree()[3].astype(np.float64)
    return box, float(np.linalg.norm(box[3:6] - box[0:3]))


def emit(result, out=None, indent=None):
    """Prints the result as one JSON line and, with `out`, writes it there (indented by `indent`)."""
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(result, indent=indent) + "\n")
    print(json.dumps(result), flush=True)

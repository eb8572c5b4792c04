#!/usr/bin/env python3
"""Throughput of the sphere cast (mirt_cast_spheres), beside mirt_trace_rays on the same rays and conservative advancement built from
mirt_closest_points.

    python tools/spherecast_bench.py [--repeats 5] [--min-seconds 0.5] [--rays 1048576] [--only NAME] [--label TEXT] [--out profiles/spherecast_bench.json]

Scenes: scenes/tenthousand.txt, scenes/redchair.txt and the synthetic scene.  Casts: `--rays` incoherent casts, tmax = inf, with the
ball's radius in three classes -- `r0` = 0, `r1` = about a primitive (the median sphere radius or half a triangle's longest edge),
`r10` = ten times that.  A cast starts at a first-hit point of the 1920 x 1080 camera rays (picked at random, seeded) lifted off its
surface along the normal by 1.5 r plus a thousandth of the scene's diagonal, in a uniform random direction.  Per scene and class:
  first, any     M casts/s of the two instances (any: MIRT_CAST_ANY_HIT), with the feature rows
  trace_rays     mirt_trace_rays on the same rays (closest hit): what a ball of radius 0 costs as a ray
  advancement    conservative advancement as a caller writes it today: mirt_closest_points from the centre with R = inf, step the
                 centre by dist - r, until dist - r < 1e-4 or t >= the scene's diagonal or nothing is near, at most --max-steps
                 launches, every launch over all rows still moving (compacted with torch); its launch count and the share of
                 rows whose t agrees with the cast's to 1e-3
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up, repeated
--repeats times (median, min, max); the advancement is timed once per repeat.  Prints one JSON line and, with --out, writes it.
"""
import sys

import torch

import bench_common as bc
from bench_common import DEV, INF, m


def primitive_size(raw):
    """About a primitive: the median of the spheres' radii and of half the triangles' longest edges."""
    sizes = []
    if raw.desc.num_spheres:
        xyzr = torch.empty((raw.desc.num_spheres, 4), dtype=torch.float32, device=DEV)
        m.get_spheres(raw, xyzr)
        sizes.append(xyzr[:, 3])
    if raw.desc.num_triangles:
        v = torch.empty((raw.desc.num_triangles, 9), dtype=torch.float32, device=DEV)
        m.get_triangles(raw, v)
        a, b, c = v[:, 0:3], v[:, 3:6], v[:, 6:9]
        edges = torch.stack([(b - a).norm(dim=1), (c - a).norm(dim=1), (c - b).norm(dim=1)], dim=1)
        sizes.append(0.5 * edges.max(dim=1).values)
    torch.cuda.synchronize()
    return float(torch.cat(sizes).median())


def advance(raw, casts, tmax, max_steps):
    """Conservative advancement: (t per row, -1 for none; launches)."""
    n = casts.shape[0]
    o = casts[:, 0:3]
    d = casts[:, 4:7] / casts[:, 4:7].norm(dim=1, keepdim=True)
    r = casts[:, 7]
    t = torch.zeros(n, dtype=torch.float32, device=DEV)
    out = torch.full((n,), -1.0, dtype=torch.float32, device=DEV)
    moving = torch.arange(n, device=DEV)
    launches = 0
    while moving.numel() and launches < max_steps:
        rows = m.pack_points(o[moving] + d[moving] * t[moving, None], INF)
        hits = torch.empty((moving.numel(), 6), dtype=torch.int32, device=DEV)
        m.closest_points(raw, rows, hits)
        launches += 1
        dist, kind, _, _ = m.unpack_hits(hits)
        gap = dist - r[moving]
        touch = (kind != 0) & (gap < 1e-4)
        out[moving[touch]] = t[moving[touch]]
        go = (kind != 0) & ~touch
        t[moving[go]] += gap[go]
        moving = moving[go & (t[moving] < tmax)]
    return out, launches


def surface_points(raw, w, h, count):
    """`count` first-hit points of the camera rays and their normals, picked by one seeded generator, and as many random directions."""
    rays = bc.camera(raw, w, h)
    hits = torch.empty((rays.shape[0], 6), dtype=torch.int32, device=DEV)
    m.trace_rays(raw, rays, hits)
    t, kind, _, nn = m.unpack_hits(hits)
    sel = torch.nonzero(kind != 0).squeeze(1)
    d = rays[sel, 4:7]
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    p = rays[sel, 0:3] + t[sel, None] * d
    g = torch.Generator(device=DEV).manual_seed(1234)
    pick = torch.randint(0, p.shape[0], (count,), generator=g, device=DEV)
    return p[pick], nn[sel][pick], torch.randn((count, 3), generator=g, device=DEV)


def measure(raw, points, radius, diagonal, a):
    p, nn, dirs = points
    n = p.shape[0]
    casts = m.pack_casts(p + nn * (1.5 * radius + 1e-3 * diagonal), dirs, INF, radius)
    rays = casts
    hits = torch.empty((n, 6), dtype=torch.int32, device=DEV)
    feat = torch.empty((n, 8), dtype=torch.float32, device=DEV)
    timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, "mcasts_per_s", 1e-6)
    res = dict(radius=round(radius, 6))
    res["any"] = timed(lambda: m.cast_spheres(raw, casts, hits, feat, any_hit=True))
    res["first"] = timed(lambda: m.cast_spheres(raw, casts, hits, feat))
    t, kind, _, _ = m.unpack_hits(hits)
    res["hit_share"] = round(float((kind != 0).float().mean()), 4)
    res["touching_at_start"] = round(float(((kind != 0) & (t == 0)).float().mean()), 4)
    ray_hits = torch.empty_like(hits)
    res["trace_rays"] = timed(lambda: m.trace_rays(raw, rays, ray_hits))
    res["first_over_trace_rays"] = round(res["first"]["mcasts_per_s"] / res["trace_rays"]["mcasts_per_s"], 3)
    sub = casts[:a.advance_rays].contiguous()
    rates, launches = [], 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.repeats):
        e0.record()
        ta, launches = advance(raw, sub, diagonal, a.max_steps)
        e1.record()
        torch.cuda.synchronize()
        rates.append(sub.shape[0] / (e0.elapsed_time(e1) * 1e-3) * 1e-6)
    rates.sort()
    both = (ta >= 0) & (kind[:sub.shape[0]] != 0)
    res["advancement"] = dict(mcasts_per_s=round(rates[len(rates) // 2], 3), min=round(rates[0], 3), max=round(rates[-1], 3), rows=sub.shape[0],
                              launches=launches, capped=launches >= a.max_steps,
                              agree_to_1e_3=round(float(((ta - t[:sub.shape[0]]).abs() < 1e-3)[both].float().mean()), 4) if bool(both.any()) else None)
    res["first_over_advancement"] = round(res["first"]["mcasts_per_s"] / res["advancement"]["mcasts_per_s"], 1)
    return res


def main():
    ap = bc.parser()
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--advance-rays", type=int, default=1 << 18)
    ap.add_argument("--max-steps", type=int, default=64, help="launches after which the advancement gives up")
    ap.add_argument("--only", default=None, help="one scene, e.g. tenthousand")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=None, help="also write the JSON here, e.g. profiles/spherecast_bench.json")
    a = ap.parse_args()
    result = dict(metric="spherecast_mcasts_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), rays=a.rays, max_steps=a.max_steps,
                  label=a.label, results={})
    for name in ("tenthousand", "redchair", "synthetic"):
        if a.only not in (None, name):
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if name == "synthetic" else m.parseInput(bc.scene_path(name))
        raw = bc.built(stl)
        _, diagonal = bc.box_diagonal(raw)
        prim = primitive_size(raw)
        points = surface_points(raw, a.width, a.height, a.rays)
        result["results"][name] = dict(primitives=int(raw.desc.num_prims), primitive_size=round(prim, 6), diagonal=round(diagonal, 4))
        for tag, radius in (("r0", 0.0), ("r1", prim), ("r10", 10.0 * prim)):
            result["results"][name][tag] = measure(raw, points, radius, diagonal, a)
            print(f"{name}/{tag} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

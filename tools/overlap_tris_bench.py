#!/usr/bin/env python3
"""Throughput of the triangle overlap queries (mirt_overlap_triangles, mirt_triangle_list): the count, the any-count, the fill and the
whole list, beside the broad phase a caller had before them and a torch brute force.

    python tools/overlap_tris_bench.py [--only NAME] [--rows 1000000] [--no-brute-force] [--label TEXT] [--out profiles/overlap_tris_bench.json]

Workloads:
  redchair      scenes/redchair.txt with its own triangles as rows (a mesh against itself)
  tenthousand   scenes/tenthousand.txt with --rows random triangles: a uniform in the scene's box, b and c within 2 % of its diagonal
  synthetic     the synthetic scene (1 M spheres and 1 M triangles) with its own triangles as rows
Per workload, in M rows per second:
  count, any        overlap_triangles, and with any=True
  fill              triangle_list into an array of exactly the total; mwords_per_s beside it
  triangle_lists    the wrapper as a caller uses it: count, scan, the host read of the total, the allocation, fill
  broad_count       count_overlaps on the rows' bounding boxes: the broad phase
  rejected          the share of the broad phase's candidates (overlap_lists of the boxes) that the exact test does not admit
  missed_by_broad   the share of the exact test's words that the broad phase does not list
  mean_list, max_list, non_empty
brute force  on tenthousand (spheres and planes only), --brute-rows rows against every sphere and plane in torch by the header's
             operations; same_counts is the share of rows whose count equals the kernel's (torch may contract or reorder a sum).
Timed with HIP events over back-to-back repetitions totalling at least --min-seconds (0.3) of device time after a warm-up, repeated
--repeats (3) times: median, min, max.  Prints one JSON line and writes it to --out.  No timing is asserted anywhere.
"""
import os
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, m


def random_triangles(box, diag, n, seed=1234):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lo = torch.tensor(box[0:3], dtype=torch.float32, device=DEV)
    hi = torch.tensor(box[3:6], dtype=torch.float32, device=DEV)
    a = lo + (hi - lo) * torch.rand((n, 3), generator=g, device=DEV)
    b = a + 0.02 * diag * (2 * torch.rand((n, 3), generator=g, device=DEV) - 1)
    c = a + 0.02 * diag * (2 * torch.rand((n, 3), generator=g, device=DEV) - 1)
    return torch.cat([a, b, c], dim=1).contiguous()


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_on_triangle(ub, uc, q):
    """mirt_closest.h's closest point of the triangle (0, ub, uc) to q, region by region, every region computed and the first chosen."""
    d1, d2 = dot(ub, q), dot(uc, q)
    bp = q - ub
    d3, d4 = dot(ub, bp), dot(uc, bp)
    cp = q - uc
    d5, d6 = dot(ub, cp), dot(uc, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e, f = d4 - d3, d5 - d6
    den = 1.0 / ((va + vb) + vc)
    P = ub * (vb * den)[..., None] + uc * (vc * den)[..., None]
    pick = lambda cond, val, rest: torch.where(cond[..., None], val, rest)
    P = pick((va <= 0) & (e >= 0) & (f >= 0), ub + (uc - ub) * (e / (e + f))[..., None], P)
    P = pick((vb <= 0) & (d2 >= 0) & (d6 <= 0), uc * (d2 / (d2 - d6))[..., None], P)
    P = pick((d6 >= 0) & (d5 <= d6), uc.expand_as(P), P)
    P = pick((vc <= 0) & (d1 >= 0) & (d3 <= 0), ub * (d1 / (d1 - d3))[..., None], P)
    P = pick((d3 >= 0) & (d4 <= d3), ub.expand_as(P), P)
    return pick((d1 <= 0) & (d2 <= 0), torch.zeros_like(P), P)


class BruteForce:
    """The counts of `rows` against every sphere (xyzr) and plane (unit normal, point) in torch, `chunk` rows at a time."""

    def __init__(self, xyzr, planes, rows, chunk):
        self.c, self.r, self.planes, self.rows, self.chunk = xyzr[:, 0:3].contiguous(), xyzr[:, 3].contiguous(), planes, rows, chunk

    def __call__(self):
        out = []
        for i in range(0, self.rows.shape[0], self.chunk):
            t = self.rows[i:i + self.chunk]
            a, b, c = t[:, None, 0:3], t[:, None, 3:6], t[:, None, 6:9]
            lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)
            ub, uc = b - a, c - a
            ctr, r = self.c[None], self.r[None]
            near = ((ctr - r[..., None] <= hi) & (ctr + r[..., None] >= lo)).all(dim=2)
            C = ctr - a
            dn = (C - closest_on_triangle(ub, uc, C)).norm(dim=2)
            df = torch.maximum(torch.maximum(C.norm(dim=2), (ub - C).norm(dim=2)), (uc - C).norm(dim=2))
            count = (near & (dn <= r) & (df >= r)).sum(dim=1)
            for nor, point in self.planes:
                s = torch.stack([((v[:, 0] - point[None]) * nor[None]).sum(dim=1) for v in (a, b, c)])
                count = count + ((s.min(dim=0).values <= 0) & (s.max(dim=0).values >= 0))
            out.append(count)
        return torch.cat(out)


def row_keys(offsets, words):
    """row << 32 | word of every word of a list."""
    row = torch.repeat_interleave(torch.arange(offsets.shape[0] - 1, dtype=torch.int64, device=DEV), offsets[1:] - offsets[:-1])
    return (row << 32) | (words.to(torch.int64) & 0xffffffff)


def measure(raw, rows, a, brute=None):
    n = rows.shape[0]
    res = dict(rows=n, primitives=int(raw.desc.num_prims))
    timed = lambda fn: bc.timed(fn, n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    counts = m.overlap_triangles(raw, rows)
    offsets = m.list_offsets(raw, counts)
    total = int(offsets[-1])
    words = torch.empty(total, dtype=torch.int32, device=DEV)
    t = rows.reshape(n, 3, 3)
    boxes = m.pack_boxes(t.min(dim=1).values, t.max(dim=1).values)
    broad = m.count_overlaps(raw, boxes)
    broad_total = int(broad.to(torch.int64).sum())
    res["count"] = timed(lambda: m.overlap_triangles(raw, rows, counts))
    res["any"] = timed(lambda: m.overlap_triangles(raw, rows, counts, any=True))
    m.overlap_triangles(raw, rows, counts)
    res["fill"] = timed(lambda: m.triangle_list(raw, rows, offsets, words))
    res["fill"]["mwords_per_s"] = round(total / (res["fill"]["ms_per_call"] * 1e-3) * 1e-6, 1)
    res["triangle_lists"] = timed(lambda: m.triangle_lists(raw, rows))
    res["broad_count"] = timed(lambda: m.count_overlaps(raw, boxes, broad))
    lens = counts.to(torch.int64)
    res["total_words"], res["broad_candidates"] = total, broad_total
    # the two sets as row << 32 | word: what the broad phase lists and the exact test does not admit, and the other way round (a
    # touch at a vertex on the bounding box's face, which the box query decides by the rounding of the box's centre and half extent)
    exact, listed = (row_keys(o, w) for o, w in (m.triangle_lists(raw, rows), m.overlap_lists(raw, boxes)))
    res["rejected"] = round(1.0 - float(torch.isin(listed, exact).float().mean()) if listed.numel() else 0.0, 5)
    res["missed_by_broad"] = round(1.0 - float(torch.isin(exact, listed).float().mean()) if exact.numel() else 0.0, 5)
    res["mean_list"], res["max_list"] = round(total / n, 4), int(lens.max())
    res["non_empty"] = round(float((lens > 0).float().mean()), 5)
    res["broad_count_over_count"] = round(res["broad_count"]["mrows_per_s"] / res["count"]["mrows_per_s"], 3)
    if brute is not None:
        sub = bc.incoherent_rows(rows, a.brute_rows)
        bf = BruteForce(brute[0], brute[1], sub, a.brute_chunk)
        mine = m.overlap_triangles(raw, sub).to(torch.int64)
        res["brute_force"] = bc.timed(bf, sub.shape[0], a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
        res["brute_force"]["rows"] = sub.shape[0]
        res["brute_force"]["same_counts"] = round(float((bf() == mine).float().mean()), 6)
        res["count_over_brute_force"] = round(res["count"]["mrows_per_s"] / res["brute_force"]["mrows_per_s"], 1)
    return res


def main():
    ap = bc.parser()
    ap.set_defaults(repeats=3, min_seconds=0.3)
    ap.add_argument("--rows", type=int, default=1_000_000, help="random triangles of the tenthousand workload")
    ap.add_argument("--synthetic", type=int, default=1_000_000, help="spheres (and as many triangles) of the synthetic scene")
    ap.add_argument("--brute-rows", type=int, default=1 << 13)
    ap.add_argument("--brute-chunk", type=int, default=1 << 8)
    ap.add_argument("--only", default=None, help="one workload: redchair, tenthousand or synthetic")
    ap.add_argument("--no-brute-force", action="store_true", help="skip the torch brute force")
    ap.add_argument("--label", default=None, help="a note kept in the result, e.g. the build variant measured")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "overlap_tris_bench.json"))
    a = ap.parse_args()
    result = dict(metric="overlap_tris_mrows_per_s", device=torch.cuda.get_device_name(0), **bc.settings(a), label=a.label, results={})
    for name in ("redchair", "tenthousand", "synthetic"):
        if a.only not in (None, name):
            continue
        stl = m.syntheticScene(a.synthetic, a.synthetic) if name == "synthetic" else m.parseInput(bc.scene_path(name))
        raw = bc.built(stl)
        box, diag = bc.box_diagonal(raw)
        rows = random_triangles(box, diag, a.rows) if name == "tenthousand" else m.scene_triangle_rows(raw)
        brute = None
        if name == "tenthousand" and raw.desc.num_triangles == 0 and not a.no_brute_force:
            xyzr = torch.empty((raw.desc.num_spheres, 4), dtype=torch.float32, device=DEV)
            m.get_spheres(raw, xyzr)
            planes = [(torch.tensor(np.array(p["nor"]), device=DEV), torch.tensor(np.array(p["point"]), device=DEV)) for p in stl.array("planes")]
            brute = (xyzr, [(nor / nor.norm(), point) for nor, point in planes])
        result["results"][name] = measure(raw, rows, a, brute)
        print(f"{name} done", file=sys.stderr, flush=True)
        raw.close()
    out_dir = os.path.dirname(a.out)
    bc.emit(result, a.out if os.path.isdir(out_dir) else None, indent=1)


if __name__ == "__main__":
    main()

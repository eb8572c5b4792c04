#!/usr/bin/env python3
"""Throughput of the hemisphere-visibility query (mirt_hemisphere_visibility) against the composition it replaces.

    python tools/visibility_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--fused-only] [--out profiles/visibility_bench.json]

Workloads, each with K = 8 and K = 64 directions (cosine_directions, one rotation per row) and with a radius of 5 % of the scene
box's diagonal and of +inf; a workload's name is ROWS/kK/near or ROWS/kK/inf:
  tenthousand   the first-hit points of the 1920 x 1080 camera rays of scenes/tenthousand.txt (spp 0)
  redchair      ... of scenes/redchair.txt
  incoherent    4 M rows drawn at random (seeded) from the hit rows of `tenthousand`: neighbouring lanes, far-apart points
fused        one mirt_hemisphere_visibility call over the rows, with the mask.
composition  the same answer from the calls that existed before: the n x K rays built in torch from the header's formulas (rays of
             rows that are no hit get tmax 0, which mirt_trace_rays answers without a walk), one mirt_trace_rays(any_hit) over
             them, and the sum and the mask reduced in torch.
Both are timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up,
repeated --repeats times (median, min, max).  The composition's mask is compared with the fused one once per workload and the
number of differing (row, direction) pairs reported: torch rounds a few of the operations its own way, so a ray that grazes a
surface may fall on the other side.  Prints one JSON line and, with --out, writes it to a file.
"""
import math
import sys

import torch

import bench_common as bc
from bench_common import DEV, INF, m


class Composition:
    """The hemisphere visibility of feature rows F from trace_rays and torch."""

    def __init__(self, raw, F, dirs, rot, radius):
        self.raw, self.F, self.dirs, self.rot, self.radius = raw, F, dirs, rot, radius
        n, k = F.shape[0], dirs.shape[0]
        self.rays = torch.zeros((n, k, 8), dtype=torch.float32, device=DEV)
        self.hits = torch.empty((n * k, 6), dtype=torch.int32, device=DEV)
        self.shift = torch.arange(k, dtype=torch.int64, device=DEV)

    def __call__(self):
        F, dirs, rot = self.F, self.dirs, self.rot
        P, ng, hit = F[:, 0:3], F[:, 4:7], F[:, 3] != 0
        mag = torch.sqrt((ng * ng).sum(dim=-1, keepdim=True))
        N = torch.where(mag < 1e-6, torch.zeros_like(ng), ng * (1.0 / mag))
        o = P + ng * 0.001
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        s = torch.copysign(torch.ones_like(nz), nz)
        a = -1.0 / (s + nz)
        b = nx * ny * a
        T = torch.stack([1.0 + s * nx * nx * a, s * b, -s * nx], dim=1)
        B = torch.stack([b, s + ny * ny * a, -ny], dim=1)
        lx, ly, lz, w = dirs[None, :, 0], dirs[None, :, 1], dirs[None, :, 2], dirs[None, :, 3]
        c, r = rot[:, 0:1], rot[:, 1:2]
        x = c * lx - r * ly
        y = r * lx + c * ly
        d = T[:, None, :] * x[..., None] + B[:, None, :] * y[..., None] + N[:, None, :] * lz[..., None]
        rays = self.rays
        rays[:, :, 0:3] = o[:, None, :]
        rays[:, :, 3] = torch.where(hit, self.radius, 0.0)[:, None]
        rays[:, :, 4:7] = d
        m.trace_rays(self.raw, rays.view(-1, 8), self.hits, any_hit=True)
        visible = hit[:, None] & (self.hits[:, 1].view(-1, dirs.shape[0]) == 0)
        u = d / torch.sqrt((d * d).sum(dim=-1, keepdim=True))
        e = torch.where(visible[..., None], torch.cat([u * w[..., None], w.expand(F.shape[0], -1)[..., None]], dim=-1), 0.0)
        out = e.sum(dim=1)
        mask = (visible.to(torch.int64) << self.shift[None, :]).sum(dim=1)
        return out, mask


def measure(raw, F, k, radius, a):
    n = F.shape[0]
    dirs, rot = m.cosine_directions(k, DEV), m.rotations(n, 77, DEV)
    out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
    mask = torch.empty(n, dtype=torch.int64, device=DEV)
    hit = F[:, 3] != 0
    rays_traced = int(hit.sum()) * k
    res = dict(rows=n, directions=k, radius=radius if math.isfinite(radius) else "inf", hit_fraction=round(float(hit.float().mean()), 4), rays=rays_traced)
    res["fused"] = bc.timed(lambda: m.hemisphere_visibility(raw, F, dirs, out, mask, rot, radius), n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    res["fused"]["grays_per_s"] = round(res["fused"]["mrows_per_s"] * 1e-3 * rays_traced / n, 4)
    bit = ((mask[:, None] >> torch.arange(k, dtype=torch.int64, device=DEV)[None, :]) & 1).bool()
    res["visible_fraction_of_rays"] = round(int(bit[hit].sum()) / max(1, rays_traced), 4)
    res["mean_visible_weight_of_hit_rows"] = round(float(out[hit, 3].mean()), 4)
    if a.fused_only:
        return res
    comp = Composition(raw, F, dirs, rot, radius)
    c_out, c_mask = comp()
    torch.cuda.synchronize()
    pairs = (((c_mask ^ mask)[:, None] >> comp.shift[None, :]) & 1).bool()
    res["mask_pairs"] = n * k
    res["mask_pairs_differing"] = int(pairs.sum())
    res["masks_agree_on_every_pair"] = res["mask_pairs_differing"] == 0
    assert res["mask_pairs_differing"] <= 1e-4 * n * k, "the composition's mask differs from the fused call's on more than grazing rays"
    same = (c_mask == mask) & hit
    res["max_abs_difference_of_the_sums"] = float((c_out[same] - out[same]).abs().max())      # (torch's sum has an order of its own)
    del c_out, c_mask, pairs
    res["composition"] = bc.timed(comp, n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    res["composition"]["grays_per_s"] = round(res["composition"]["mrows_per_s"] * 1e-3 * rays_traced / n, 4)
    res["fused_over_composition"] = round(res["fused"]["mrows_per_s"] / res["composition"]["mrows_per_s"], 3)
    return res


def main():
    ap = bc.parser()
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand/k64/near (for a counter pass)")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here, e.g. profiles/visibility_bench.json")
    a = ap.parse_args()
    w, h = a.width, a.height
    result = dict(metric="hemisphere_visibility_mrows_per_s", **bc.settings(a), results={})
    for name in ("tenthousand", "redchair"):
        sets = [name] + (["incoherent"] if name == "tenthousand" else [])
        wanted = [(rows, k, tag) for rows in sets for k in (8, 64) for tag in ("near", "inf") if a.only in (None, f"{rows}/k{k}/{tag}")]
        if not wanted:
            continue
        raw = bc.built(m.parseInput(bc.scene_path(name)))
        near = 0.05 * bc.box_diagonal(raw)[1]
        F = bc.first_hit_features(raw, w, h)
        incoherent = bc.incoherent_rows(F[F[:, 3] != 0], a.incoherent) if any(rows != name for rows, _, _ in wanted) else None
        for rows, k, tag in wanted:
            rows_f = F if rows == name else incoherent
            result["results"][f"{rows}/k{k}/{tag}"] = measure(raw, rows_f, k, near if tag == "near" else INF, a)
            print(f"{rows}/k{k}/{tag} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

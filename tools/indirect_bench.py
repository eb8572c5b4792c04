#!/usr/bin/env python3
"""Throughput of the indirect-light query (mirt_indirect_light) against the composition it replaces.

    python tools/indirect_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--fused-only] [--out profiles/indirect_bench.json]

Workloads, each with K = 8 and K = 64 directions (cosine_directions, one rotation per row) and with a radius of 5 % of the scene
box's diagonal and of +inf; a workload's name is ROWS/kK/near or ROWS/kK/inf:
  tenthousand   the first-hit points of the 1920 x 1080 camera rays of scenes/tenthousand.txt (spp 0)
  redchair      ... of scenes/redchair.txt
fused        one mirt_indirect_light call over the rows, with the mask.
composition  the same answer from the calls that existed before: the n x K rays built in torch from the header's formulas (rays of
             rows that are no hit get tmax 0, which mirt_trace_rays answers without a walk), one closest-hit mirt_trace_rays over
             them, mirt_hit_features, mirt_direct_light with MIRT_LIGHT_RAW on the n x K rows, the materials gathered by
             (kind, id) and the weighted sum and the mask reduced in torch -- in chunks of rows, so that the n x K intermediates of
             a chunk stay below --chunk-rays rows.
Both are timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up,
repeated --repeats times (median, min, max).  The composition's mask is compared with the fused one once per workload and the
number of differing (row, direction) pairs reported: torch rounds a few of the operations its own way, so a ray that grazes a
surface may fall on the other side.  Prints one JSON line and, with --out, writes it to a file.
"""
import math
import sys

import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, INF, m


def material_table(raw):
    """rho = (1 - shininess)(1 - trans) colour of every primitive and plane, float32 [Ns + Nt + Np, 3], and the offsets of the
    three kinds in it indexed by MirtHit's kind."""
    ns, nt = raw.desc.num_spheres, raw.desc.num_triangles
    mats = torch.zeros((ns + nt, 11), dtype=torch.float32, device=DEV)
    if ns:
        m.get_sphere_materials(raw, mats[:ns])
    if nt:
        m.get_triangle_materials(raw, mats[ns:])
    planes = raw.planes()
    pm = torch.from_numpy(np.ascontiguousarray(planes["mat"]).view(np.float32).reshape(-1, 11).copy()).to(DEV)
    mats = torch.cat([mats, pm])
    rho = (1.0 - mats[:, 3:6]) * (1.0 - mats[:, 6:9]) * mats[:, 0:3]
    offsets = torch.tensor([0, 0, ns, ns + nt], dtype=torch.int64, device=DEV)
    return rho.contiguous(), offsets


class Composition:
    """The indirect light of feature rows F from trace_rays, hit_features, direct_light and torch."""

    def __init__(self, raw, F, dirs, rot, radius, chunk_rays):
        self.raw, self.F, self.dirs, self.rot, self.radius = raw, F, dirs, rot, radius
        n, k = F.shape[0], dirs.shape[0]
        self.chunk = max(1, min(n, chunk_rays // k))
        c = self.chunk
        self.rays = torch.zeros((c, k, 8), dtype=torch.float32, device=DEV)
        self.hits = torch.empty((c * k, 6), dtype=torch.int32, device=DEV)
        self.rows = torch.empty((c * k, 8), dtype=torch.float32, device=DEV)
        self.light = torch.empty((c * k, 4), dtype=torch.float32, device=DEV)
        self.shift = torch.arange(k, dtype=torch.int64, device=DEV)
        self.rho, self.offsets = material_table(raw)
        self.out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
        self.mask = torch.empty(n, dtype=torch.int64, device=DEV)

    def part(self, a, b):
        F, dirs, rot = self.F[a:b], self.dirs, self.rot[a:b]
        c, k = b - a, dirs.shape[0]
        P, ng, hit = F[:, 0:3], F[:, 4:7], F[:, 3] != 0
        mag = torch.sqrt((ng * ng).sum(dim=-1, keepdim=True))
        N = torch.where(mag < 1e-6, torch.zeros_like(ng), ng * (1.0 / mag))
        o = P + ng * 0.001
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        s = torch.copysign(torch.ones_like(nz), nz)
        aa = -1.0 / (s + nz)
        bb = nx * ny * aa
        T = torch.stack([1.0 + s * nx * nx * aa, s * bb, -s * nx], dim=1)
        B = torch.stack([bb, s + ny * ny * aa, -ny], dim=1)
        lx, ly, lz, w = dirs[None, :, 0], dirs[None, :, 1], dirs[None, :, 2], dirs[None, :, 3]
        cs, sn = rot[:, 0:1], rot[:, 1:2]
        x = cs * lx - sn * ly
        y = sn * lx + cs * ly
        d = T[:, None, :] * x[..., None] + B[:, None, :] * y[..., None] + N[:, None, :] * lz[..., None]
        rays = self.rays[:c]
        rays[:, :, 0:3] = o[:, None, :]
        rays[:, :, 3] = torch.where(hit, self.radius, 0.0)[:, None]
        rays[:, :, 4:7] = d
        hits, rows, light = self.hits[:c * k], self.rows[:c * k], self.light[:c * k]
        m.trace_rays(self.raw, rays.view(-1, 8), hits)
        m.hit_features(self.raw, rays.view(-1, 8), hits, rows)
        m.direct_light(self.raw, rows, light, raw_units=True)
        kind, ident = hits[:, 1].to(torch.int64), hits[:, 2].to(torch.int64)
        found = (kind != 0).view(c, k) & hit[:, None]
        rho = self.rho[self.offsets[kind] + ident].view(c, k, 3)
        term = torch.where(found[..., None], rho * light[:, 0:3].view(c, k, 3) * w[..., None], 0.0)
        free = torch.where(~found & hit[:, None], w.expand(c, -1), 0.0)
        self.out[a:b, 0:3] = term.sum(dim=1)
        self.out[a:b, 3] = free.sum(dim=1)
        self.mask[a:b] = (found.to(torch.int64) << self.shift[None, :]).sum(dim=1)

    def __call__(self):
        n = self.F.shape[0]
        for a in range(0, n, self.chunk):
            self.part(a, min(n, a + self.chunk))
        return self.out, self.mask


def measure(raw, F, k, radius, a):
    n = F.shape[0]
    dirs, rot = m.cosine_directions(k, DEV), m.rotations(n, 77, DEV)
    out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
    mask = torch.empty(n, dtype=torch.int64, device=DEV)
    hit = F[:, 3] != 0
    rays_traced = int(hit.sum()) * k
    suns, bulbs = raw.lights()
    res = dict(rows=n, directions=k, radius=radius if math.isfinite(radius) else "inf", hit_fraction=round(float(hit.float().mean()), 4),
               gather_rays=rays_traced, lights=len(suns) + len(bulbs))
    res["fused"] = bc.timed(lambda: m.indirect_light(raw, F, dirs, out, mask, rot, radius), n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    res["fused"]["gather_grays_per_s"] = round(res["fused"]["mrows_per_s"] * 1e-3 * rays_traced / n, 4)
    bit = ((mask[:, None] >> torch.arange(k, dtype=torch.int64, device=DEV)[None, :]) & 1).bool()
    res["hit_fraction_of_gather_rays"] = round(int(bit[hit].sum()) / max(1, rays_traced), 4)
    res["mean_rgb_of_hit_rows"] = [round(float(v), 5) for v in out[hit, 0:3].mean(dim=0)]
    if a.fused_only:
        return res
    comp = Composition(raw, F, dirs, rot, radius, a.chunk_rays)
    c_out, c_mask = comp()
    torch.cuda.synchronize()
    pairs = (((c_mask ^ mask)[:, None] >> comp.shift[None, :]) & 1).bool()
    res["chunk_rows"] = comp.chunk
    res["mask_pairs"] = n * k
    res["mask_pairs_differing"] = int(pairs.sum())
    res["masks_differing"] = int((c_mask != mask).sum())
    assert res["mask_pairs_differing"] <= 1e-4 * n * k, "the composition's mask differs from the fused call's on more than grazing rays"
    same = (c_mask == mask) & hit
    res["max_abs_difference_of_the_sums"] = float((c_out[same] - out[same]).abs().max())      # (torch's sum has an order of its own)
    del pairs
    res["composition"] = bc.timed(comp, n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    res["composition"]["gather_grays_per_s"] = round(res["composition"]["mrows_per_s"] * 1e-3 * rays_traced / n, 4)
    res["fused_over_composition"] = round(res["fused"]["mrows_per_s"] / res["composition"]["mrows_per_s"], 3)
    return res


def main():
    ap = bc.parser()
    ap.add_argument("--chunk-rays", type=int, default=1 << 24, help="most (row, direction) pairs the composition holds at a time")
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand/k64/near (for a counter pass)")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here, e.g. profiles/indirect_bench.json")
    a = ap.parse_args()
    w, h = a.width, a.height
    result = dict(metric="indirect_light_mrows_per_s", **bc.settings(a), results={})
    for name in ("tenthousand", "redchair"):
        wanted = [(k, tag) for k in (8, 64) for tag in ("near", "inf") if a.only in (None, f"{name}/k{k}/{tag}")]
        if not wanted:
            continue
        raw = bc.built(m.parseInput(bc.scene_path(name)))
        near = 0.05 * bc.box_diagonal(raw)[1]
        F = bc.first_hit_features(raw, w, h)
        for k, tag in wanted:
            result["results"][f"{name}/k{k}/{tag}"] = measure(raw, F, k, near if tag == "near" else INF, a)
            print(f"{name}/k{k}/{tag} done", file=sys.stderr, flush=True)
        raw.close()
    bc.emit(result, a.out, indent=1)


if __name__ == "__main__":
    main()

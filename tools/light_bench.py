#!/usr/bin/env python3
"""Throughput of the direct-light query (mirt_direct_light) against the composition it replaces.

    python tools/light_bench.py [--repeats 5] [--min-seconds 0.5] [--only NAME] [--fused-only]

Workloads, each with the scene's own lights and with 16 bulbs added:
  tenthousand   the first-hit points of the 1920 x 1080 camera rays of scenes/tenthousand.txt (spp 0)
  redchair      ... of scenes/redchair.txt
  incoherent    4 M rows drawn at random (seeded) from the hit rows of `tenthousand`: neighbouring lanes, far-apart points
fused        one mirt_direct_light call over the rows, with the mask.
composition  the same answer from the calls that existed before: the n x L shadow rays built in torch (rays of rows that are no
             hit, or of lights the normal faces away from, get tmax 0, which mirt_trace_rays answers without a walk), one
             mirt_trace_rays(any_hit) over them, and the terms and the mask reduced in torch.
Both are timed with HIP events over back-to-back repetitions totalling at least --min-seconds of device time after a warm-up,
repeated --repeats times (median, min, max).  The composition's mask is compared with the fused one once per workload: torch
rounds the facing test's normalisations its own way, so a pair may differ where |cos| < 1e-6 and nowhere else (asserted; the
counts are reported).  Prints one JSON line.
"""
import numpy as np
import torch

import bench_common as bc
from bench_common import DEV, INF, m


def _unit(v):
    return v / torch.sqrt((v * v).sum(dim=-1, keepdim=True))


class Composition:
    """The direct light of feature rows F from trace_rays and torch."""

    def __init__(self, raw, F):
        suns, bulbs = raw.lights()
        self.raw, self.F, self.ns, self.L = raw, F, len(suns), len(suns) + len(bulbs)
        self.sun_dir = torch.from_numpy(np.ascontiguousarray(suns["v"])).to(DEV)
        self.bulb_pos = torch.from_numpy(np.ascontiguousarray(bulbs["v"])).to(DEV)
        self.colour = torch.from_numpy(np.concatenate([suns["color"], bulbs["color"]]).astype(np.float32)).to(DEV)
        self.expose = float(raw.shading().expose)
        n = F.shape[0]
        self.rays = torch.zeros((n, self.L, 8), dtype=torch.float32, device=DEV)
        self.hits = torch.empty((n * self.L, 6), dtype=torch.int32, device=DEV)
        self.shift = torch.arange(self.L, dtype=torch.int64, device=DEV)

    def __call__(self):
        F, ns = self.F, self.ns
        P, ng, hit = F[:, 0:3], F[:, 4:7], F[:, 3] != 0
        N = _unit(ng)
        o = P + ng * 0.001
        bd = self.bulb_pos[None, :, :] - P[:, None, :]
        tl = torch.sqrt((bd * bd).sum(dim=-1))
        lam = torch.cat([N @ _unit(self.sun_dir).T, (N[:, None, :] * (bd / tl[..., None])).sum(dim=-1)], dim=1)
        need = hit[:, None] & (lam > 0)
        tmax = torch.cat([torch.full((F.shape[0], ns), INF, device=DEV), tl], dim=1)
        rays = self.rays
        rays[:, :, 0:3] = o[:, None, :]
        rays[:, :, 3] = torch.where(need, tmax, torch.zeros_like(tmax))
        rays[:, :ns, 4:7] = self.sun_dir[None, :, :]
        rays[:, ns:, 4:7] = bd
        m.trace_rays(self.raw, rays.view(-1, 8), self.hits, any_hit=True)
        lit = need & (self.hits[:, 1].view(-1, self.L) == 0)
        c = self.colour[None, :, :] * lam[..., None]
        e = c if self.expose == INF else 1.0 - torch.exp(-self.expose * c)
        e = torch.cat([e[:, :ns], e[:, ns:] / (tl * tl)[..., None]], dim=1)
        rgb = torch.where(lit[..., None], e, torch.zeros_like(e)).sum(dim=1)
        out = torch.cat([rgb, hit[:, None].to(torch.float32)], dim=1)
        mask = (lit.to(torch.int64) << self.shift[None, :]).sum(dim=1)
        self.lam, self.need = lam, need
        return out, mask


def measure(raw, F, a):
    n = F.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=DEV)
    mask = torch.empty(n, dtype=torch.int64, device=DEV)
    suns, bulbs = raw.lights()
    L = len(suns) + len(bulbs)
    res = dict(rows=n, lights=L, hit_fraction=round(float((F[:, 3] != 0).float().mean()), 4))
    res["fused"] = bc.timed(lambda: m.direct_light(raw, F, out, mask), n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    if a.fused_only:
        return res
    comp = Composition(raw, F)
    c_out, c_mask = comp()
    torch.cuda.synchronize()
    # the masks agree, but for pairs whose facing test torch's own rounding of the normalisations decides
    diff = (c_mask ^ mask)
    pairs = ((diff[:, None] >> comp.shift[None, :]) & 1).bool()
    grazing = comp.lam.abs() < 1e-6
    res["mask_pairs"] = n * L
    res["mask_pairs_differing"] = int(pairs.sum())
    res["mask_pairs_differing_off_grazing_incidence"] = int((pairs & ~grazing).sum())
    assert res["mask_pairs_differing_off_grazing_incidence"] == 0, "the composition's mask differs from the fused call's beyond a grazing facing test"
    same = diff == 0
    res["max_abs_colour_difference"] = float((c_out[same] - out[same]).abs().max())      # (torch's exp is not the library's)
    walked = int(comp.need.sum())
    res["shadow_rays"] = walked
    res["lit_fraction_of_shadow_rays"] = round(int(((mask[:, None] >> comp.shift[None, :]) & 1).sum()) / max(1, walked), 4)
    res["fused"]["gshadow_rays_per_s"] = round(res["fused"]["mrows_per_s"] * 1e-3 * walked / n, 4)
    res["composition"] = bc.timed(comp, n, a.repeats, a.min_seconds, "mrows_per_s", 1e-6)
    res["composition"]["gshadow_rays_per_s"] = round(res["composition"]["mrows_per_s"] * 1e-3 * walked / n, 4)
    res["fused_over_composition"] = round(res["fused"]["mrows_per_s"] / res["composition"]["mrows_per_s"], 3)
    return res


def added_bulbs(F, count=16, seed=99):
    """`count` bulb lines spread over the box that holds the middle 90 % of the hit points per axis (a floor plane's horizon is far
    away), lifted into its upper half."""
    P = F[F[:, 3] != 0][:, 0:3]
    P = P[:: max(1, P.shape[0] // 100000)]
    lo, hi = torch.quantile(P, 0.05, dim=0).cpu().numpy(), torch.quantile(P, 0.95, dim=0).cpu().numpy()
    rng = np.random.default_rng(seed)
    pts = lo + (hi - lo) * rng.random((count, 3))
    pts[:, 1] = lo[1] + (hi[1] - lo[1]) * (0.5 + 0.5 * rng.random(count))
    return "\ncolor 1 1 1\n" + "".join("bulb %.5f %.5f %.5f\n" % tuple(p) for p in pts)


def workloads(name, suffix):
    return [name + suffix] + (["incoherent" + suffix] if name == "tenthousand" else [])


def main():
    ap = bc.parser()
    ap.add_argument("--incoherent", type=int, default=4 << 20)
    ap.add_argument("--only", default=None, help="one workload, e.g. tenthousand+16 (for a counter pass)")
    ap.add_argument("--fused-only", action="store_true")
    a = ap.parse_args()
    w, h = a.width, a.height
    out = dict(metric="direct_light_mrows_per_s", **bc.settings(a), results={})
    extra = {}
    for name in ("tenthousand", "redchair"):
        text = open(bc.scene_path(name)).read()
        for suffix in ("", "+16"):
            wanted = [k for k in workloads(name, suffix) if a.only in (None, k)]
            later = not suffix and any(a.only in (None, k) for k in workloads(name, "+16"))      # (its hit points place the added bulbs)
            if not wanted and not later:
                continue
            raw = bc.built(m.parseText(text + (extra[name] if suffix else "")))
            _, _, F = m.direct_light_frame(raw, w, h, 0, want_mask=False)
            if not suffix:
                extra[name] = added_bulbs(F)
            if name + suffix in wanted:
                out["results"][name + suffix] = measure(raw, F, a)
            if "incoherent" + suffix in wanted:
                out["results"]["incoherent" + suffix] = measure(raw, bc.incoherent_rows(F[F[:, 3] != 0], a.incoherent), a)
            raw.close()
    bc.emit(out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Adaptive sampling (mirt_render_accumulate_pixels / mirt_select_pixels / mirt_finalize_counts) measured, DESIGN.md section 6e.

    python tools/adaptive_bench.py [--width 1920 --height 1080] [--repeats 5] [--min-seconds 0.5] [--reference-spp 4096] [--only i,ii,iv]

  (i)  sparse throughput: M samples/s of a call with a pixel list of 5 %, 25 % and 100 % of the frame at 16 samples per pixel,
       on scenes/tenthousand.txt and scenes/redchair.txt -- a fixed-seed random list and the list select_pixels makes from an
       8-spp frame (the threshold is the quantile of the frame's own variance estimate that gives the density) -- against the
       dense render_accumulate of the frame in the same process, alternating.  A timed window repeats the call until it has
       lasted --min-seconds, between two HIP events; --repeats windows each: median, min, max.
  (ii) end to end on redchair.txt: render_adaptive (min 8, step 8, cap 64) at two thresholds against uniform sampling at the
       samples per pixel that spend about as many samples, and at the cap: wall time (host clock, ends in a synchronise), total
       samples, mean squared error of the linear RGB mean against a --reference-spp accumulate of the same frame.
  (iv) the dense hand-out order survives: a dense 16-spp frame timed before and after a burst of sparse calls.
((iii), the headline through bench.py for two builds, needs two libraries: tools/ab.py.)  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402
from cuda_ray_tracer_amd import api  # noqa: E402

DEV = "cuda"
COUNT = 16


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def summary(v, digits=3):
    s = sorted(v)
    return dict(median=round(s[len(s) // 2], digits), min=round(s[0], digits), max=round(s[-1], digits))


def window_ms(fn, min_seconds):
    """Device ms per call of one timed window: fn repeated until the window has lasted min_seconds, between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    e0.record()
    while True:
        fn()
        n += 1
        if n % 4 == 0 or n == 1:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def load(name):
    stl = m.parseInput(os.path.join(ROOT, "scenes", name + ".txt"))
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    return stl, raw


def variance_estimate(acc, asq, n):
    """The e of mirt_select_pixels, in torch float32 (used only to pick thresholds)."""
    nf = float(n)
    mean, q = acc.view(-1, 4)[:, :3] / nf, asq.view(-1, 4)[:, :3] / nf
    v = torch.clamp(torch.nan_to_num(q - mean * mean, nan=0.0), min=0.0)
    return (v / (nf - 1.0)).max(dim=1).values


def selected_list(raw, w, h, density):
    """The list select_pixels makes from an 8-spp frame at the threshold that selects about `density` of it."""
    n = w * h
    acc, asq = torch.zeros(4 * n, device=DEV), torch.zeros(4 * n, device=DEV)
    cn = torch.zeros(n, dtype=torch.int32, device=DEV)
    m.render_accumulate_pixels(raw, acc, w, h, 0, 8, None, asq, cn)
    if density >= 1.0:
        thr = -1.0
    else:
        thr = float(torch.quantile(variance_estimate(acc, asq, 8)[torch.randperm(n, device=DEV)[:1_000_000]], 1.0 - density))
    out, num = torch.empty(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    m.select_pixels(acc, asq, cn, w, h, 4, 4096, thr, out, num)
    k = int(num.item())
    return out[:k].clone(), thr


def sparse_throughput(a):
    res = {}
    for name in ("tenthousand", "redchair"):
        stl, raw = load(name)
        w, h = a.width, a.height
        n = w * h
        acc = torch.zeros(4 * n, device=DEV)
        dense = lambda: m.render_accumulate(acc, w, h, 8, COUNT, raw)      # noqa: E731
        for _ in range(3):
            dense()      # warm-up: workspaces, tables, the measured hand-out order
        scene = {}
        g = torch.Generator(device=DEV).manual_seed(1234)
        for density in (0.05, 0.25, 1.0):
            lists = {"random": torch.randperm(n, device=DEV, generator=g)[:int(round(density * n))].to(torch.int32).contiguous()}
            lists["selected"], thr = selected_list(raw, w, h, density)
            for kind, lst in lists.items():
                k = int(lst.shape[0])
                call = lambda: m.render_accumulate_pixels(raw, acc, w, h, 8, COUNT, lst)      # noqa: E731
                call()
                sp, de = [], []
                for _ in range(a.repeats):
                    sp.append(window_ms(call, a.min_seconds))
                    de.append(window_ms(dense, a.min_seconds))
                s_rate = [k * COUNT / (1e3 * t) for t in sp]
                d_rate = [n * COUNT / (1e3 * t) for t in de]
                row = dict(listed=k, sparse_ms=summary(sp), dense_ms=summary(de), sparse_msamples_per_s=summary(s_rate, 1),
                           dense_msamples_per_s=summary(d_rate, 1), rate_ratio=round(summary(s_rate, 6)["median"] / summary(d_rate, 6)["median"], 3))
                if kind == "selected":
                    row["threshold"] = thr
                scene[f"{kind}_{int(round(100 * density))}pct"] = row
                log(name, kind, density, row)
        scene["overflow_events"] = raw.stats()["overflow_events"]
        res[name] = scene
        raw.close()
    return res


def end_to_end(a):
    stl, raw = load("redchair")
    w, h = a.width, a.height
    n = w * h
    ref = torch.zeros(4 * n, device=DEV)
    done = 0
    while done < a.reference_spp:
        c = min(256, a.reference_spp - done)
        m.render_accumulate(ref, w, h, done, c, raw)
        done += c
    ref_mean = (ref.view(n, 4)[:, :3] / float(a.reference_spp)).double()
    mn, step, cap = 8, 8, 64

    def mse(acc, counts):
        mean = acc.view(n, 4)[:, :3].double() / counts.double().view(n, 1)
        return float(((mean - ref_mean) ** 2).mean())

    def adaptive(thr):
        """render_adaptive's loop, keeping the accumulation buffer (the driver returns the 8-bit image only)."""
        acc, asq = torch.zeros(4 * n, device=DEV), torch.zeros(4 * n, device=DEV)
        cn = torch.zeros(n, dtype=torch.int32, device=DEV)
        pix, num = torch.empty(n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        img = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
        m.render_accumulate_pixels(raw, acc, w, h, 0, mn, None, asq, cn)
        r = 0
        while mn + (r + 1) * step <= cap:
            m.select_pixels(acc, asq, cn, w, h, mn, cap, thr, pix, num)
            k = int(num.item())
            if k == 0:
                break
            m.render_accumulate_pixels(raw, acc, w, h, mn + r * step, step, pix[:k], asq, cn)
            r += 1
        m.finalize_counts(img, acc, cn, w, h)
        torch.cuda.synchronize()
        return acc, cn, r

    def uniform(spp):
        acc = torch.zeros(4 * n, device=DEV)
        img = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
        m.render_accumulate(acc, w, h, 0, spp, raw)
        m.finalize(img, acc, w, h, spp)
        torch.cuda.synchronize()
        return acc

    def wall(fn):
        fn()      # warm-up
        t = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return summary(t)

    res = dict(reference_spp=a.reference_spp, min_spp=mn, step=step, max_spp=cap, runs={})
    for label, thr in (("max_variance_1e-4", 1e-4), ("max_variance_1e-5", 1e-5)):
        acc, cn, rounds = adaptive(thr)
        total = int(cn.sum().item())
        row = dict(kind="adaptive", max_variance=thr, rounds=rounds, total_samples=total, mean_spp=round(total / n, 2), mse=mse(acc, cn),
                   wall_ms=wall(lambda: adaptive(thr)))
        res["runs"][label] = row
        log(label, row)
        spp = max(2, int(round(total / n)))
        acc = uniform(spp)
        row = dict(kind="uniform", spp=spp, total_samples=spp * n, mse=mse(acc, torch.full((n,), spp, device=DEV)), wall_ms=wall(lambda: uniform(spp)))
        res["runs"][f"uniform_{spp}spp_matching_{label}"] = row
        log("uniform", row)
    acc = uniform(cap)
    res["runs"][f"uniform_{cap}spp"] = dict(kind="uniform", spp=cap, total_samples=cap * n, mse=mse(acc, torch.full((n,), cap, device=DEV)),
                                            wall_ms=wall(lambda: uniform(cap)))
    log("uniform cap", res["runs"][f"uniform_{cap}spp"])
    res["overflow_events"] = raw.stats()["overflow_events"]
    raw.close()
    return res


def dense_order_kept(a):
    res = {}
    for name in ("tenthousand", "redchair"):
        stl, raw = load(name)
        w, h = a.width, a.height
        n = w * h
        img = torch.empty(4 * n, dtype=torch.uint8, device=DEV)
        acc = torch.zeros(4 * n, device=DEV)
        frame = lambda: m.render(img, w, h, COUNT, raw)      # noqa: E731
        for _ in range(3):
            frame()
        before = [window_ms(frame, a.min_seconds) for _ in range(a.repeats)]
        g = torch.Generator(device=DEV).manual_seed(99)
        for k in range(12):
            lst = torch.randperm(n, device=DEV, generator=g)[:n // (2 + k)].to(torch.int32).contiguous()
            m.render_accumulate_pixels(raw, acc, w, h, 0, COUNT, lst)
        torch.cuda.synchronize()
        after = [window_ms(frame, a.min_seconds) for _ in range(a.repeats)]
        raw.set_option("sched", 0)
        frame()
        unordered = [window_ms(frame, a.min_seconds) for _ in range(a.repeats)]
        b, f = summary(before), summary(after)
        spread = max(b["max"] - b["min"], f["max"] - f["min"])
        res[name] = dict(before_ms=b, after_ms=f, frame_order_ms=summary(unordered), spread_ms=round(spread, 3),
                         equal_within_spread=bool(abs(b["median"] - f["median"]) <= max(spread, 0.01 * b["median"])))
        log(name, res[name])
        raw.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--only", default="i,ii,iv")
    a = ap.parse_args()
    only = set(a.only.split(","))
    out = dict(metric="adaptive_sampling", width=a.width, height=a.height, samples_per_call=COUNT, repeats=a.repeats, min_seconds=a.min_seconds)
    if "i" in only:
        out["sparse_throughput"] = sparse_throughput(a)
    if "ii" in only:
        out["end_to_end_redchair"] = end_to_end(a)
    if "iv" in only:
        out["dense_order_kept"] = dense_order_kept(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

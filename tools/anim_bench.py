#!/usr/bin/env python3
"""Animated sequences: updates of a built scene in place against creating the scene again for every frame, in ms per frame.

    python tools/anim_bench.py [--frames 60] [--repeats 5] [--min-seconds 0.5] [--skip-synthetic] [--only camera,spheres,shading,synthetic]

Sequences (1920 x 1080, 16 spp unless stated; --frames frames each):
  camera      scenes/tenthousand.txt, the camera orbiting the scene centre by 1 degree per frame
  spheres     the same, and every sphere displaced per frame from a torch tensor (update + build + render)
  synthetic   the 1 M sphere + 1 M triangle synthetic scene (BASELINE config 5) at 8 spp: camera orbit + sphere positions updated
  shading     scenes/tenthousand.txt plus one point light: the bulb flies through the scene and every sphere's colour is swept,
              per frame (mirt_scene_set_lights + mirt_scene_update_sphere_materials; no build); fixed camera
Each sequence runs two ways, alternating within every repeat:
  in_place    mirt_scene_set_camera / mirt_scene_update_spheres + mirt_build_lbvh on one scene
  recreate    mirt_scene_create + mirt_build_lbvh + render + destroy per frame (moved spheres / swept materials are copied to the
              host and put into the MirtSphere array first: the only way without the update calls)
and, next to them, `static` (the same number of frames with nothing changing) and -- camera sequence -- `in_place_sched0` (the
hand-out order switched off instead of kept from the first frame).  A timed window is the whole sequence, repeated until it
lasts --min-seconds; the host clock brackets it and it ends in a synchronise.  --repeats windows each: median, min, max.
`update_build_ms` is the device time of update + build per frame (HIP events around them).
`material_update_wait_ms`: what the render that follows a material update waits for on the host -- host clock from issuing an update
of every primitive's material to the end of its kernels (update, OR over all flag bytes, 4-byte copy) -- at 10 k primitives and, unless
--skip-synthetic, at 2 M.  Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cuda_ray_tracer_amd as m  # noqa: E402
from cuda_ray_tracer_amd import api  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def summary(ms):
    s = sorted(ms)
    return dict(ms_per_frame=round(s[len(s) // 2], 4), min=round(s[0], 4), max=round(s[-1], 4))


def orbit(cam, centre, degrees):
    """`cam` turned about the vertical axis through `centre`."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)

    def rot(v):
        return (c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2])

    eye = cam.eye.tolist()
    rel = rot([eye[k] - centre[k] for k in range(3)])
    return api._camera_with(cam, dict(eye=[rel[k] + centre[k] for k in range(3)], forward=rot(cam.forward.tolist()),
                                      right=rot(cam.right.tolist()), up=rot(cam.up.tolist())))


def mat_rows(records):
    """float32 [n, 11] rows of a sphere / triangle array's materials: the format of the material update calls."""
    return np.ascontiguousarray(records["mat"]).view(np.float32).reshape(len(records), 11)


def material_update_wait(stl, repeats):
    """Host clock from issuing a material update of every primitive to the end of its kernels: what the next render waits for."""
    raw = m.initRawConfigFromStl(stl, 0)
    kinds = [(m.update_sphere_materials, torch.from_numpy(mat_rows(stl.array("spheres"))).cuda()),
             (m.update_triangle_materials, torch.from_numpy(mat_rows(stl.array("triangles"))).cuda())]
    ms = []
    for r in range(repeats + 1):             # (the first allocates the flag bytes: not timed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for update, rows in kinds:
            if rows.shape[0]:
                update(raw, rows)
        torch.cuda.current_stream().synchronize()
        if r:
            ms.append(1e3 * (time.perf_counter() - t0))
    raw.close()
    s = sorted(ms)
    return dict(ms=round(s[len(s) // 2], 4), min=round(s[0], 4), max=round(s[-1], 4), primitives=int(stl.num_prims))


class Sequence:
    def __init__(self, stl, w, h, spp, frames, move_camera, move_spheres, move_shading=False):
        self.stl, self.w, self.h, self.spp, self.frames = stl, w, h, spp, frames
        self.move_camera, self.move_spheres, self.move_shading = move_camera, move_spheres, move_shading
        self.img = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
        self.raw = m.initRawConfigFromStl(stl, 0)
        m.build_lbvh_karas(self.raw)
        bounds = self.raw.tree()[3]
        self.centre = [0.5 * float(bounds[k] + bounds[3 + k]) for k in range(3)]
        self.cam0 = self.raw.camera()
        self.cams = [orbit(self.cam0, self.centre, f + 1.0) for f in range(frames)]
        self.sph = stl.array("spheres")
        base = np.concatenate([self.sph["c"], self.sph["r"][:, None]], axis=1).astype(np.float32)
        self.base = torch.from_numpy(base).cuda()
        g = torch.Generator(device="cuda").manual_seed(1234)
        self.phase = torch.rand((base.shape[0], 3), generator=g, device="cuda") * (2 * math.pi)
        self.amp = 0.25 * self.base[:, 3:4]
        self.xyzr = self.base.clone()
        self.update_build_ms = []
        if move_shading:
            self.bulbs0 = stl.array("bulbs")
            self.mats0 = torch.from_numpy(mat_rows(self.sph)).cuda()
            self.mats = self.mats0.clone()

    def bulbs(self, f):
        """Frame f's point lights: each on a circle about the scene centre."""
        b = self.bulbs0.copy()
        a = 0.1 * (f + 1)
        b["v"][:, 0] = self.centre[0] + 1.5 * math.cos(a)
        b["v"][:, 2] = self.centre[2] + 1.5 * math.sin(a)
        return b

    def materials(self, f):
        """Frame f's sphere materials, on the device: the colours swept (the caller's animation step: the same work both ways)."""
        self.mats[:, 0:3] = self.mats0[:, 0:3] * (0.6 + 0.4 * torch.sin(self.phase + 0.1 * (f + 1)))
        return self.mats

    def positions(self, f):
        """Frame f's spheres, on the device (the caller's simulation step: the same work both ways)."""
        self.xyzr[:, :3] = self.base[:, :3] + self.amp * torch.sin(self.phase + 0.1 * (f + 1))
        return self.xyzr

    def static(self):
        for _ in range(self.frames):
            m.render(self.img, self.w, self.h, self.spp, self.raw)
        torch.cuda.synchronize()

    def in_place(self):
        raw = self.raw
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        spent = 0.0
        for f in range(self.frames):
            if self.move_camera:
                raw.set_camera(self.cams[f])
            if self.move_spheres:
                x = self.positions(f)
                e0.record()
                m.update_spheres(raw, x)
                m.build_lbvh_karas(raw)
                e1.record()
            if self.move_shading:
                raw.set_lights(bulbs=self.bulbs(f))
                m.update_sphere_materials(raw, self.materials(f))
            m.render(self.img, self.w, self.h, self.spp, raw)
            if self.move_spheres:
                e1.synchronize()
                spent += e0.elapsed_time(e1)
        torch.cuda.synchronize()
        if self.move_spheres:
            self.update_build_ms.append(spent / self.frames)

    def reset(self):
        """Back to frame 0's scene (not timed)."""
        self.raw.set_camera(self.cam0)
        if self.move_spheres:
            m.update_spheres(self.raw, self.base)
            m.build_lbvh_karas(self.raw)
        if self.move_shading:
            self.raw.set_lights(bulbs=self.bulbs0)
            m.update_sphere_materials(self.raw, self.mats0)
        torch.cuda.synchronize()

    def recreate(self):
        d = api.SceneDesc.from_buffer_copy(bytes(self.stl.desc))
        sph = self.sph.copy()
        for f in range(self.frames):
            if self.move_camera:
                cam = self.cams[f]
                d.eye, d.forward, d.right, d.up = cam.eye, cam.forward, cam.right, cam.up
            if self.move_spheres:
                x = self.positions(f).cpu().numpy()
                sph["c"] = x[:, :3]
                sph["r"] = x[:, 3]
                d.spheres = sph.ctypes.data
            if self.move_shading:
                bulbs = self.bulbs(f)
                d.bulbs = bulbs.ctypes.data
                sph["mat"] = self.materials(f).cpu().numpy().view(sph.dtype["mat"]).reshape(-1)
                d.spheres = sph.ctypes.data
            raw = m.RawConfig(d, 0)
            m.build_lbvh_karas(raw)
            m.render(self.img, self.w, self.h, self.spp, raw)
            raw.close()                      # (mirt_scene_destroy waits for the frame)
        torch.cuda.synchronize()

    def window(self, fn, min_seconds):
        """ms per frame of one timed window: the whole sequence, as often as it takes to last min_seconds."""
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                return 1e3 * dt / (n * self.frames)

    def close(self):
        self.raw.close()


def run(name, seq, repeats, min_seconds, with_sched0):
    ways = [("in_place", seq.in_place), ("recreate", seq.recreate), ("static", seq.static)]
    times = {k: [] for k, _ in ways}
    seq.static()                             # warm-up: workspaces, random-number tables, the hand-out order
    seq.in_place()
    seq.reset()
    seq.update_build_ms.clear()
    for r in range(repeats):
        for k, fn in ways:
            times[k].append(seq.window(fn, min_seconds))
            seq.reset()
        log(f"{name} repeat {r}: " + ", ".join(f"{k} {times[k][-1]:.3f}" for k, _ in ways))
    res = {k: summary(v) for k, v in times.items()}
    if with_sched0:
        seq.raw.set_option("sched", 0)
        seq.in_place()
        seq.reset()
        t = [seq.window(seq.in_place, min_seconds) for _ in range(repeats)]
        seq.reset()
        seq.raw.set_option("sched", 2)
        res["in_place_sched0"] = summary(t)
        log(f"{name} sched 0: {res['in_place_sched0']}")
    if seq.update_build_ms:
        res["update_build_ms"] = summary(seq.update_build_ms)
        res["update_build_ms"]["ms"] = res["update_build_ms"].pop("ms_per_frame")
    spread = max(res[k]["max"] - res[k]["min"] for k in ("in_place", "recreate"))
    res["spread_ms"] = round(spread, 4)
    res["in_place_over_static_ms"] = round(res["in_place"]["ms_per_frame"] - res["static"]["ms_per_frame"], 4)
    res["recreate_over_static_ms"] = round(res["recreate"]["ms_per_frame"] - res["static"]["ms_per_frame"], 4)
    res["in_place_not_slower"] = bool(res["in_place"]["ms_per_frame"] <= res["recreate"]["ms_per_frame"] + spread)
    res.update(frames=seq.frames, spp=seq.spp, spheres=int(seq.base.shape[0]), primitives=int(seq.stl.num_prims))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--skip-synthetic", action="store_true")
    ap.add_argument("--only", default="camera,spheres,shading,synthetic", help="the sequences to run, comma separated")
    a = ap.parse_args()
    only = set(a.only.split(","))
    out = dict(metric="anim_ms_per_frame", width=a.width, height=a.height, frames=a.frames, repeats=a.repeats, min_seconds=a.min_seconds,
               sequences={})
    stl = m.parseInput(os.path.join(ROOT, "scenes", "tenthousand.txt"))
    for name, cam, sph in (("camera", True, False), ("spheres", True, True)):
        if name not in only:
            continue
        seq = Sequence(stl, a.width, a.height, 16, a.frames, cam, sph)
        out["sequences"][name] = run(name, seq, a.repeats, a.min_seconds, with_sched0=(name == "camera"))
        st = seq.raw.stats()
        out["sequences"][name]["overflow_events"] = st["overflow_events"]
        seq.close()
    text = open(os.path.join(ROOT, "scenes", "tenthousand.txt")).read() + "\ncolor 1 1 1\nbulb 0 1 0\n"
    stl_bulb = m.parseText(text)
    if "shading" in only:
        seq = Sequence(stl_bulb, a.width, a.height, 16, a.frames, False, False, move_shading=True)
        out["sequences"]["shading"] = run("shading", seq, a.repeats, a.min_seconds, with_sched0=False)
        out["sequences"]["shading"]["overflow_events"] = seq.raw.stats()["overflow_events"]
        seq.close()
        out["material_update_wait_ms"] = {"tenthousand": material_update_wait(stl_bulb, max(a.repeats, 5))}
    if not a.skip_synthetic and only & {"shading", "synthetic"}:
        stl = m.syntheticScene()
        if "shading" in only:
            out["material_update_wait_ms"]["synthetic"] = material_update_wait(stl, max(a.repeats, 5))
    if not a.skip_synthetic and "synthetic" in only:
        seq = Sequence(stl, a.width, a.height, 8, a.frames, True, True)
        out["sequences"]["synthetic"] = run("synthetic", seq, a.repeats, a.min_seconds, with_sched0=False)
        out["sequences"]["synthetic"]["overflow_events"] = seq.raw.stats()["overflow_events"]
        seq.close()
    out["in_place_not_slower_anywhere"] = all(s["in_place_not_slower"] for s in out["sequences"].values())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

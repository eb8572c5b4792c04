"""Pass length and batch threshold by what a scene's rays do (csrc/render_plan.h, PASS_STEPS): r, the primitive tests per
internal-node visit counted by the call that measures the sample order, enters plan_call as one more fact.  The sphere-only
quantised kernels take `reps` and `batch_k` from a monotone step function of r -- fewer primitive tests per visit, longer passes --
when the options are at 0; before r is known, and for every other kind of kernel, the values are the ones from before the rule;
an explicit option wins.  No GPU for the plan: tests/pass_length_plan_probe.cpp is compiled with the host compiler.  One GPU test
holds the r a scene reports to the ratio of its counters, and a geometry update to discarding it."""
import json
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

KEYS = ("prim_ratio", "reps", "batch_k", "Nt", "N", "qnodes", "traversal", "wavefront", "tree_depth")
BASE = dict(prim_ratio=-1.0, reps=0, batch_k=0, Nt=0, N=10000, qnodes=1, traversal=1, wavefront=0, tree_depth=20)      # a sphere-only scene, options by plan
DEEP = dict(BASE, tree_depth=29)      # ... whose tree is too deep for the kernel that starts rays from LDS: the other sphere-only quantised kernels
TODAY = (4, 8)              # reps, batch_k of the sphere-only quantised kernels before the rule
with open(os.path.join(HERE, "golden", "pass_length_ratios.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def probe():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_pass_length_plan_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "pass_length_plan_probe")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "pass_length_plan_probe.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

        def plans(cases):
            text = "".join(" ".join(repr(float(c[k])) if k == "prim_ratio" else str(int(c[k])) for k in KEYS) + "\n" for c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield plans


RATIOS = [0.0, 0.01, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.5, 0.6, 0.75, 1.0, 1.5, 2.0, 10.0, 1e6] + [s["r"] for s in GOLDEN["scenes"].values()]


def test_unknown_r_gives_the_values_from_before_the_rule(probe):
    for r in (-1.0, -0.5, -1e30):
        p = probe([dict(BASE, prim_ratio=r)])[0]
        assert (p["qn"], p["notri"]) == (1, 1) and (p["reps"], p["batch_k"]) == TODAY, r


def test_an_explicit_option_wins_each_on_its_own(probe):
    for r in RATIOS + [-1.0]:
        by_plan = probe([dict(BASE, prim_ratio=r)])[0]
        for reps in (1, 3, 4, 8):
            p = probe([dict(BASE, prim_ratio=r, reps=reps)])[0]
            assert p["reps"] == reps and p["batch_k"] == by_plan["batch_k"], (r, reps)
        for batch_k in (1, 8, 13, 64):
            p = probe([dict(BASE, prim_ratio=r, batch_k=batch_k)])[0]
            assert p["batch_k"] == batch_k and p["reps"] == by_plan["reps"], (r, batch_k)
        p = probe([dict(BASE, prim_ratio=r, reps=5, batch_k=7)])[0]
        assert (p["reps"], p["batch_k"]) == (5, 7)


def test_fewer_primitive_tests_per_visit_never_mean_shorter_passes(probe):
    rs = sorted(RATIOS)
    for base, start_lds in ((BASE, 1), (DEEP, 0)):      # (either kind of sphere-only quantised kernel)
        got = probe([dict(base, prim_ratio=r) for r in rs])
        assert all(p["start_lds"] == start_lds and p["qn"] == 1 and p["notri"] == 1 for p in got)
        reps = [p["reps"] for p in got]
        assert all(a >= b for a, b in zip(reps, reps[1:])), list(zip(rs, reps))
        assert all(1 <= p["reps"] <= 8 and 1 <= p["batch_k"] <= 64 for p in got)
        # the rule is a step function with few steps; the two ends differ (the rule does something)
        assert len(set((p["reps"], p["batch_k"]) for p in got)) <= 4 and reps[0] > reps[-1]


def test_other_kinds_of_kernel_are_unaffected(probe):
    for r in RATIOS:
        # triangles: the wide records (N >= 65536) or the exact ones; the reference's walk order; no quantised records; the wavefront pair
        for kw, want in ((dict(Nt=100000, N=200000), (5, 8)), (dict(Nt=100, N=1700), (4, 8)), (dict(traversal=0), (4, 8)), (dict(qnodes=0), (4, 8)),
                         (dict(wavefront=1), (4, 8))):
            p = probe([dict(BASE, prim_ratio=r, **kw)])[0]
            assert not (p["qn"] and p["notri"]) and (p["reps"], p["batch_k"]) == want, (r, kw, p)


def test_the_bundled_sphere_scenes_get_the_settings_the_sweep_recorded(probe):
    """r of tenthousand.txt and spiral.txt at 1920 x 1080 x 16 as measured (and of the synthetic scenes of the sweep), with the
    depth of their trees, and the settings profiles/r09_ab_runs.txt records as their best."""
    assert {"tenthousand", "spiral"} <= set(GOLDEN["scenes"])
    for name, s in GOLDEN["scenes"].items():
        assert abs(s["r"] - s["prim_tests"] / s["internal_visits"]) < 1e-6, name
        p = probe([dict(BASE, prim_ratio=s["r"], tree_depth=s["tree_depth"])])[0]
        assert p["start_lds"] == (1 if s["tree_depth"] <= 23 else 0), name
        assert (p["reps"], p["batch_k"]) == (s["reps"], s["batch_k"]), (name, p)
    assert GOLDEN["scenes"]["tenthousand"]["r"] < GOLDEN["scenes"]["spiral"]["r"]


@pytest.mark.gpu
def test_the_ratio_read_back_is_the_counters_ratio_and_a_geometry_update_discards_it():
    import torch
    import cuda_ray_tracer_amd as m
    from cuda_ray_tracer_amd import api

    def ratio(raw):
        return struct.unpack("<f", struct.pack("<i", raw.get_option("prim_ratio_bits")))[0]

    w, h, spp = 64, 36, 4
    stl = m.parseInput(os.path.join(ROOT, "scenes", "tenthousand.txt"))
    raw = m.initRawConfigFromStl(stl, 0)
    m.build_lbvh_karas(raw)
    assert ratio(raw) == -1.0                        # nothing rendered yet
    img = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
    m.render(img, w, h, spp, raw)                    # the first call of the shape: measures the sample order, and r with it
    torch.cuda.synchronize()
    assert ratio(raw) == -1.0                        # the option polls nothing: r is taken by the next render call ...
    raw.sample_order()                               # ... or by mirt_get_sample_order, which waits for the measurement
    got = ratio(raw)
    m.render(img, w, h, spp, raw, params=api.render_params(w, h, spp, counters=True))      # a counting render
    torch.cuda.synchronize()
    st = raw.stats()
    want = np.float32((st["sphere_tests"] + st["tri_tests"]) / st["internal_visits"])
    assert st["internal_visits"] > 0 and got == want, (got, want)
    assert ratio(raw) == got                         # an ordered call leaves it alone
    sph = stl.array("spheres")
    xyzr = np.ascontiguousarray(np.concatenate([sph["c"], sph["r"][:, None]], axis=1), dtype=np.float32)
    xyzr[:, 0] += 0.5
    api.update_spheres(raw, torch.from_numpy(xyzr).cuda())
    m.build_lbvh_karas(raw)
    assert ratio(raw) == -1.0                        # the old geometry's rays say nothing about the new one
    m.render(img, w, h, spp, raw)                    # (the order is kept across the update: nothing measures again for this shape)
    torch.cuda.synchronize()
    assert ratio(raw) == -1.0
    m.render(img, w, h, spp + 4, raw)                # another shape measures afresh, on the moved geometry
    torch.cuda.synchronize()
    m.render(img, w, h, spp + 4, raw)                # (the next call of the shape finds the measurement finished)
    torch.cuda.synchronize()
    moved = ratio(raw)
    assert moved > 0.0
    # An update that arrives while a measurement is still in flight: what that call counted is the old geometry's and is not kept.
    m.render(img, w, h, spp, raw)                    # (the shape of the first call again: measures again) -- no synchronise
    assert ratio(raw) == -1.0                        # (the new shape's measurement discarded the old r at once)
    xyzr[:, 1] += 0.25
    api.update_spheres(raw, torch.from_numpy(xyzr).cuda())
    m.build_lbvh_karas(raw)
    raw.sample_order()                               # the measurement has landed by now: its order is kept, its counts are not
    assert ratio(raw) == -1.0
    m.render(img, w, h, spp, raw)
    torch.cuda.synchronize()
    assert ratio(raw) == -1.0
    raw.close()

"""When a render's plan picks the kernel whose loop header starts rays from LDS (csrc/render_plan.h, CallPlan::start_lds;
render.hip, SPEC_START_LDS): its stack is one slot shorter, 23 of the wave's 24, and the block sits in the slot that frees.
Exactly when the kernel without a spill path is chosen (lds_only) for the specialised sphere-only quantised walk, the built tree
is at most 23 internal nodes deep -- D bounds the entries of the walk -- the option `ray_start_lds` is on and the scene's suns fit
the block.  No GPU: tests/ray_start_plan_probe.cpp is compiled with the host compiler."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

KEYS = ("tree_depth", "stack_lds_depth", "ray_start_lds", "specialise", "num_suns", "num_bulbs", "any_trans", "gi", "Nt", "wavefront", "traversal")
BASE = dict(tree_depth=20, stack_lds_depth=-1, ray_start_lds=1, specialise=1, num_suns=1, num_bulbs=0, any_trans=0, gi=0, Nt=0, wavefront=0, traversal=1)      # tenthousand.txt: D = 20


@pytest.fixture(scope="module")
def probe():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_ray_start_plan_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "ray_start_plan_probe")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "ray_start_plan_probe.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

        def plans(cases):
            text = "".join(" ".join(str(int(c[k])) for k in KEYS) + "\n" for c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield plans


def test_the_block_fits_the_slot_the_shorter_stack_frees(probe):
    p = probe([BASE])[0]
    assert (p["slots"], p["stack_lds"]) == (23, 24)
    assert 16 + 24 * p["suns"] <= 64 * 4 and 6 * p["suns"] <= 64 and p["suns"] >= 1      # one wave per workgroup: 256 bytes per slot


def test_the_headline_scene_gets_it(probe):
    p = probe([BASE])[0]
    assert (p["start_lds"], p["lds_only"], p["qn"], p["notri"], p["nobulb"], p["nopend"]) == (1, 1, 1, 1, 1, 1)


def test_tree_depth_on_each_side_of_the_23_slots(probe):
    depths = [0, 1, 13, 22, 23, 24, 25, 58, -1]
    got = probe([dict(BASE, tree_depth=d) for d in depths])
    assert [p["start_lds"] for p in got] == [1, 1, 1, 1, 1, 0, 0, 0, 0], got
    # (lds_only itself keeps its boundary at the 24 slots of the general stack)
    assert [p["lds_only"] for p in got] == [1, 1, 1, 1, 1, 1, 0, 0, 0], got


def test_sun_count_on_each_side_of_the_block(probe):
    suns = probe([BASE])[0]["suns"]
    counts = [0, 1, suns - 1, suns, suns + 1, 32, 64]
    got = probe([dict(BASE, num_suns=c) for c in counts])
    assert [p["start_lds"] for p in got] == [1, 1, 1, 1, 0, 0, 0], got
    assert all(p["lds_only"] == 1 for p in got)


def test_the_option_and_the_switches_that_keep_the_other_kernels(probe):
    off, on = probe([dict(BASE, ray_start_lds=0), dict(BASE, ray_start_lds=1)])
    assert (off["start_lds"], off["lds_only"]) == (0, 1) and on["start_lds"] == 1
    # specialise = 0: the general kernels; an explicit stack_lds_depth (the compiled size included): the kernel with a spill path
    assert probe([dict(BASE, specialise=0)])[0]["start_lds"] == 0
    for d in (0, 2, 23, 24):
        p = probe([dict(BASE, stack_lds_depth=d)])[0]
        assert (p["start_lds"], p["lds_only"]) == (0, 0), d
    assert probe([dict(BASE, wavefront=1)])[0]["start_lds"] == 0
    # the reference's walk order: exact records, no quantised walk
    p = probe([dict(BASE, traversal=0)])[0]
    assert (p["start_lds"], p["qn"], p["lds_only"]) == (0, 0, 1)


def test_only_the_sphere_only_kernel_without_point_lights_transparency_or_gi(probe):
    for kw in (dict(num_bulbs=1), dict(any_trans=1), dict(gi=2), dict(Nt=100)):
        p = probe([dict(BASE, **kw)])[0]
        assert p["start_lds"] == 0, kw
    # every condition at its boundary at once
    suns = probe([BASE])[0]["suns"]
    assert probe([dict(BASE, tree_depth=23, num_suns=suns)])[0]["start_lds"] == 1
    assert probe([dict(BASE, tree_depth=24, num_suns=suns)])[0]["start_lds"] == 0
    assert probe([dict(BASE, tree_depth=23, num_suns=suns + 1)])[0]["start_lds"] == 0

"""Which trace kernel a render's plan picks for the traversal stack (csrc/render_plan.h, CallPlan::lds_only): the one without a
spill path exactly when the built tree's depth D -- the most internal nodes on a root-to-leaf path, which bounds the entries a
two-child walk keeps pending -- is within the capacity of the register-plus-LDS stack, the option stack_lds_depth is at its
default, and the walk is over two-child records.  No GPU: tests/stack_plan_probe.cpp is compiled with the host compiler."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

KEYS = ("tree_depth", "stack_lds_depth", "wavefront", "traversal", "qnodes", "N", "Nt", "grid_ok", "has_quantised", "has_wide")
SPHERES = dict(tree_depth=13, stack_lds_depth=-1, wavefront=0, traversal=1, qnodes=1, N=10000, Nt=0, grid_ok=1, has_quantised=1, has_wide=0)
EXACT = dict(SPHERES, N=1700, Nt=1000, has_quantised=0, has_wide=1)             # triangles, fewer than 65536 primitives: the 64-byte records
WIDE = dict(SPHERES, N=65536, Nt=1000, has_quantised=0, has_wide=1)             # the wide quantised records: up to three pushes a step


@pytest.fixture(scope="module")
def probe():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_stack_plan_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "stack_plan_probe")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "stack_plan_probe.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr

        def plans(cases):
            text = "".join(" ".join(str(int(c[k])) for k in KEYS) + "\n" for c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield plans


def test_the_capacity_is_every_lds_slot(probe):
    """One entry in a register, the others in slots 1 .. STACK_LDS - 1; slot 0 holds no entry (render.hip, MIRT_PUSH)."""
    p = probe([SPHERES])[0]
    assert p["capacity"] == p["stack_lds"] == 24


def test_depth_just_below_at_and_just_above_the_capacity(probe):
    cap = probe([SPHERES])[0]["capacity"]
    for base in (SPHERES, EXACT):
        depths = [0, 1, cap - 1, cap, cap + 1, 58]
        got = probe([dict(base, tree_depth=d) for d in depths])
        assert [p["lds_only"] for p in got] == [1, 1, 1, 1, 0, 0], (base, got)
    # a scene whose depth is not known (nothing built) keeps the general kernel
    assert probe([dict(SPHERES, tree_depth=-1)])[0]["lds_only"] == 0


def test_the_two_child_walks_only(probe):
    sph, exact, wide = probe([SPHERES, EXACT, WIDE])
    assert (sph["qn"], sph["notri"], sph["lds_only"]) == (1, 1, 1)
    assert (exact["qn"], exact["notri"], exact["lds_only"]) == (0, 0, 1)
    assert (wide["qn"], wide["notri"], wide["lds_only"]) == (1, 0, 0)
    # qnodes = 2: a small scene with triangles walks the wide records as well; qnodes = 0: everything the exact ones
    small_wide, all_exact = probe([dict(EXACT, qnodes=2), dict(WIDE, qnodes=0)])
    assert (small_wide["qn"], small_wide["lds_only"]) == (1, 0)
    assert (all_exact["qn"], all_exact["lds_only"]) == (0, 1)
    # a sphere-only scene on the exact records (the reference's order, or a grid that does not resolve it) is a two-child walk too
    for kw in (dict(traversal=0), dict(grid_ok=0), dict(qnodes=0)):
        p = probe([dict(SPHERES, **kw)])[0]
        assert (p["qn"], p["lds_only"]) == (0, 1), kw
    # the trace / shade kernel pair has its own stack
    assert probe([dict(SPHERES, wavefront=1)])[0]["lds_only"] == 0


def test_any_explicit_stack_lds_depth_keeps_the_general_kernel(probe):
    """The tests force the spill path with the option, and it must keep doing exactly that: the depth the kernel is given is
    unchanged, and no value but the default -- not even the compiled size -- selects the kernel without a spill path."""
    cap = probe([SPHERES])[0]["capacity"]
    depths = [-1, 0, 1, 2, cap - 1, cap, cap + 1, 64]
    for base in (SPHERES, EXACT, WIDE):
        got = probe([dict(base, stack_lds_depth=d) for d in depths])
        assert [p["lds_depth"] for p in got] == [d if 0 <= d <= cap else cap for d in depths]
        assert [p["lds_only"] for p in got] == [int(base is not WIDE)] + [0] * (len(depths) - 1), (base, got)

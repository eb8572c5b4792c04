"""The owning types of csrc/dev_mem.h (DevBuf, PinnedBuf, Event, Stream) need no GPU: a stand-alone probe, tests/dev_mem_probe.cpp, defines
the few runtime entry points the header calls over malloc -- a set of live handles, an abort on a free of something not live, a
k-th allocation that can be told to fail -- and is compiled with the host compiler (address + undefined sanitizers where they
link).  Each case checks itself and that nothing is live when it ends.  The same file holds the source check that keeps the
library's allocation and release calls inside that header."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cuda_ray_tracer_amd", "csrc")

CASES = ["grow_device", "grow_pinned", "failure_device", "failure_pinned", "move_device", "move_pinned", "reset_device", "reset_pinned", "conversion", "event", "stream", "together", "message"]


def rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    hipcc = shutil.which("hipcc")
    if hipcc:
        inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
        if os.path.exists(os.path.join(inc, "hip", "hip_runtime_api.h")):
            return inc
    return None


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe into a private directory; returns run(case) -> CompletedProcess."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    inc = rocm_include()
    if not cxx or not inc:
        pytest.skip("no host C++ compiler or no HIP headers")
    with tempfile.TemporaryDirectory(prefix="mirt_dev_mem_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "dev_mem_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + inc, os.path.join(HERE, "dev_mem_probe.cpp"), "-o", exe]
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        if san.returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr
        # which build ran is in the test's output (pytest -rA, or -s), so that a toolchain that lost the sanitizers shows
        print("dev_mem_probe: built with the address and undefined sanitizers" if san.returncode == 0 else
              "dev_mem_probe: built WITHOUT sanitizers, the sanitizer build failed:\n" + san.stderr[-2000:])
        yield lambda *args: subprocess.run([exe, *args], capture_output=True, text=True)


def test_the_probe_has_exactly_these_cases(probe):
    r = probe()
    assert r.returncode == 0 and r.stdout.split() == CASES, (r.stdout, r.stderr)


@pytest.mark.parametrize("case", CASES)
def test_owning_types(probe, case):
    """grow_*: below, at and above capacity -- the pointer kept and no wait in the first two; one wait, the old block freed and the
    new capacity in the third.  failure_*: a failed alloc / grow leaves pointer null and capacity 0 with the old block freed and
    returns the error status, the raw form the runtime's error with no message set.  move_*: construction and assignment empty the
    source, assignment frees the target's old block.  reset_*: reset twice, destruction of an empty object, zero-length alloc.
    event: create twice makes one event; a std::vector<Event> grown past several reallocations destroys each event exactly once.
    stream: the same of Stream, with reset twice, destruction of an empty object and a failing creation that leaves it empty and
    names the call's file and line.
    together: four buffers whose last capacity stands for all (the chunk orders), the k-th allocation failing, then a smaller
    request: it allocates again.  message: a failure names the file and line of the call and the caller's label.
    Every case: the live set is empty at exit (a free of something not live aborts in the probe)."""
    r = probe(case)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith(case + ":") and r.stdout.rstrip().endswith(" 0 failures"), r.stdout


FORBIDDEN = ("hipFree", "hipHostFree", "hipEventDestroy", "hipMalloc(", "hipHostMalloc(", "hipEventCreate", "hipStreamCreate", "hipStreamDestroy")
EXEMPT = ("dev_mem.h", "raytracer_main.cpp")      # the types themselves; a client of the C ABI


def test_only_the_owning_types_allocate_and_release():
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name in EXEMPT:
            continue
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                found += [(name, no, word) for word in FORBIDDEN if word in line]
    assert not found, found
    assert len(os.listdir(CSRC)) > len(EXEMPT) and all(os.path.exists(os.path.join(CSRC, e)) for e in EXEMPT)


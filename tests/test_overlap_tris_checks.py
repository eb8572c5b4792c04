"""The argument checks of the two triangle-overlap entry points (csrc/host_scene.cpp: check_overlap_triangles and
check_triangle_list, through check_row_query) need no GPU: a stand-alone probe, tests/overlap_tris_checks_probe.cpp, is compiled with
the host compiler together with host_scene.cpp -- once plainly and once with the address and undefined-behaviour sanitizers, where they
link -- and prints the status, `go` and the message of every case it reads.  The addresses are made up and never dereferenced.

Held here: the status and the exact message of every check, every message naming its entry point, and the order of the checks --
flags, n, capacity, null, alignment, overlap, built."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cuda_ray_tracer_amd", "csrc")
OK, ERR_ARG, ERR_STATE = 0, 3, 6
N, CAP = 100, 1000
A, B_, C_ = 1 << 48, 2 << 48, 3 << 48      # far apart, aligned to everything
COUNT, FILL = "mirt_overlap_triangles: ", "mirt_triangle_list: "
FILL_NULL = FILL + "null buffer (d_tris and d_offsets when n > 0; d_words when capacity > 0)"
FILL_ALIGN = FILL + "d_tris and d_words must be 4-byte aligned, d_offsets 8-byte aligned"
FILL_OVER = FILL + "d_tris, d_offsets and d_words must not overlap each other"
COUNT_ALIGN = COUNT + "d_tris and d_counts must be 4-byte aligned"
COUNT_OVER = COUNT + "d_tris and d_counts must not overlap each other"


def line(entry, flags=0, n=N, p=(A, B_, C_), capacity=CAP, built=1):
    return f"{entry} {flags} {n} {p[0]} {p[1]} {p[2]} {capacity} {built}"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request):
    """Compiles the probe with host_scene.cpp into a private directory; returns run(list of lines) -> [(status, go, message)]."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_tris_checks_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "overlap_tris_checks_probe")
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(HERE, "overlap_tris_checks_probe.cpp"), os.path.join(CSRC, "host_scene.cpp"), "-o", exe]
        if request.param == "sanitized":
            cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0 and request.param == "sanitized":
            pytest.skip("the toolchain has no sanitizer runtimes")
        assert r.returncode == 0, r.stderr

        def run(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", r.stderr
            out = r.stdout.splitlines()
            assert len(out) == len(lines)
            got = []
            for text in out:
                head, message = text.split("|", 1)
                status, go = head.split()
                got.append((int(status), int(go), message))
            return got
        yield run


def test_every_check_of_the_count_call_in_order(probe):
    bad = dict(built=0)      # (every later check fails as well: the first one's message is reported)
    cases = [
        (line("count", flags=2, n=-1, p=(A + 2, A, 0), **bad), (ERR_ARG, 0, COUNT + "unknown flag bits")),
        (line("count", flags=0xfffffffe, **bad), (ERR_ARG, 0, COUNT + "unknown flag bits")),
        (line("count", flags=3), (ERR_ARG, 0, COUNT + "unknown flag bits")),
        (line("count", n=-1, p=(0, A + 2, 0), **bad), (ERR_ARG, 0, COUNT + "negative n")),
        (line("count", n=-(1 << 40)), (ERR_ARG, 0, COUNT + "negative n")),
        (line("count", p=(0, A + 2, 0), **bad), (ERR_ARG, 0, COUNT + "null buffer")),
        (line("count", p=(A + 2, 0, 0), **bad), (ERR_ARG, 0, COUNT + "null buffer")),
        (line("count", p=(A + 2, A, 0), **bad), (ERR_ARG, 0, COUNT_ALIGN)),
        (line("count", p=(A, A + 36 * N - 2, 0), **bad), (ERR_ARG, 0, COUNT_ALIGN)),
        (line("count", p=(A + 1, B_, 0)), (ERR_ARG, 0, COUNT_ALIGN)),
        (line("count", p=(A, A + 36 * N - 4, 0), **bad), (ERR_ARG, 0, COUNT_OVER)),      # the counts' first word on the rows' last
        (line("count", p=(A + 4 * N - 4, A, 0), **bad), (ERR_ARG, 0, COUNT_OVER)),
        (line("count", p=(A, A, 0)), (ERR_ARG, 0, COUNT_OVER)),
        (line("count", p=(A, A + 36 * N, 0)), (OK, 1, "")),                             # touching is not overlapping
        (line("count", p=(A + 4 * N, A, 0)), (OK, 1, "")),
        (line("count", **bad), (ERR_STATE, 0, COUNT + "call mirt_build_lbvh first")),
        (line("count", n=0, **bad), (ERR_STATE, 0, COUNT + "call mirt_build_lbvh first")),
        (line("count", n=0, p=(0, 0, 0)), (OK, 0, "")),                                  # n == 0: nothing to do, no buffer looked at
        (line("count", n=0, p=(A, A, 0)), (OK, 0, "")),
        (line("count"), (OK, 1, "")),
        (line("count", flags=1), (OK, 1, "")),                                           # MIRT_TRIS_ANY
        (line("count", p=(A + 4, B_ + 4, 0)), (OK, 1, "")),                              # rows of 36 bytes need 4-byte alignment only
    ]
    got = probe([c for c, _ in cases])
    for (c, want), have in zip(cases, got):
        assert have == want, (c, want, have)
    assert len({w[2] for _, w in cases}) >= 7      # every message of the entry point was asked for


def test_every_check_of_the_fill_in_order(probe):
    bad = dict(built=0)
    rows, offs, words = 36 * N, 8 * (N + 1), 4 * CAP
    cases = [
        (line("fill", flags=1), (OK, 1, "")),                                            # (the fill takes no flags: the probe's are not passed on)
        (line("fill", n=-1, capacity=-1, p=(A + 2, A, A), **bad), (ERR_ARG, 0, FILL + "negative n")),
        (line("fill", capacity=-1, p=(0, A + 4, A), **bad), (ERR_ARG, 0, FILL + "negative capacity")),
        (line("fill", capacity=-1, p=(0, 0, 0)), (ERR_ARG, 0, FILL + "negative capacity")),
        (line("fill", p=(0, B_ + 4, C_), **bad), (ERR_ARG, 0, FILL_NULL)),
        (line("fill", p=(A + 2, 0, C_), **bad), (ERR_ARG, 0, FILL_NULL)),
        (line("fill", p=(A + 2, B_, 0), **bad), (ERR_ARG, 0, FILL_NULL)),
        (line("fill", p=(A + 2, A, C_), **bad), (ERR_ARG, 0, FILL_ALIGN)),
        (line("fill", p=(A, A + 4, C_), **bad), (ERR_ARG, 0, FILL_ALIGN)),              # offsets need 8
        (line("fill", p=(A, B_, A + 2), **bad), (ERR_ARG, 0, FILL_ALIGN)),
        (line("fill", p=(A, A + rows - 4 - (rows - 4) % 8, C_), **bad), (ERR_ARG, 0, FILL_OVER)),      # offsets inside the rows
        (line("fill", p=(A + offs - 4, A, C_), **bad), (ERR_ARG, 0, FILL_OVER)),                       # rows on the offsets' last word
        (line("fill", p=(A, B_, A + rows - 4), **bad), (ERR_ARG, 0, FILL_OVER)),                       # words on the rows' last word
        (line("fill", p=(A + words - 4, B_, A), **bad), (ERR_ARG, 0, FILL_OVER)),
        (line("fill", p=(A, B_, B_ + offs - 4), **bad), (ERR_ARG, 0, FILL_OVER)),                      # words on the offsets' last word
        (line("fill", p=(A, B_ + words - 8, B_), **bad), (ERR_ARG, 0, FILL_OVER)),
        (line("fill", p=(A, B_, A + rows)), (OK, 1, "")),                                # touching is not overlapping
        (line("fill", p=(A, B_, B_ + offs)), (OK, 1, "")),
        (line("fill", p=(A + offs, A, C_)), (OK, 1, "")),
        (line("fill", **bad), (ERR_STATE, 0, FILL + "call mirt_build_lbvh first")),
        (line("fill", n=0, capacity=0, p=(0, 0, 0), **bad), (ERR_STATE, 0, FILL + "call mirt_build_lbvh first")),
        (line("fill", n=0, p=(0, 0, C_)), (OK, 0, "")),                                  # no row
        (line("fill", n=0, capacity=0, p=(0, 0, 0)), (OK, 0, "")),
        (line("fill", capacity=0, p=(A, B_, 0)), (OK, 0, "")),                           # no word any row could write
        (line("fill", capacity=0, p=(A, B_, A)), (OK, 0, "")),                           # ... and a range of no bytes overlaps nothing
        (line("fill"), (OK, 1, "")),
    ]
    got = probe([c for c, _ in cases])
    for (c, want), have in zip(cases, got):
        assert have == want, (c, want, have)
    assert len({w[2] for _, w in cases}) >= 7

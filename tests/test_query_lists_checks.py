"""The argument checks of the ray and ball lists (csrc/host_scene.cpp: check_ray_list and check_ball_list, through check_row_query)
need no GPU: a stand-alone probe, tests/query_lists_checks_probe.cpp, is compiled with the host compiler together with
host_scene.cpp (address + undefined sanitizers where they link) and prints the status, `go` and the message of every case it reads.
The addresses are made up and never dereferenced; `built` arrives as a bool.

Held here, per entry point: the status and the exact message of every check, and the order of the checks -- unknown flag bits, a
negative row count, a negative capacity, a required buffer that is null, alignment, overlap, the scene's tree: a call that fails
check i also fails every later check it can, and check i's message is the one reported.

Buffers are multiples of four bytes at addresses that are multiples of four, so the overlap cases put one buffer's start at the last
address its alignment allows inside the other, and right at the other's end (touching: no error)."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cuda_ray_tracer_amd", "csrc")
OK, ERR_ARG, ERR_STATE = 0, 3, 6
N, CAP = 100, 1000
BASE = [(i + 1) << 48 for i in range(4)]      # far apart, aligned to everything

# probe name: (entry point, the row count's name, bytes per row, the rows' and the values' parameter names)
ENTRIES = {"ray": ("mirt_ray_list", "num_rays", 32, "d_rays", "d_t"), "ball": ("mirt_ball_list", "n", 16, "d_points", "d_dist")}


def messages(name):
    who, n_name, _, rows, vals = ENTRIES[name]
    return dict(flags=f"{who}: unknown flag bits", n=f"{who}: negative {n_name}", capacity=f"{who}: negative capacity",
                null=f"{who}: null buffer ({rows} and d_offsets when {n_name} > 0; d_words when capacity > 0)",
                align=f"{who}: {rows} must be 16-byte aligned, d_offsets 8-byte aligned, d_words and {vals} 4-byte aligned",
                overlap=f"{who}: {rows}, d_offsets, d_words and {vals} must not overlap each other", built=f"{who}: call mirt_build_lbvh first")


def good(**over):
    c = dict(flags=0, n=N, p=list(BASE), capacity=CAP, built=1)
    c.update(over)
    c["p"] = list(c["p"])
    return c


def sizes(name, c):
    return [ENTRIES[name][2] * c["n"], 8 * (c["n"] + 1) if c["n"] > 0 else 0, 4 * c["capacity"], 4 * c["capacity"]]


ALIGN = [16, 8, 4, 4]


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe with host_scene.cpp into a private directory; returns run(name, cases) -> [(status, go, message)]."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_checks_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "query_lists_checks_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(HERE, "query_lists_checks_probe.cpp"), os.path.join(CSRC, "host_scene.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr

        def run(name, cases):
            lines = [f"{name} {c['flags']} {c['n']} {c['p'][0]} {c['p'][1]} {c['p'][2]} {c['p'][3]} {c['capacity']} {c['built']}" for c in cases]
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = r.stdout.splitlines()
            assert len(out) == len(lines)
            got = []
            for text in out:
                head, message = text.split("|", 1)
                status, go = head.split()
                got.append((int(status), int(go), message))
            return got
        yield run


def later_failures(c, after):
    """The call c made to fail, as well, the checks that come after check `after` where it can: misaligned, overlapping, not built."""
    c = good(**c)
    order = ["flags", "n", "capacity", "null", "align", "overlap", "built"]
    rank = order.index(after)
    c["built"] = 0
    if rank < order.index("overlap"):
        c["p"][1] = c["p"][0]           # (the offsets on top of the rows)
    if rank < order.index("align"):
        c["p"][0] += 4                  # (and the rows off their alignment)
    return c


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_check_has_its_status_and_message_in_the_order_of_the_checks(probe, name):
    msg = messages(name)
    cases, want = [], []

    def expect(c, status, go, message):
        cases.append(c)
        want.append((status, go, message))

    # flags must be 0: every bit; before a negative row count and everything later
    for flags in (1, 2, 4, 1 << 31, 0xffffffff):
        expect(later_failures(good(flags=flags, n=-1, capacity=-1), "flags"), ERR_ARG, 0, msg["flags"])
    # a negative row count: before a negative capacity and everything later
    for n in (-1, -(1 << 40)):
        expect(later_failures(good(n=n, capacity=-1), "n"), ERR_ARG, 0, msg["n"])
    # a negative capacity: before the null check (every pointer null, too) and everything later
    for capacity in (-1, -(1 << 40)):
        expect(later_failures(good(capacity=capacity), "capacity"), ERR_ARG, 0, msg["capacity"])
        expect(good(capacity=capacity, p=[0, 0, 0, 0], built=0), ERR_ARG, 0, msg["capacity"])
    # each required buffer null: before alignment and everything later; the values may be absent
    for i in range(4):
        c = good(built=0)
        c["p"][i] = 0
        c["p"][1 if i == 0 else 0] += 2      # (another buffer misaligned)
        expect(c, ERR_ARG, 0, msg["null"] if i < 3 else msg["align"])
    expect(good(p=[0, 0, 0, 0]), ERR_ARG, 0, msg["null"])
    expect(good(p=BASE[:3] + [0]), OK, 1, "")
    # with no rows only the words are required, with no capacity only the rows and offsets
    expect(good(n=0, p=[0, 0, 0, 0], built=0), ERR_ARG, 0, msg["null"])
    expect(good(capacity=0, p=[0, BASE[1], 0, 0], built=0), ERR_ARG, 0, msg["null"])
    expect(good(capacity=0, p=[BASE[0], 0, 0, 0], built=0), ERR_ARG, 0, msg["null"])
    # each alignment class off by 4 or 8 bytes (4-byte buffers: by 2): before the overlap and `built`
    for i, align in enumerate(ALIGN):
        for off in ({16: (4, 8), 8: (4,), 4: (2,)})[align]:
            c = good(built=0)
            c["p"][i] += off
            c["p"][1 if i == 0 else 0] = c["p"][i] - off      # (and on top of another buffer)
            expect(c, ERR_ARG, 0, msg["align"])
    # each pair of the four ranges: sharing the least their alignments allow (both ways round) is refused before `built`; touching is not
    g = good()
    size = sizes(name, g)
    assert all(s > 0 for s in size)
    pairs = 0
    for x in range(4):
        for y in range(4):
            if x == y:
                continue
            end = g["p"][x] + size[x]
            inside = (end - 1) // ALIGN[y] * ALIGN[y]      # the last address y's alignment allows inside x
            assert g["p"][x] <= inside < end and end - inside <= 16
            c = good(built=0)
            c["p"][y] = inside
            expect(c, ERR_ARG, 0, msg["overlap"])
            if end % ALIGN[y] == 0:
                c = good()
                c["p"][y] = end
                expect(c, OK, 1, "")
            pairs += 1
    assert pairs == 12
    # not built -- also with no rows or no capacity --, no work, and a good call
    for over in (dict(), dict(n=0), dict(capacity=0), dict(n=0, capacity=0, p=[0, 0, 0, 0])):
        expect(good(built=0, **over), ERR_STATE, 0, msg["built"])
    expect(good(n=0), OK, 0, "")
    expect(good(capacity=0), OK, 0, "")
    expect(good(n=0, capacity=0, p=[0, 0, 0, 0]), OK, 0, "")
    expect(good(), OK, 1, "")
    expect(good(n=1, capacity=1), OK, 1, "")
    got = probe(name, cases)
    for c, w, r in zip(cases, want, got):
        assert r == w, (c, w, r)
    assert {w[2] for w in want} == set(msg.values()) | {""}      # every message of the entry point was asked for


@pytest.mark.parametrize("name", list(ENTRIES))
def test_a_range_of_zero_bytes_overlaps_nothing(probe, name):
    """capacity == 0 (no word, no value), no rows, absent values: such a buffer may lie anywhere, on top of another one too."""
    msg = messages(name)
    same = [BASE[0]] * 4
    assert probe(name, [good(n=0, p=same), good(capacity=0, p=[BASE[0], BASE[1], BASE[0], BASE[0]]), good(n=0, capacity=0, p=same)]) == \
        [(ERR_ARG, 0, msg["overlap"]), (OK, 0, ""), (OK, 0, "")]      # (with no rows the words and the values still have bytes)
    assert probe(name, [good(n=0, p=[BASE[0], BASE[0], BASE[0], BASE[1]]), good(n=0, p=[BASE[0], BASE[0], BASE[0], 0])]) == [(OK, 0, ""), (OK, 0, "")]
    # the values on top of the words are refused; absent they are no range
    assert probe(name, [good(p=BASE[:3] + [BASE[2]]), good(p=BASE[:3] + [0])]) == [(ERR_ARG, 0, msg["overlap"]), (OK, 1, "")]

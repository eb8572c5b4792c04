"""The argument checks of the seven row queries (csrc/host_scene.cpp: check_row_query and its callers check_closest_points,
check_closest_points_multi, check_cast_spheres, check_overlap_boxes, check_list_offsets, check_overlap_list and
check_trace_rays_multi; any_overlap) need no GPU: a stand-alone probe, tests/row_query_checks_probe.cpp, is compiled with the host
compiler together with host_scene.cpp (address + undefined sanitizers where they link) and prints the status, `go` and the message of
every case it reads.  The addresses are made up and never dereferenced; `built` arrives as a bool.

Held here, per entry point: the status and the exact message of every check, and the order of the checks -- a call that fails check i
also fails every later check it can (at least `built`), and check i's message is the one reported.  The messages are written out
below as the entry points had them before the checks were shared.

Buffers are multiples of four bytes at addresses that are multiples of four, so two of an entry point's buffers cannot share exactly
one byte: the overlap cases put one buffer's start at the last address its alignment allows inside the other (a shared word or row),
and right at the other's end (touching: no error).  Ranges that share exactly one byte go to any_overlap directly."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cuda_ray_tracer_amd", "csrc")
OK, ERR_ARG, ERR_STATE = 0, 3, 6
N, K = 100, 2
BASE = [(i + 1) << 48 for i in range(4)]      # far apart, aligned to everything


class Entry:
    def __init__(self, probe, who, n_name, flag, max_k, any_flag, bufs, null_msg, align_msg, overlap_msg, rules=(), built=True, extra=0):
        self.probe, self.who, self.n_name, self.flag, self.max_k, self.any_flag = probe, who, n_name, flag, max_k, any_flag
        self.bufs = bufs          # (name, bytes(n, k, extra), alignment, required(n, k, extra)) in the probe's order p0..
        self.null_msg, self.align_msg, self.overlap_msg, self.rules, self.built, self.extra = null_msg, align_msg, overlap_msg, rules, built, extra

    def good(self, **over):
        c = dict(flags=0, n=N, k=K if self.max_k is not None else 0, p=list(BASE), extra=self.extra, built=1)
        c.update(over)
        return c

    def line(self, c):
        p = list(c["p"]) + [0] * (4 - len(c["p"]))
        return f"{self.probe} {c['flags']} {c['n']} {c['k']} {p[0]} {p[1]} {p[2]} {p[3]} {c['extra']} {c['built']}"

    def msg(self, text):
        return f"{self.who}: {text}"


ENTRIES = [
    Entry("closest", "mirt_closest_points", "n", 0, None, None,
          [("d_points", lambda n, k, x: 16 * n, 16, lambda n, k, x: n > 0), ("d_hits", lambda n, k, x: 24 * n, 4, lambda n, k, x: n > 0),
           ("d_features", lambda n, k, x: 32 * n, 16, lambda n, k, x: False)],
          "null buffer", "d_points and d_features must be 16-byte aligned, d_hits 4-byte aligned",
          "d_hits and d_features must not overlap d_points or each other"),
    Entry("multi", "mirt_closest_points_multi", "n", 0, 8, None,
          [("d_points", lambda n, k, x: 16 * n, 16, lambda n, k, x: n > 0), ("d_hits", lambda n, k, x: 24 * n * k, 4, lambda n, k, x: n > 0 and k > 0),
           ("d_counts", lambda n, k, x: 4 * n, 4, lambda n, k, x: n > 0 and k == 0), ("d_features", lambda n, k, x: 32 * n * k, 16, lambda n, k, x: False)],
          "null buffer (d_points; d_hits unless k is 0; d_counts when k is 0)",
          "d_points and d_features must be 16-byte aligned, d_hits and d_counts 4-byte aligned",
          "d_points, d_hits, d_counts and d_features must not overlap each other",
          rules=[(dict(k=-1), "k must be 0 to MIRT_CONTACTS_MAX_K (8)"), (dict(k=9), "k must be 0 to MIRT_CONTACTS_MAX_K (8)")]),
    Entry("cast", "mirt_cast_spheres", "n", 1, None, None,
          [("d_casts", lambda n, k, x: 32 * n, 16, lambda n, k, x: n > 0), ("d_hits", lambda n, k, x: 24 * n, 4, lambda n, k, x: n > 0),
           ("d_features", lambda n, k, x: 32 * n, 16, lambda n, k, x: False)],
          "null buffer", "d_casts and d_features must be 16-byte aligned, d_hits 4-byte aligned",
          "d_hits and d_features must not overlap d_casts or each other"),
    Entry("overlap", "mirt_overlap_boxes", "n", 1, 8, 1,
          [("d_boxes", lambda n, k, x: 32 * n, 16, lambda n, k, x: n > 0), ("d_hits", lambda n, k, x: 24 * n * k, 4, lambda n, k, x: n > 0 and k > 0),
           ("d_counts", lambda n, k, x: 4 * n, 4, lambda n, k, x: n > 0 and k == 0), ("d_features", lambda n, k, x: 32 * n * k, 16, lambda n, k, x: False)],
          "null buffer (d_boxes; d_hits unless k is 0; d_counts when k is 0)",
          "d_boxes and d_features must be 16-byte aligned, d_hits and d_counts 4-byte aligned",
          "d_boxes, d_hits, d_counts and d_features must not overlap each other",
          rules=[(dict(k=-1), "k must be 0 to MIRT_OVERLAP_MAX_K (8)"), (dict(k=9), "k must be 0 to MIRT_OVERLAP_MAX_K (8)"),
                 (dict(flags=1, k=1), "MIRT_OVERLAP_ANY needs k == 0"), (dict(flags=1, k=8), "MIRT_OVERLAP_ANY needs k == 0")]),
    Entry("offsets", "mirt_list_offsets", "n", None, None, None,
          [("d_counts", lambda n, k, x: 4 * n, 4, lambda n, k, x: n > 0), ("d_offsets", lambda n, k, x: 8 * (n + 1), 8, lambda n, k, x: True),
           ("d_work", lambda n, k, x: x, 8, lambda n, k, x: x > 0)],
          "null buffer (d_offsets; d_counts when n > 0; d_work when mirt_list_offsets_work_bytes(n) > 0)",
          "d_counts must be 4-byte aligned, d_offsets and d_work 8-byte aligned", "d_counts, d_offsets and d_work must not overlap each other",
          rules=[(dict(n=(1 << 40) + 1), "n above 2^40")], built=False, extra=64),
    Entry("list", "mirt_overlap_list", "n", None, None, None,
          [("d_boxes", lambda n, k, x: 32 * n, 16, lambda n, k, x: n > 0), ("d_offsets", lambda n, k, x: 8 * (n + 1) if n > 0 else 0, 8, lambda n, k, x: n > 0),
           ("d_words", lambda n, k, x: 4 * x, 4, lambda n, k, x: x > 0)],
          "null buffer (d_boxes and d_offsets when n > 0; d_words when capacity > 0)",
          "d_boxes must be 16-byte aligned, d_offsets 8-byte aligned, d_words 4-byte aligned", "d_boxes, d_offsets and d_words must not overlap each other",
          rules=[(dict(extra=-1), "negative capacity")], extra=1000),
    Entry("multihit", "mirt_trace_rays_multi", "num_rays", 0, 8, None,
          [("d_rays", lambda n, k, x: 32 * n, 16, lambda n, k, x: n > 0), ("d_hits", lambda n, k, x: 24 * n * k, 4, lambda n, k, x: n > 0 and k > 0),
           ("d_counts", lambda n, k, x: 4 * n, 4, lambda n, k, x: n > 0 and k == 0)],
          "null buffer (d_rays; d_hits unless k is 0; d_counts when k is 0)", "d_rays must be 16-byte aligned, d_hits and d_counts 4-byte aligned",
          "d_hits and d_counts must not overlap d_rays or each other",
          rules=[(dict(k=-1), "k must be 0 to MIRT_MULTIHIT_MAX_K (8)"), (dict(k=9), "k must be 0 to MIRT_MULTIHIT_MAX_K (8)")]),
]
BY_NAME = {e.probe: e for e in ENTRIES}


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe with host_scene.cpp into a private directory; returns run(list of lines) -> list of output lines."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_checks_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "row_query_checks_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(HERE, "row_query_checks_probe.cpp"), os.path.join(CSRC, "host_scene.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr

        def run(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = r.stdout.splitlines()
            assert len(out) == len(lines)
            return out
        yield run


def results(probe, entry, cases):
    """[(status, go, message)] of the calls `cases` of one entry point."""
    out = []
    for text in probe([entry.line(c) for c in cases]):
        head, message = text.split("|", 1)
        status, go = head.split()
        out.append((int(status), int(go), message))
    return out


def later_failures(e, c, after):
    """The call c made to fail, as well, the checks that come after check `after` where it can: misaligned, overlapping, not built."""
    c = dict(c, p=list(c["p"]))
    order = ["flags", "n", "rules", "null", "align", "overlap", "built"]
    rank = order.index(after)
    if rank < order.index("built"):
        c["built"] = 0
    if rank < order.index("overlap") and c["p"][0] and c["p"][1]:
        c["p"][1] = c["p"][0]                        # (the second buffer on top of the first)
    if rank < order.index("align") and c["p"][0]:
        c["p"][0] += 4 if e.bufs[0][2] > 4 else 2    # (and the first off its alignment)
    if rank < order.index("null") and rank >= order.index("rules"):
        pass                                         # (a null buffer would hide the pointer cases above; the null check has its own cases)
    return c


@pytest.mark.parametrize("name", [e.probe for e in ENTRIES])
def test_every_check_has_its_status_and_message_in_the_order_of_the_checks(probe, name):
    e = BY_NAME[name]
    cases, want = [], []

    def expect(c, status, go, message):
        cases.append(c)
        want.append((status, go, message))

    # unknown flag bits: every bit but the entry point's own; before a negative n and everything later
    if e.flag is not None:
        for flags in (2, 4, 1 << 31, 0xfffffffe) + ((1,) if e.flag == 0 else ()):
            expect(later_failures(e, e.good(flags=flags, n=-1), "flags"), ERR_ARG, 0, e.msg("unknown flag bits"))
    # negative n: before the entry point's own rules and everything later
    for n in (-1, -(1 << 40)):
        c = e.good(n=n)
        if e.max_k is not None:
            c["k"] = 9
        if e.probe == "list":
            c["extra"] = -1
        expect(later_failures(e, c, "n"), ERR_ARG, 0, e.msg("negative " + e.n_name))
    # the entry point's own rules, in their order (k's range before MIRT_OVERLAP_ANY's k): before the null check and everything later
    for change, text in e.rules:
        expect(later_failures(e, e.good(**change), "rules"), ERR_ARG, 0, e.msg(text))
        nulls = e.good(**change)
        nulls["p"] = [0, 0, 0, 0]
        expect(nulls, ERR_ARG, 0, e.msg(text))
    if e.any_flag is not None:
        expect(e.good(flags=e.any_flag, k=9), ERR_ARG, 0, e.msg("k must be 0 to MIRT_OVERLAP_MAX_K (8)"))
    # each required buffer null (k > 0 and k == 0 ask for different ones): before alignment and everything later
    for k in ([K, 0] if e.max_k is not None else [0]):
        g = e.good(k=k)
        for i, (bname, nbytes, align, required) in enumerate(e.bufs):
            c = dict(g, p=list(g["p"]))
            c["p"][i] = 0
            other = 1 if i == 0 else 0
            c["p"][other] += 2                       # (another buffer misaligned)
            c["built"] = 0
            if required(c["n"], k, c["extra"]):
                expect(c, ERR_ARG, 0, e.msg(e.null_msg))
            else:                                    # an optional buffer may be absent: the next failure is the alignment
                expect(c, ERR_ARG, 0, e.msg(e.align_msg))
    # each alignment class off by 4 or 8 bytes (4-byte buffers: by 2): before the overlap and `built`
    for i, (bname, nbytes, align, required) in enumerate(e.bufs):
        for off in ({16: (4, 8), 8: (4,), 4: (2,)})[align]:
            c = e.good(built=0)
            c["p"][i] += off
            j = 1 if i == 0 else 0
            c["p"][j] = c["p"][i] - off              # (and on top of another buffer)
            expect(c, ERR_ARG, 0, e.msg(e.align_msg))
    # each pair of buffers: sharing the least their alignments allow (both ways round) is refused before `built`; touching is not
    g = e.good()
    size = [nbytes(g["n"], g["k"], g["extra"]) for _, nbytes, _, _ in e.bufs]
    assert all(s > 0 for s in size)
    pairs = 0
    for x in range(len(e.bufs)):
        for y in range(len(e.bufs)):
            if x == y:
                continue
            end = g["p"][x] + size[x]
            inside = (end - 1) // e.bufs[y][2] * e.bufs[y][2]      # the last address y's alignment allows inside x
            assert g["p"][x] <= inside < end and end - inside <= 16
            c = e.good(built=0)
            c["p"][y] = inside
            expect(c, ERR_ARG, 0, e.msg(e.overlap_msg))
            if end % e.bufs[y][2] == 0:
                c = e.good()
                c["p"][y] = end
                expect(c, OK, 1, "")
            pairs += 1
    assert pairs == len(e.bufs) * (len(e.bufs) - 1)
    # not built -- also with n == 0 --, n == 0, and a good call
    if e.built:
        expect(e.good(built=0), ERR_STATE, 0, e.msg("call mirt_build_lbvh first"))
        expect(e.good(built=0, n=0), ERR_STATE, 0, e.msg("call mirt_build_lbvh first"))
    expect(e.good(n=0), OK, 0, "")
    expect(e.good(), OK, 1, "")
    if e.flag:
        expect(e.good(flags=e.flag, k=0), OK, 1, "")
    if e.max_k is not None:
        for k in range(0, e.max_k + 1):
            expect(e.good(k=k), OK, 1, "")
    got = results(probe, e, cases)
    for c, w, r in zip(cases, want, got):
        assert r == w, (e.line(c), w, r)
    assert len({w[2] for w in want}) >= 6      # every message of the entry point was asked for


def test_a_range_of_zero_bytes_overlaps_nothing(probe):
    """k == 0 (no hit records, no feature rows), an absent d_features, capacity == 0, n == 0, no work bytes: such a buffer may lie
    anywhere, on top of another one too."""
    same = [BASE[0]] * 4
    for name in ("multi", "overlap", "multihit"):
        e = BY_NAME[name]
        # k == 0: d_hits and d_features on top of the rows; d_counts, which has bytes, apart
        p = [BASE[0], BASE[0], BASE[1], BASE[0]]
        assert results(probe, e, [e.good(k=0, p=p)]) == [(OK, 1, "")]
        # ... and d_counts on top of them is refused
        assert results(probe, e, [e.good(k=0, p=same)]) == [(ERR_ARG, 0, e.msg(e.overlap_msg))]
        # k > 0 without counts: a null d_counts has no bytes
        assert results(probe, e, [e.good(p=[BASE[0], BASE[1], 0, BASE[2]])]) == [(OK, 1, "")]
    for name in ("closest", "cast", "multi", "overlap"):
        e = BY_NAME[name]
        p = list(BASE)
        p[len(e.bufs) - 1] = 0                       # d_features absent
        assert results(probe, e, [e.good(p=p)]) == [(OK, 1, "")]
    for e in ENTRIES:
        assert results(probe, e, [e.good(n=0, p=same, extra=0)]) == [(OK, 0, "")], e.probe      # n == 0: nothing has bytes but d_offsets' total
    lst = BY_NAME["list"]
    # capacity == 0: d_words anywhere, nothing to do; with a capacity it is refused
    assert results(probe, lst, [lst.good(extra=0, p=[BASE[0], BASE[1], BASE[0]]), lst.good(p=[BASE[0], BASE[1], BASE[0]])]) == \
        [(OK, 0, ""), (ERR_ARG, 0, lst.msg(lst.overlap_msg))]
    off = BY_NAME["offsets"]
    # no work bytes: d_work is not looked at -- null, misaligned or on top of the counts
    assert results(probe, off, [off.good(extra=0, p=[BASE[0], BASE[1], 0]), off.good(extra=0, p=[BASE[0], BASE[1], BASE[0] + 3]),
                                off.good(p=[BASE[0], BASE[1], BASE[0]])]) == [(OK, 1, ""), (OK, 1, ""), (ERR_ARG, 0, off.msg(off.overlap_msg))]
    # n == 0 still writes the total: d_offsets is required and checked
    assert results(probe, off, [off.good(n=0, extra=0, p=[0, 0, 0]), off.good(n=0, extra=0, p=[0, BASE[1] + 4, 0])]) == \
        [(ERR_ARG, 0, off.msg(off.null_msg)), (ERR_ARG, 0, off.msg(off.align_msg))]


def test_list_offsets_refuses_more_than_2_to_the_40_counts(probe):
    off = BY_NAME["offsets"]
    work = 8 * (((1 << 40) + 2047) // 2048)
    got = results(probe, off, [off.good(n=1 << 40, extra=work), off.good(n=(1 << 40) + 1, extra=work), off.good(n=(1 << 40) + 1, extra=work, p=[0, 0, 0]),
                               off.good(n=1 << 62, extra=0), off.good(n=-1, extra=0)])
    assert got == [(OK, 1, ""), (ERR_ARG, 0, off.msg("n above 2^40")), (ERR_ARG, 0, off.msg("n above 2^40")), (ERR_ARG, 0, off.msg("n above 2^40")),
                   (ERR_ARG, 0, off.msg("negative n"))]


def test_any_overlap_is_exact_to_the_byte_and_skips_empty_ranges(probe):
    a = 1 << 20
    cases = [
        ([(a, 10), (a + 9, 5)], 1),                  # one shared byte
        ([(a, 10), (a + 10, 5)], 0),                 # touching
        ([(a + 9, 5), (a, 10)], 1),
        ([(a, 10), (a + 3, 1)], 1),                  # one byte inside
        ([(a, 10), (a + 3, 0)], 0),                  # no bytes: inside, and overlapping nothing
        ([(a, 0), (a, 0)], 0),
        ([(0, 0), (a, 10), (0, 0)], 0),
        ([(a, 10), (a + 20, 10), (a + 40, 10), (a + 49, 1)], 1),      # the last pair of four
        ([(a, 10), (a + 20, 10), (a + 40, 10), (a + 50, 1)], 0),
        ([(a, 1)], 0),
        ([], 0),
    ]
    lines = ["ranges %d %s" % (len(r), " ".join(f"{p} {b}" for p, b in r)) for r, _ in cases]
    assert probe(lines) == [f"overlap={w}" for _, w in cases]

"""What the LBVH build decides on the host (csrc/build_plan.h: grid counts, the workspace layout, the ordered-key map of the scene
bounds, the facts read off the root record) needs no GPU: a stand-alone probe, tests/build_plan_probe.cpp, is compiled with the
host compiler (address + undefined sanitizers where they link) and prints what the header computes for every case it reads.
Checked here against Python integers and a numpy float32 restatement."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SIZES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 2_000_000, 2**31 - 1]
REF_LEAF, REF_TRI = 0x80000000, 0x40000000


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe into a private directory; returns ask(list of lines) -> list of dicts of ints."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_build_plan_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "build_plan_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "build_plan_probe.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr

        def ask(lines):
            r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(lines)
            return out
        yield ask


def ceil_div(a, b):
    return -(-a // b)


def test_the_workspace_regions_lie_where_the_build_uses_them(probe):
    """Python integers on this side: a 32-bit overflow on the way (4 n words pass 2^32 at the largest n) would show as a mismatch."""
    for n, w in zip(SIZES, probe([f"L {n}" for n in SIZES])):
        assert (w["block"], w["sort_tile"], w["scan_tile"], w["radix"]) == (256, 2048, 2048, 256)
        sblocks, scan = ceil_div(n, 2048), ceil_div(n, 2048)
        size = dict(k0=n, v0=n, k1=n, v1=n, hist=256 * sblocks, totals=256, arrived=n - 1, block_sums=scan)
        want = dict(k0=0, v0=n, k1=2 * n, v1=3 * n, hist=4 * n, totals=4 * n + 256 * sblocks, arrived=4 * n + 256 * sblocks + 256)
        assert {k: w[k] for k in want} == want and w["total"] == want["arrived"] + n - 1, (n, w)
        for k, s in size.items():      # every region inside the allocation
            assert 0 <= w[k] and w[k] + s <= w["total"], (n, k)
        # live together: everything the sort touches and the arrival counters; later the block sums and the arrival counters
        for group in (("k0", "v0", "k1", "v1", "hist", "totals", "arrived"), ("block_sums", "arrived")):
            spans = sorted((w[k], w[k] + size[k]) for k in group)
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (n, group, spans)
        assert w["k1"] <= w["block_sums"] and w["block_sums"] + size["block_sums"] <= w["k1"] + size["k1"], n      # the alias: inside k1
        assert w["sort_ws"] == 256 * ceil_div(n, 2048) + 256, n


def test_grid_counts_are_ceilings(probe):
    for n, w in zip(SIZES, probe([f"L {n}" for n in SIZES])):
        assert (w["item_blocks"], w["inner_blocks"], w["sort_blocks"], w["scan_blocks"]) == \
            (ceil_div(n, 256), ceil_div(n - 1, 256), ceil_div(n, 2048), ceil_div(n, 2048)), n


def test_ordered_keys_invert_and_keep_the_order(probe):
    flt_max, denorm = np.finfo(F).max, F(1e-42)
    special = [F(0.0), F(-0.0), denorm, -denorm, F(1), F(-1), flt_max, -flt_max, F(np.inf), F(-np.inf)]
    rng = np.random.default_rng(7)
    # (random bit patterns cover every exponent; NaNs among them are dropped: they have no place in the order)
    random = rng.integers(0, 2**32, 400, dtype=np.uint64).astype(np.uint32).view(F)
    x = np.concatenate([np.array(special, F), random[~np.isnan(random)], rng.normal(0, 100, 200).astype(F)])
    assert len(x) > 500
    got = probe([f"K {b:08x}" for b in x.view(np.uint32)])
    key = np.array([g["key"] for g in got], np.int64)
    assert np.array_equal(np.array([g["back"] for g in got], np.uint32), x.view(np.uint32))      # key2f(f2key(x)) has x's bits, -0.0 and denormals included
    less = x[:, None] < x[None, :]
    assert less.sum() > 100000 and np.all((key[:, None] < key[None, :])[less])
    assert 0 <= key.min() and key.max() < 2**32


def test_the_bounds_key_tables_equal_their_definitions(probe):
    t, = probe(["T"])
    assert [t[f"empty{i}"] for i in range(6)] == [2**32 - 1] * 3 + [0] * 3          # the identities of min and of max over uint32
    assert [t[f"shipped{i}"] for i in range(6)] == [t["key_pos_inf"]] * 3 + [t["key_neg_inf"]] * 3      # min = +inf, max = -inf
    assert (t["key_pos_inf"], t["key_neg_inf"]) == (0xff800000, 0x007fffff)          # ... as the build has always uploaded them


def box_facts(rec):
    """scene_box_facts in numpy float32: rec = left (xmin, xmax, ymin, ymax, zmin, zmax), right the same."""
    rec = np.asarray(rec, F)
    coord_max = F(0)
    for v in rec:
        coord_max = np.fmax(coord_max, np.abs(v))
    lo, hi = np.fmin(rec[0:6:2], rec[6:12:2]), np.fmax(rec[1:6:2], rec[7:12:2])
    with np.errstate(invalid="ignore"):
        ok = bool(np.all(np.fmax(np.abs(lo), np.abs(hi)) <= F(64) * (hi - lo)))      # (a NaN compares false)
    return coord_max, ok


def record(x_lo, x_hi, rest=(-1.0, 1.0)):
    """A root record whose x extent is [x_lo, x_hi], split between the children in the middle; the other axes span `rest`."""
    mid = F(0.5) * (F(x_lo) + F(x_hi))
    return np.array([x_lo, mid, rest[0], rest[1], rest[0], rest[1], mid, x_hi, rest[0], rest[1], rest[0], rest[1]], F)


def test_scene_box_facts(probe):
    above = np.nextafter(F(128), F(np.inf))
    assert above - F(2) + F(2) == above and F(64) * (above - (above - F(2))) == F(128)      # the box moved by one ulp keeps its extent of 2
    # A NaN plane of the scene box fails the test through !(a <= b).  fminf / fmaxf drop a NaN that only ONE child's box holds
    # (the union is the other child's plane), so such a word changes nothing: the rule is kept as the build has always had it.
    nan, nan_one_child = record(-1, 1), record(-1, 1)
    nan[3] = nan[9] = np.nan
    nan_one_child[3] = np.nan
    cases = {
        "at the origin": (record(-1, 1), True),
        "64 extents exactly": (record(126, 128), True),
        "one ulp above": (record(above - F(2), above), False),
        "64 extents, negative side": (record(-128, -126), True),
        "no extent, off the origin": (record(1, 1, rest=(1.0, 1.0)), False),
        "all zero": (np.zeros(12, F), True),
        "a NaN word": (nan, False),
        "a NaN word in one child only": (nan_one_child, True),
        "far from the origin": (record(1000, 1001), False),
    }
    got = probe(["B " + " ".join(f"{b:08x}" for b in rec.view(np.uint32)) for rec, _ in cases.values()])
    for (name, (rec, ok)), g in zip(cases.items(), got):
        coord_max, want_ok = box_facts(rec)
        assert want_ok == ok, name
        assert (g["coord_max"], g["grid_ok"]) == (int(coord_max.view(np.uint32)), int(ok)), name
        assert coord_max == np.nanmax(np.abs(rec)), name      # the largest magnitude of the twelve


def test_the_root_of_a_single_primitive_is_its_record(probe):
    got = probe(["R 1 0 0", "R 1 1 0", "R 1 0 12345", "R 2 0 4", "R 2 1 4", "R 3000 1 11996"])
    assert [g["root_ref"] for g in got] == [REF_LEAF, REF_LEAF | REF_TRI, REF_LEAF | 12345, 0, 0, 0]

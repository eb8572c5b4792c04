"""The launch arithmetic the query kernels share (csrc/query_launch.h: group_launch, used by light.hip, visibility.hip and
indirect.hip; row_launch, used through scene_dev.h's launch_rows by query.hip, closest.hip, closest_multi.hip, spherecast.hip,
overlap.hip, overlap_list.hip and multihit.hip) needs no GPU: a stand-alone probe, tests/group_launch_probe.cpp, is compiled with
the host compiler (address + undefined sanitizers where they link) and prints gshift and the block counts of every case it reads.  Checked here against the
expressions each of the files had of its own before they were shared, restated below."""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 256          # LBLOCK, VBLOCK and IBLOCK of the three files
CACHED = 2048        # a persistent grid: 256 compute units x 8 blocks


def former(n, lanes_per_row, cached_blocks):
    """light.hip, visibility.hip and indirect.hip as they were, with nlights / num_dirs = lanes_per_row and sc->light_blocks /
    vis_blocks / indirect_blocks = cached_blocks:
        q.gshift = 0;
        while ((1 << q.gshift) < num_dirs) ++q.gshift;
        const long long rows_per_block = (long long)(BLOCK / 64) * (64 >> q.gshift);
        const long long want = (n + rows_per_block - 1) / rows_per_block;
        const int blocks = (int)(want < cached_blocks ? want : cached_blocks);"""
    gshift = 0
    while (1 << gshift) < lanes_per_row:
        gshift += 1
    rows_per_block = (BLOCK // 64) * (64 >> gshift)
    want = (n + rows_per_block - 1) // rows_per_block
    return gshift, min(want, cached_blocks)


def former_rows(n, cached_blocks):
    """query.hip, closest.hip and multihit.hip as they were, with the cached grid = cached_blocks:
        const long long want = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
        const int blocks = (int)(want < grid ? want : grid);"""
    want = (n + BLOCK - 1) // BLOCK
    return min(want, cached_blocks)


@pytest.fixture(scope="module")
def probe():
    """Compiles the probe into a private directory; returns launch(list of (n, lanes_per_row, cached_blocks)) -> list of dicts."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory(prefix="mirt_group_") as tmp:      # private: /tmp is shared between users
        exe = os.path.join(tmp, "group_launch_probe")
        base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "group_launch_probe.cpp"), "-o", exe]
        if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            r = subprocess.run(base, capture_output=True, text=True)      # (a toolchain without the sanitizer runtimes)
            assert r.returncode == 0, r.stderr

        def launch(cases):
            text = "".join(f"{n} {k} {c}\n" for n, k, c in cases)
            r = subprocess.run([exe], input=text, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield launch


def test_the_shared_constants_are_the_former_four_pairs(probe):
    (p,) = probe([(1, 1, 1)])
    assert (p["block"], p["stack_lds"]) == (BLOCK, 20)


def test_gshift_is_the_least_power_of_two_that_holds_the_lanes(probe):
    """Every lane count a scene or a table can have, and none: direct_light with no lights has G = 1."""
    ks = list(range(0, 65))
    got = probe([(1000, k, CACHED) for k in ks])
    for k, p in zip(ks, got):
        g = p["gshift"]
        assert (1 << g) >= k and (g == 0 or (1 << (g - 1)) < k), (k, p)
        assert g == (0 if k == 0 else (k - 1).bit_length())
        assert (g, p["blocks"]) == former(1000, k, CACHED), (k, p)
    assert got[0]["gshift"] == 0 and got[1]["gshift"] == 0 and got[64]["gshift"] == 6


def test_block_count_covers_the_rows_and_stops_at_the_cached_grid(probe):
    """Around one block's rows for every G, and the largest n the entry points admit (n < 2^56), with a grid that caps and one
    that never does."""
    cases = []
    for k in (0, 1, 2, 3, 5, 16, 33, 64):
        rows_per_block = (BLOCK // 64) * (64 >> former(1, k, 1)[0])
        for n in (1, rows_per_block - 1, rows_per_block, rows_per_block + 1, 5 * rows_per_block + 1, (1 << 56) - 1):
            if n < 1:
                continue
            for cached in (1, 3, CACHED, (1 << 31) - 1):
                cases.append((n, k, cached))
    got = probe(cases)
    capped = uncapped = 0
    for (n, k, cached), p in zip(cases, got):
        gshift, blocks = former(n, k, cached)
        assert (p["gshift"], p["blocks"]) == (gshift, blocks), (n, k, cached, p)
        rows_per_block = (BLOCK // 64) * (64 >> gshift)
        want = -(-n // rows_per_block)
        assert 1 <= p["blocks"] <= cached and p["blocks"] == min(want, cached)
        capped += want > cached
        uncapped += want <= cached
        if want <= cached:
            assert (p["blocks"] - 1) * rows_per_block < n <= p["blocks"] * rows_per_block      # the last block has a row, and no row is left over
    assert capped > 20 and uncapped > 20
    # one row fewer than a block's, a block's, one more: 1, 1 and 2 blocks (K = 64: a block serves 4 rows)
    assert [p["blocks"] for p in probe([(3, 64, CACHED), (4, 64, CACHED), (5, 64, CACHED)])] == [1, 1, 2]
    # just under 2^56 rows: the count is the cached grid's, whatever it is
    assert [p["blocks"] for p in probe([((1 << 56) - 1, 64, 1), ((1 << 56) - 1, 1, CACHED), ((1 << 56) - 1, 0, (1 << 31) - 1)])] == [1, CACHED, (1 << 31) - 1]


def test_row_launch_gives_one_lane_per_row_and_stops_at_the_cached_grid(probe):
    """Around one block's rows, a count above what the cached grid serves at a time, the largest n the entry points admit, and a
    cached grid of one block."""
    ns = (1, 255, 256, 257, 5 * 256 + 1, CACHED * 256, CACHED * 256 + 1, 3 * CACHED * 256 + 7, (1 << 56) - 1)
    cases = [(n, 1, cached) for n in ns for cached in (1, 3, CACHED, (1 << 31) - 1)]
    got = probe(cases)
    for (n, _, cached), p in zip(cases, got):
        want = -(-n // BLOCK)
        assert p["row_blocks"] == former_rows(n, cached) == min(want, cached), (n, cached, p)
        assert 1 <= p["row_blocks"] <= cached
        assert p["row_blocks"] == p["blocks"]                                    # a grouped launch with G = 1 is the same grid
        if want <= cached:
            assert (p["row_blocks"] - 1) * BLOCK < n <= p["row_blocks"] * BLOCK      # the last block has a row, and no row is left over
    by = {(n, cached): p["row_blocks"] for (n, _, cached), p in zip(cases, got)}
    assert [by[(n, CACHED)] for n in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert by[(CACHED * 256, CACHED)] == CACHED and by[(CACHED * 256 + 1, CACHED)] == CACHED and by[(3 * CACHED * 256 + 7, CACHED)] == CACHED
    assert all(by[(n, 1)] == 1 for n in ns)
    # the lanes of a row do not enter it
    assert [p["row_blocks"] for p in probe([(1000, k, CACHED) for k in (0, 1, 16, 64)])] == [4, 4, 4, 4]
